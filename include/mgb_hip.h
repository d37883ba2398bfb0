/* mgb_hip.h -- C ABI of libmgb_hip.so, the MI355X-native multigrid-barrier Newton path.
 *
 * Drop-in boundary for the distributed path of sloisel/MultiGridBarrierMPI.jl: each entry point
 * names the reference interface it replaces (file:line relative to the reference repository,
 * src = src/MultiGridBarrierMPI.jl).  All functions return 0 on success or a negative MGB_E_* code;
 * mgb_last_error() returns the message of the last failure on the calling thread.  Nothing throws
 * or aborts across this boundary.  The library owns all device memory behind opaque handles; the
 * caller owns every host buffer.  One host thread drives one context; calls are not re-entrant
 * per context (mirrors "all functions are collective", docs/src/guide.md:63-81).
 *
 * Matrices cross the boundary as CSR with Int32 indices (0-based) and fp64 values -- the layout of
 * the local row block of an HPCSparseMatrix (test/test_dump_matrices.jl:62-71; Ti=Int32 src:260).
 * Dense n x k matrices are row-major unless stated; `z` is the Julia `vec` of the n x S state matrix
 * (column-major, [u; s]).
 */
#ifndef MGB_HIP_H
#define MGB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGB_OK 0
#define MGB_E_ARG (-1)      /* bad argument / unknown name / shape mismatch */
#define MGB_E_HIP (-2)      /* HIP runtime failure, or no GPU visible (there is no CPU fallback) */
#define MGB_E_NUMERIC (-3)  /* solver breakdown: non-SPD Hessian, infeasible start, kappa collapse */
#define MGB_E_INTERNAL (-4)

typedef struct mgb_ctx_s* mgb_ctx;   /* device + stream; replaces the HPCBackend instance (src:84-114) */
typedef struct mgb_geo_s* mgb_geo;   /* native Geometry (host); fields of src:318-330 */
typedef struct mgb_amg_s* mgb_amg;   /* AMG hierarchy + barrier problem resident in HBM */
typedef struct mgb_vec_s* mgb_vec;   /* device fp64 vector  == HPCVector.v (src:175) */
typedef struct mgb_csr_s* mgb_csr;   /* device CSR          == HPCSparseMatrix local block (src:216-221) */
typedef struct mgb_locator_s* mgb_locator;   /* point locator of a geometry, device resident (interpolation) */

const char* mgb_last_error(void);
int mgb_version(void);
/* number of visible HIP devices (0 when there is no GPU); never fails */
int mgb_device_count(void);

/* ---- context ------------------------------------------------------------------------------- */
int mgb_ctx_create(int device_id, mgb_ctx* out);
int mgb_ctx_destroy(mgb_ctx ctx);
int mgb_ctx_synchronize(mgb_ctx ctx);
/* Row-block sharding over `world` ranks (one process + one GPU + one mgb_ctx per rank); replaces the
 * reference's MPI.COMM_WORLD (src:125) + HPCSparseArrays row partition (src:216-221, 259-338).  Every rank
 * uploads the WHOLE geometry; an AMG created on a sharded context keeps the element-aligned row block
 * mgb_shard_rows() assigns to its rank (x, w, z, Dz, c, the barrier kernels and the rows of every operator),
 * replicates the Newton unknowns and the factorisation, and calls `fn` (sum-allreduce of `count` doubles, in
 * place at a device pointer) for the gradient, the Hessian values and the scalar reductions.  The callback is
 * entered with the context stream idle and must return with the result visible to it (e.g. RCCL
 * ncclAllReduce + stream sync, MPI_Allreduce on GPU-aware MPI, torch.distributed.all_reduce).  world == 1
 * (default) never calls it. */
typedef int (*mgb_allreduce_fn)(void* user, double* dev_ptr, long long count);
int mgb_ctx_set_comm(mgb_ctx ctx, int rank, int world, mgb_allreduce_fn fn, void* user);
/* The same sharding with a communicator the LIBRARY owns (RCCL over xGMI; the reference's collectives are in-library too,
 * src:125,132): rank 0 calls mgb_rccl_unique_id (128 bytes) and hands the id to the other ranks by whatever channel the host
 * has (MPI_Bcast, torch.distributed broadcast, a file); every rank then calls mgb_ctx_set_comm_rccl -> ncclCommInitRank.  All
 * collectives of the Newton path become ncclAllReduce calls enqueued on the context stream: no host synchronisation around
 * them and no callback into the host language.  librccl is opened at run time (MGB_RCCL_LIB overrides the name); MGB_E_HIP if
 * it cannot be opened.  world == 1 is allowed (one-rank communicator; mgb_vec_allreduce_sum then runs through RCCL). */
int mgb_rccl_unique_id(char* out128);
int mgb_ctx_set_comm_rccl(mgb_ctx ctx, const char* unique_id128, int rank, int world);
int mgb_ctx_comm_stats(mgb_ctx ctx, long long* calls, double* bytes);
int mgb_shard_rows(int rank, int world, int n, int block, int* r0, int* r1);

/* ---- native geometry (host, setup time) ---------------------------------------------------- *
 * fem1d / fem2d are MultiGridBarrier's geometry builders, called at src:561 and src:628 before
 * native_to_mpi.  K: 3m x 2 row-major coarse triangle vertices or NULL for the default square. */
int mgb_fem1d_native(int L, mgb_geo* out);
int mgb_fem2d_native(int L, const double* K, int nK_rows, mgb_geo* out);
/* fem3d (called at src:698): Q_k hexahedra on the default cube, k = 1..3 (reference default k = 3, src:682-684) */
int mgb_fem3d_native(int L, int k, mgb_geo* out);
/* A Geometry assembled by the caller (native_to_mpi input, src:259-302): create, then add matrices.
 * names: "op:<key>" (n x n), "sub:<key>:<level>" (n x m_l, level 0 = coarsest),
 *        "refine:<level>", "coarsen:<level>".  block = rows per element (1 if unknown). */
int mgb_geo_create(int n, int dim, int L, int block, const double* x, const double* w, mgb_geo* out);
int mgb_geo_set_matrix(mgb_geo g, const char* name, int rows, int cols, const int32_t* rowptr,
                       const int32_t* colidx, const double* vals);
int mgb_geo_destroy(mgb_geo g);
int mgb_geo_dims(mgb_geo g, int* n, int* dim, int* L, int* block);
int mgb_geo_get_xw(mgb_geo g, double* x, double* w);          /* mpi_to_native(geometry), src:355-407 */
int mgb_geo_matrix_info(mgb_geo g, const char* name, int* rows, int* cols, int* nnz);
int mgb_geo_matrix_get(mgb_geo g, const char* name, int32_t* rowptr, int32_t* colidx, double* vals);

/* ---- device vectors / sparse matrices: the array algebra MultiGridBarrier applies - */
int mgb_vec_create(mgb_ctx ctx, int n, const double* host_or_null, mgb_vec* out);  /* HPCVector(v, backend) src:268; amgb_zeros src:116 */
int mgb_vec_free(mgb_vec v);
int mgb_vec_len(mgb_vec v, int* n);
int mgb_vec_upload(mgb_vec v, const double* host);
int mgb_vec_download(mgb_vec v, double* host);                /* Vector(x) gather, src:360; _to_cpu_array src:183-188 */
int mgb_csr_create(mgb_ctx ctx, int rows, int cols, const int32_t* rowptr, const int32_t* colidx,
                   const double* vals, mgb_csr* out);         /* HPCSparseMatrix(S, backend) src:271 */
int mgb_csr_free(mgb_csr A);
int mgb_csr_dims(mgb_csr A, int* rows, int* cols, int* nnz);
int mgb_csr_get(mgb_csr A, int32_t* rowptr, int32_t* colidx, double* vals);   /* SparseMatrixCSC(x) gather, src:371,381 */
/* setup-time sparse algebra MultiGridBarrier applies to M; structural patterns (entries that cancel to 0 are
 * kept: the reference hit a cancellation-dependent sparsity bug, test/test_matrix_addition.jl:21-24).  The symbolic
 * work runs on the host copy of the operands (setup, not the Newton path); the result is device resident. */
int mgb_csr_spgemm(mgb_csr A, mgb_csr B, mgb_csr* out);        /* M*M, M'*M  test/test_basic_ops.jl:39,55; test_nonsquare.jl:83 */
int mgb_csr_transpose(mgb_csr A, mgb_csr* out);                /* materialize_transpose, test/test_transpose_only.jl:38,58 */
int mgb_csr_add(mgb_csr A, double alpha, mgb_csr B, mgb_csr* out);  /* M + alpha*M  test/test_matrix_addition.jl:48-63; scalar*M tools/profile_ops.jl:117 */
int mgb_csr_hcat(int count, const mgb_csr* mats, mgb_csr* out);     /* hcat(M...)  test/test_d0_construction.jl:92-100 */
int mgb_csr_blockdiag(int count, const mgb_csr* mats, mgb_csr* out); /* amgb_blockdiag src:150; test/test_helpers.jl:117-121 */
int mgb_diag(mgb_ctx ctx, mgb_vec z, int m, int n, mgb_csr* out);  /* amgb_diag: spdiagm(m,n,0=>z) src:137-147 */
int mgb_spmv(mgb_csr A, mgb_vec x, mgb_vec y);                /* y = A*x   (HPCSparseMatrix * HPCVector, test_nonsquare.jl:43) */
int mgb_spmv_add(mgb_csr A, mgb_vec x, mgb_vec y0, mgb_vec y); /* y = y0 + A*x */
int mgb_dot(mgb_vec x, mgb_vec y, double* out);               /* dot(w,y) tools/profile_scaling.jl:102 */
int mgb_norm(mgb_vec x, double* out);                         /* norm(x) (2-norm) tools/profile_scaling.jl:89-134 */
int mgb_sum(mgb_vec x, double* out);                          /* sum(x) tools/profile_barrier.jl:45-59,95-114 */
/* out[q] = M[q*K + k] of a row-major n x K device matrix: y[:, j] -> HPCVector, test/test_column_extract.jl:50 */
int mgb_col_extract(mgb_vec M, int n, int K, int k, mgb_vec out);
/* map_rows / map_rows_gpu (src:161-170) for the closures MultiGridBarrier derives from a convex set -- the only closures the
 * Newton path ever maps: which = 0: out[q] = F(Dz_q) (n values, +inf outside the set); 1: out = F1 rows (n x K, row-major);
 * 2: out = F2 rows flattened to K*K columns (n x K*K; column j*K + k, test/test_map_rows_compare.jl:73).  The set is described
 * as in mgb_amg_create_terms; Dz is an n x K row-major device matrix.  Any other closure has no device form: the host side
 * evaluates it on a device -> host copy (the reference's _to_cpu_array trade, src:183-188). */
int mgb_map_rows_barrier(int which, int K, int nterms, const int* kind, const int* nq, const int* idx_q, const int* idx_s,
                         const int* idx_s2, const double* p, const double* coef, const double* off, int n, mgb_vec Dz,
                         mgb_vec out);
int mgb_mul(mgb_vec x, mgb_vec y, mgb_vec out);               /* w .* col, test_column_extract.jl:65 */
int mgb_axpy(mgb_vec x, double alpha, mgb_vec y, mgb_vec out); /* out = x + alpha*y */
int mgb_vec_allreduce_sum(mgb_vec x);                         /* sum over the ranks of a sharded context (no-op for world 1); MPI.Allreduce src:125 */
int mgb_all_isfinite(mgb_vec x, int* out);                    /* amgb_all_isfinite src:121-133 */

/* ---- AMG + barrier problem ------------------------------------------------------------------ *
 * state_vars: S pairs "name\0subspace\0" flattened as 2*S C strings; D: K pairs (state var, operator)
 * (amg(geometry; state_variables, D): layout test/test_d0_construction.jl:82-100).
 * Barrier: power cone {(q,s): s >= |q|^p} on D rows idx_q[0..nq) and idx_s (convex_Euclidian_power).
 * Uploads the geometry to HBM (the native_to_mpi step, src:259-338); levels are built on first use. */
int mgb_amg_create(mgb_ctx ctx, mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D,
                   int nq, const int* idx_q, int idx_s, double p, mgb_amg* out);
/* Barrier of an intersection of 1 or 2 power cones (upstream `intersect` of convex_Euclidian_power sets, as
 * used by parabolic_solve: s1 >= u^2 and s2 >= |grad u|^p).  nq[c], idx_q[3*c + i], idx_s[c], p[c] per cone;
 * idx_s2 (nullable) names an extra D row added to the cone's slack (feasibility phase), -1 for none.
 * The rows a cone names -- idx_q[3*c .. 3*c + nq[c]), idx_s[c] and idx_s2[c] -- must be distinct (MGB_E_ARG otherwise, here and
 * in mgb_amg_create / mgb_amg_create_terms / mgb_map_rows_barrier): the Hessian keeps one off-diagonal slot per pair of them. */
int mgb_amg_create_cones(mgb_ctx ctx, mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D,
                         int ncones, const int* nq, const int* idx_q, const int* idx_s, const int* idx_s2,
                         const double* p, mgb_amg* out);
/* General barrier menu: an intersection of 1 to 3 convex sets (upstream `intersect`), term c being
 *   kind[c] = 0: the power cone above (nq[c], idx_q[3c + i], idx_s[c], idx_s2[c] (nullable array), p[c]);
 *   kind[c] = 1: the half space  sum_i coef[3c + i] * Dz[:, idx_q[3c + i]] + off[c] > 0,  i < nq[c] <= 3  (upstream
 *                convex_linear with one constant row: bounds and constant obstacles), barrier -log of the affine form;
 *                idx_s[c], p[c] ignored.
 * coef / off may be NULL when every term is a power cone. */
int mgb_amg_create_terms(mgb_ctx ctx, mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D,
                         int nterms, const int* kind, const int* nq, const int* idx_q, const int* idx_s, const int* idx_s2,
                         const double* p, const double* coef, const double* off, mgb_amg* out);
/* x-dependent exponent p(x) of power-cone term `term` (upstream convex_Euclidian_power with a function p):
 * p_nodes[q] = p(x_q) >= 1 at the n (global) nodes; the barrier kernels then use a = 2 / p(x_q) and mu(p(x_q)) per node.
 * Call after mgb_amg_create*, before the first evaluation. */
int mgb_amg_set_exponents(mgb_amg a, int term, const double* p_nodes);
/* upstream convex_piecewise (a convex set that varies in space: at x the intersection of the pieces selected there;
 * [UPSTREAM-UNVERIFIED] semantics): mask[q * nterms + c] != 0 iff barrier term c is active at node q (n
 * global nodes x the terms of mgb_amg_create_terms); an inactive term contributes nothing at that node.  Every node must keep at
 * least one term.  Call after mgb_amg_create*, before the first evaluation; the start must be strictly feasible. */
int mgb_amg_set_term_mask(mgb_amg a, const unsigned char* mask);
int mgb_amg_destroy(mgb_amg a);
int mgb_amg_dims(mgb_amg a, int* n, int* S, int* K, int* L, int* nY);   /* n = LOCAL rows on a sharded context */
int mgb_amg_local_rows(mgb_amg a, int* n_global, int* row0, int* n_local);
/* levels (operators, Hessian plan) are built on first use and the factorisation structures on the first solve;
 * mgb_amg_prepare builds both now for `level` (-1: every level the current schedule visits), so that the next
 * mgb_amg_solve is pure compute */
int mgb_amg_prepare(mgb_amg a, int level);
int mgb_amg_level_size(mgb_amg a, int level, int* N, int* nnz_lower);
/* device factorisation of `level` (built now if needed): *split_world = ranks it is split over by nested-dissection subtrees
 * on a sharded context (1 = replicated: single GPU, or a world the tree cannot be split into), doubles exchanged per Newton
 * system (subtree-root Schur complements + the assembled solution), kernel launches per Newton system */
/* Float32 evaluation of f0 / f1 / f2 at a level (the reference runs Float32 on its Metal backend, test/test_utils.jl:67-88;
 * SURVEY.md section 8 f3): the SpMV and barrier kernels instantiated for float -- float operators, weights, costs and vectors
 * are shadows of the double ones, built on first use -- with s in / g, lower_vals out as float; f0 is summed in double from
 * per-row float terms.  Single-GPU contexts.  There is no Float32 factorisation (fp64 runs at the fp32 vector rate on MI355X
 * and the direct solve is latency-bound): mgb_amg_solve stays in double.  *_template_f64: the double instantiation of the
 * same kernel templates, which must reproduce mgb_amg_f1 / f2 bit for bit (that is how the tests tie the float kernels to
 * the production ones). */
int mgb_amg_f0_f32(mgb_amg a, int level, const float* s, float t, double* f0);
int mgb_amg_f1_f32(mgb_amg a, int level, const float* s, float t, float* g);
int mgb_amg_f2_f32(mgb_amg a, int level, const float* s, float t, float* lower_vals);
int mgb_amg_f1_template_f64(mgb_amg a, int level, const double* s, double t, double* g);
int mgb_amg_f2_template_f64(mgb_amg a, int level, const double* s, double t, double* lower_vals);
/* The line search's speculated objective on the buffers a solve uses (tests): the na (1..3) points x_a = s + alpha[a] * nstep
 * (nstep nullable: x_a = s), with the fraction-to-the-boundary rule against phi_ref (n x nterms, nullable: no rule).
 * mode 0: one fused launch for all points; 1: one fused launch per point; 2: the unfused path (x_a, apply_D, objective) per point.
 * sums_host / sums_dev [2 na]: per point (sum w F, sum w <c, Dz>) as the kernels left them in pinned host memory and as
 * copied from the device; s_out [na x N], dz [na x n x K], phi [na x n x nterms].  Single-GPU contexts. */
int mgb_amg_trial_set(mgb_amg a, int level, const double* s, const double* nstep, int na, const double* alpha,
                      const double* phi_ref, int mode, double* sums_host, double* sums_dev, double* s_out, double* dz,
                      double* phi);
int mgb_amg_chol_info(mgb_amg a, int level, int* split_world, double* exchange_doubles, int* launches);
/* the launch chain of that factorisation (built now if needed; read-only: no numerics or launches change), in launch order:
 * *nlaunch launches, the kind code and the workgroup count of the first min(cap, *nlaunch).  Kind codes (GpuChol::Kind):
 *   0 Leaf  1 Single  2 SingleNarrow  3 SingleDense  4 SingleDenseNarrow  5 Start  6 Step  7 Step2  8 Panel2  9 Update2
 *   10 BwdRect  11 Bwd256  12 Bwd1024  13 BwdFused
 * unknown_node / unknown_col (nullable, N entries each): per unknown of the original ordering its tree node (postorder, as
 * mgb_amg_chol_tree) and its column among that node's own columns (0 .. ns - 1).  kind / workgroups may be null.  A launch
 * listed with no workgroup (the first launch of a height whose fronts have no row: the root of a disconnected domain) is never
 * issued. */
int mgb_amg_chol_schedule(mgb_amg a, int level, int cap, int* nlaunch, int* kind, int* workgroups, int* unknown_node,
                          int* unknown_col);
/* pre-mapped child contributions of that chain (MGB_CHOL_PREMAP; nullable outputs), per launch of the first
 * min(cap, launches) in the order of mgb_amg_chol_schedule: consumer = 1 if the launch reads its fronts' contribution slabs
 * instead of gathering through the index maps, producers = how many of its fronts store their Schur complement into their
 * parent's slab; *slab_bytes = device memory of the slabs */
int mgb_amg_chol_premap(mgb_amg a, int level, int cap, int* consumer, int* producers, double* slab_bytes);
/* the elimination tree of that factorisation in postorder (children first): own size, front size and parent (-1 = root)
 * of the first min(cap, *nnodes) nodes -- mgb_plan_chol_tree for the level as the device factors it */
int mgb_amg_chol_tree(mgb_amg a, int level, int cap, int* nnodes, int* ns, int* nf, int* parent);
/* *yes = 1 if the subtrees of the split follow the row partition: a rank's Hessian values are then used where they were
 * computed, only the entries among separator unknowns are summed (inside the Schur-complement collective, counted in
 * exchange_doubles), and the allreduce of all nnz values per Newton step is gone (MGB_RANK_ALIGNED=0 restores it) */
int mgb_amg_chol_values_local(mgb_amg a, int level, int* yes);
int mgb_amg_hessian_pattern(mgb_amg a, int level, int32_t* rowptr, int32_t* colidx);  /* lower triangle of R'HR */
int mgb_amg_set_c(mgb_amg a, const double* c);     /* n x K row-major cost (f_grid) */
int mgb_amg_set_z(mgb_amg a, const double* z);     /* S*n, [u; s] */
int mgb_amg_get_z(mgb_amg a, double* z);           /* mpi_to_native(sol).z, src:422-474 */
int mgb_amg_get_c(mgb_amg a, double* c);           /* the cost as the device holds it, n x K row-major (local rows); waits for the stream */
/* barrier(F).f0/f1/f2 at level `level`, subspace coordinates s (N_l host values), parameter t:
 *   f0: test/test_apply_d.jl:44 + tools/profile_barrier.jl:45-59; parts = {sum w F, sum w c.Dz}
 *   f1: test/test_column_extract.jl:50-80;  f2: test/test_map_rows_compare.jl:102-123,165-170 */
int mgb_amg_apply_D(mgb_amg a, int level, const double* s, double* Dz /* n x K */);
int mgb_amg_f0(mgb_amg a, int level, const double* s, double t, double* y, double* parts2);
/* line-search trial (amgb_all_isfinite semantics, src:121-133, plus the fraction-to-the-boundary rule):
 * y = f0(s) if every row keeps >= 10 % of the cone distance it has at s_ref, else +inf */
int mgb_amg_f0_trial(mgb_amg a, int level, const double* s_ref, const double* s, double t, double* y);
int mgb_amg_f1(mgb_amg a, int level, const double* s, double t, double* g);
int mgb_amg_f2(mgb_amg a, int level, const double* s, double t, double* lower_vals);
/* MultiGridBarrier.solve(A, b) = A \ b (test/test_instrumented_solve.jl:25-28,99), host direct solve */
int mgb_amg_solve_linear(mgb_amg a, int level, const double* lower_vals, const double* g, double* x);
/* the same solve with the device multifrontal Cholesky (csrc/gpuchol.hip): the solver the Newton loop uses
 * by default.  Returns MGB_E_NUMERIC if a pivot is not positive. */
int mgb_amg_solve_linear_gpu(mgb_amg a, int level, const double* lower_vals, const double* g, double* x);
/* The owner-local pieces of a sharded Newton step, one call each, through the functions the solve itself calls (tests).
 * Inside a solve on a sharded context whose factorisation keeps its values local (mgb_amg_chol_values_local) the Newton
 * vectors are valid on a rank's own unknowns and on the replicated top only; the entry points above take the
 * allreduce-everything branches instead.  MGB_E_ARG on an unsharded context ("sharded contexts only") and on a level whose
 * values are summed over the ranks.  Collective: every rank calls them in the same order.
 *   f1_owner: g [N] = the gradient as the device holds it, complete where kind >= 1 (top entries summed over the ranks: the
 *     one collective of ntop + 1 doubles); *gg = |g|^2 summed over the owners, as the device produced it; kind [N] per
 *     unknown: 0 = interior of another rank's subtree, 1 = of this rank's, 2 = top (separator).  gg, kind nullable.
 *   f2_local: this rank's contributions to the Hessian values (lower triangle, pattern order), before any reduction.
 *   solve_linear_local: local_vals = this rank's contributions to the matrix, g valid where kind >= 1.  x [N] = the solution
 *     where kind >= 1, zero elsewhere; *inc = <g, x> and *flag (1 = a pivot was not positive on some rank, else 0) as the
 *     step's one scalar collective left them -- a non-positive pivot is RETURNED, never MGB_E_NUMERIC, so the ranks stay in
 *     lock step; vals_after [nnz] = the values buffer behind the solve (entries among top unknowns <- their sums over the
 *     ranks, every other entry untouched).  inc, flag, vals_after nullable. */
int mgb_amg_f1_owner(mgb_amg a, int level, const double* s, double t, double* g, double* gg, int32_t* kind);
int mgb_amg_f2_local(mgb_amg a, int level, const double* s, double t, double* lower_vals);
int mgb_amg_solve_linear_local(mgb_amg a, int level, const double* local_vals, const double* g, double* x, double* inc,
                               int* flag, double* vals_after);
/* Newton linear solver: 0 (default) = GPU multifrontal Cholesky, 1 = host multifrontal Cholesky, 2 = conjugate gradients
 * preconditioned by a V-cycle over the AMG levels, H applied matrix-free (single-GPU contexts; see the multigrid block below) */
int mgb_amg_set_solver(mgb_amg a, int solver);
/* amgb_step level schedule: 0 (default) = Newton on the finest subspace only, 1 = literal coarse -> fine
 * level loop (R_1 ... R_L).  Both end at the same z; see DESIGN.md section 2. */
int mgb_amg_set_schedule(mgb_amg a, int all_levels);
/* end of the t-continuation: 0 (default) = at the fixed t_stop = the first value of t0 kappa^k beyond 1/tol, the last step
 * clipped to land on it (the end point, and z to ~1e-6 at p = 1, then no longer hangs on the history of kappa reductions);
 * 1 = the literal loop of SURVEY.md Appendix A, `while t <= 1/tol: t <- kappa t`.  Neither is confirmed by anything in the
 * reference ([UPSTREAM-UNVERIFIED]; SOL_main.ts is an observable, docs/src/api.md:97-101); both visit the same ts when kappa is
 * never reduced. */
int mgb_amg_set_stop_rule(mgb_amg a, int upstream);
/* Newton's stopping rule on the finest level at the intermediate t: 1 (default) = stagnation of the objective at every t; 0 = stop
 * once the Newton decrement <g, n> is below 0.01 min w -- the path is followed, not resolved -- and keep the stagnation rule for the
 * last t, whose centre is the answer.  Same end point; 15-17 % fewer Newton steps at p = 1.5 / in 3-D, but MORE at p = 1 (fem2d
 * L=7: 466 -> 580), hence the default.  A phase with mgb_amg_set_early_stop resolves every centre.  [UPSTREAM-UNVERIFIED] like
 * every stopping constant (oracle CENTERING). */
int mgb_amg_set_centering(mgb_amg a, int exact);
/* amgb main phase: t-continuation x level loop x Newton; z updated in place */
int mgb_amg_solve(mgb_amg a, double tol, double t0, double kappa, int maxit, int max_newton, int verbose);
/* 1 (default): later solves bracket the kernels of every 8th Newton step with HIP events and time the factorisation chain on
 * another 8th (mgb_amg_sol_kernels, time_factor); those steps go out as plain launches.  0: no timing, every eligible step is
 * one replayed graph.  Same kernels, same arguments, same values either way. */
int mgb_amg_set_time_kernels(mgb_amg a, int on);
/* Newton trace of the later solves ("Newton trace"): max_steps = 0 (default) turns it off; else a solve records every
 * newton() call and every Newton step, and one that needs more than max_steps steps fails with MGB_E_ARG (before anything is
 * launched when max_steps is below the Newton budget of one centering, else before the step that does not fit).  keep_vectors:
 * also the vectors, copied back behind a stream synchronisation per copy.  Tracing changes no launch and no argument.
 * A solve that fails, for this or any other reason, leaves z partly advanced (as every failed solve does) and a partial
 * trace: the centerings and steps recorded up to the failure.
 * trace_info: centerings and steps recorded by the last solve, doubles in `vectors`.
 * trace_get (each pointer nullable): centerings = ncentering rows of 9 doubles: level, t, finest, final, Newton budget, k reached,
 *   converged, index of its first step, its steps; steps = nsteps rows of 14 doubles: centering, y, |g|, ymin, gmin before the
 *   step, inc = <g, n>, accepted step length (0: rejected), y and |g| after, pivot flag, launch mode (0 graph replay, 1 graph
 *   capture, 2 plain sampled, 3 plain timed chain, 4 pcg, 5 pcg fallback, 6 host solver, 7 sharded, 8 plain untimed), bit mask of
 *   the speculated results (steps 1, 1/2, 1/4) consumed, further objective evaluations launched, reason the loop ended (0 none,
 *   1 inc <= 0, 2 decrement rule, 3 stagnation rule, 4 budget, 5 pivot failure, 6 non-finite decrement); vectors, in the order of
 *   recording: per centering Dz0 (n x K), then per step s before it (N), nstep (N), s (N) and Dz (n x K) after it. */
int mgb_amg_set_trace(mgb_amg a, int max_steps, int keep_vectors);
int mgb_amg_trace_info(mgb_amg a, int* ncentering, int* nsteps, long long* nvec);
int mgb_amg_trace_get(mgb_amg a, double* centerings, double* steps, double* vectors);
/* feasibility phases (SOL_feasibility, src:428-455): make mgb_amg_solve return after the first centering at which row `col`
 * of D z -- the slack of a relaxed problem -- is negative at every node, instead of following the path to t = 1/tol.
 * col = -1 (default): off. */
int mgb_amg_set_early_stop(mgb_amg a, int col);
/* SOL_main fields (docs/src/api.md:97-101) of the last mgb_amg_solve */
int mgb_amg_sol_info(mgb_amg a, int* nt, double* t_elapsed, double* time_factor, long long* counts4);
int mgb_amg_sol_get(mgb_amg a, long long* its /* L x nt col-major */, double* ts, double* c_dot_Dz);
/* live HIP-event timing of the 11 kernel classes accumulated over the last mgb_amg_solve (event pairs
 * recorded on the context stream around single launches, on every 8th Newton step -- bracketing every launch
 * costs ~14 % of a solve): total ms, total algorithmic bytes, launches timed;
 * order = apply_D, barrier_f2, hessian_assemble, barrier_f1, restrict, barrier_f0,
 *         chol_front_start, chol_front_step, chol_backward_rect, chol_backward, chol_front_single */
int mgb_amg_sol_kernels(mgb_amg a, double* ms11, double* bytes11, long long* launches11);
/* per-kernel device timings (HIP events on the context stream around `reps` back-to-back launches, rotating over `nrot`
 * distinct copies of every operand so that a working set of nrot x bytes beyond the 256 MiB Infinity Cache is read from
 * HBM), ms and algorithmic bytes per launch:
 * order = apply_D (as the solve runs it: through the element-local view of B on bandwidth-bound meshes), barrier_f2,
 * hessian_assemble, barrier_f1, restrict, barrier_f0, trial_f0 (the fused trial point + apply_D + barrier_f0 launch of
 * launch-bound meshes), apply_D through the plain CSR kernel; bytes8[7] = 1 if slot 0 used the element-local view */
int mgb_amg_time_kernels(mgb_amg a, int level, int reps, int nrot, double* ms8, double* bytes8);

/* ---- time loop of parabolic_solve: the transition between two barrier solves, on the device (docs/src/guide.md "Time-Dependent
 * (Parabolic) Problems"; time-dependent closures f1(t, x), g(t, x) are [UPSTREAM-UNVERIFIED], the contract is this project's) -- *
 * For an AMG with the parabolic layout: S = 3 state variables [u; s1; s2] (z column-major), K = dim + 3 rows of D = (u id,
 * u dx.., s1 id, s2 id), cones s1 >= u^2 and s2 >= |grad u|^p.  Single-GPU contexts.
 * mgb_amg_parabolic_begin: bidx = the nb nodes whose u is Dirichlet data (the empty rows of the finest `dirichlet` subspace),
 * kept on the device.  MGB_E_ARG -- before anything is launched -- on another layout, a sharded context, nb < 0 or an index
 * outside [0, n).
 * mgb_amg_parabolic_step: from t_k to t_{k+1} = t_k + h (finite h > 0, p >= 1), enqueued on the context stream in this order:
 *   1. cost       c[i, 0] = f_nodes[i] - u[i] / h with the OLD u (a division, then a subtraction: bitwise what fp64 numpy gives for
 *                 f - u / h), c[i, K-2] = 1 / (2h), c[i, K-1] = 1 / p (host scalars), 0 elsewhere;
 *   2. boundary   u[bidx[j]] = gb[j] (gb null: kept); interior u, s1, s2 untouched;
 *   3. violations Dz0 = D z, then v1 = max_i (u_i^2 - s1_i), v2 = max_i ((sum_d g_id^2)^(p/2) - s2_i), g = columns 1..dim of
 *                 Dz0; a node with a non-finite u, g, s1 or s2 makes both maxima NaN (never dropped);
 *   4. lift       lift_j = 1 + v_j if v_j >= 0, else exactly 0;  s_j += lift_j at every node (a constant shift, the closed-form
 *                 feasibility phase of amgb); a column whose lift is 0 is not written; Dz0 = D z again.
 * f_nodes (n) and gb (nb) are device vectors of the AMG's context.  lift2 null: the call does not wait for the device;
 * non-null: as mgb_amg_parabolic_lifts.  The next mgb_amg_solve starts from this state.
 * mgb_amg_parabolic_lifts: waits for the stream; (lift_1, lift_2) of the last step; MGB_E_NUMERIC if one is not finite.
 * mgb_amg_snapshot: one launch, out[i * S + s] = z[s * n + i] (row-major n x S, the layout of an HPCMatrix); out is a device
 * vector of n * S values owned by the caller; no host wait. */
int mgb_amg_parabolic_begin(mgb_amg a, int nb, const int32_t* bidx);
int mgb_amg_parabolic_step(mgb_amg a, double h, double p, mgb_vec f_nodes, mgb_vec gb_or_null, double* lift2_or_null);
int mgb_amg_parabolic_lifts(mgb_amg a, double* lift2);
int mgb_amg_snapshot(mgb_amg a, mgb_vec out);

/* ---- multigrid pieces: SURVEY.md section 8 row a11 / 8(b) `mgb_hessian_apply / mgb_smooth / mgb_prolong / mgb_restrict` ------ *
 * The reference has no smoother: its "multigrid" is Newton on the nested subspaces R_l with MultiGridBarrier.solve -> MUMPS per
 * level (test/test_instrumented_solve.jl:25-28,99; README.md:23).  BASELINE.json's north star asks for prolongation /
 * restriction / smoother on the GPU; they replace nothing one-to-one and serve solver 2 above, which solves the SAME Newton
 * system H n = g (H = R_l' (sum_jk D_j' diag(w y_jk) D_k) R_l, test/test_map_rows_compare.jl:102-123,165-170) iteratively.
 * All take host arrays like mgb_amg_f1 / f2; `s` = the point (N_l subspace coordinates) whose Hessian is meant. */
/* Hv = H(s) v at `level`.  matrix_free != 0: B' (Y o (B v)) element by element -- the element's v and Y staged in LDS, the
 * per-node K x K block applied in registers between the two halves (csrc/mg.hip: elop_apply_kernel); 0: through the assembled
 * matrix (full symmetric CSR).  Both must agree with mgb_amg_f2's matrix times v. */
int mgb_hessian_apply(mgb_amg a, int level, const double* s, const double* v, double* Hv, int matrix_free);
/* `sweeps` Chebyshev-Jacobi passes on H(s) x = b from the given x (in/out), each `degree` (1..7) applications of H; eigenvalue
 * interval [lo, hi] * lambda with lambda = lmax if lmax > 0, else lambda_max(Dinv H) estimated on the device (power steps in the
 * D inner product); *lmax_used (nullable) = the lambda the coefficients were built from. */
int mgb_smooth(mgb_amg a, int level, const double* s, const double* b, double* x, int degree, int sweeps, double lmax,
               int matrix_free, double* lmax_used);
/* transfer between the unknowns of level and level + 1 (R_level = R_{level+1} P): xf = P xc, rc = P' rf */
int mgb_prolong(mgb_amg a, int level, const double* xc, double* xf);
int mgb_restrict(mgb_amg a, int level, const double* rf, double* rc);
/* P of `level` as CSR: sizes first (null arrays), then the arrays */
int mgb_amg_prolongation(mgb_amg a, int level, int* rows, int* cols, int* nnz, int32_t* rowptr, int32_t* colidx, double* vals);
/* x = H(s)^{-1} g by the V-cycle-preconditioned CG the Newton loop runs with solver 2; *converged = 0 if it stopped at maxit */
int mgb_amg_pcg_solve_linear(mgb_amg a, int level, const double* s, const double* g, double* x, int* iters, double* relres,
                             int* converged);
/* tests: lambda_max(Dinv A) of `level` for every later V-cycle setup (mgb_amg_vcycle, mgb_amg_pcg_solve_linear, solver 2) in place
 * of the device's warm-started estimate; 0 unpins (the default); a negative or non-finite value is an argument error */
int mgb_amg_mg_pin_lmax(mgb_amg a, int level, double lmax);
/* x = V(b): one V-cycle of the preconditioner of solver 2 at the Hessian H(s) of level `top`, enqueued exactly as CG enqueues it
 * (single-GPU contexts; the parameters of mgb_amg_set_pcg apply); lmax_used[l] (one double per level of the hierarchy) = the
 * lambda the Chebyshev coefficients of level l were built from, for the levels above the coarsest one of the cycle, 0 elsewhere */
int mgb_amg_vcycle(mgb_amg a, int top, const double* s, const double* b, double* x, double* lmax_used);
/* CG / V-cycle parameters (a value <= 0, or < 0 for the two flags, keeps the current one): relative tolerance on
 * sqrt(<r, M r>), iteration cap, applications of H per Chebyshev pre-/post-smoothing, power steps per level and Newton matrix,
 * Chebyshev interval fractions, CG iterations enqueued between two looks at the convergence flag, direct solve of a step whose
 * CG did not converge, top level through its assembled matrix instead of the matrix-free product, consecutive non-converged
 * systems after which the rest of the solve goes to the direct solver (0 = keep trying) */
int mgb_amg_set_pcg(mgb_amg a, double rtol, int maxit, int degree, int power_its, double lo_frac, double hi_frac, int chunk,
                    int fallback, int assembled_top, int giveup);
/* of the last mgb_amg_solve with solver 2: counts4 = {Newton systems CG was tried on, CG iterations, direct fallbacks, the
 * Newton system after which the solve went to the direct solver for good (-1: never)}, seconds inside CG */
int mgb_amg_sol_pcg(mgb_amg a, long long* counts4, double* time_s);
/* HIP-event timing of the multigrid kernels at `level` (the Hessian of the current z), `reps` back-to-back launches rotating
 * over `nrot` distinct copies of the operands (as mgb_amg_time_kernels), ms / bytes moved by construction / algorithmic bytes
 * (the CSR-based figure of SURVEY.md section 8d) per call: [0] H v matrix-free, [1] one Chebyshev step on it, [2] H v through the
 * assembled CSR, [3] prolongation from level - 1, [4] restriction to level - 1, [5] bytes of the unfused CSR sequence for H v */
int mgb_amg_time_mg_kernels(mgb_amg a, int level, int reps, int nrot, double* ms6, double* bytes6, double* alg6);
/* coarsest level of the V-cycle whose top is level `top` (the largest level with at most 128 unknowns; dense inverse there) */
int mgb_amg_mg_info(mgb_amg a, int top, int* coarsest);
/* read-only description of the element operator of `level` (the matrix-free H v and the element-slab assembly), built first if
 * it is not yet.  out[13]: [0] valid (0: the operators are not element-local, or an element does not fit into LDS; the rest is
 * zero then), [1] threads per element (8 .. 256: the kernel instantiation), [2] rows per element, [3] cmax, [4] nnz_max,
 * [5] structure classes, [6] elements, [7] K, [8] nY, [9] 1 if the software-pipelined load path is taken, 0 for the plain one,
 * [10] 1 if the element-slab assembly is valid, [11] workgroups of the apply launch, [12] passes of its busiest workgroup */
int mgb_amg_elop_info(mgb_amg a, int level, int* out);

/* ---- evaluation at arbitrary points (the step after mpi_to_native in the reference's workflow: README.md:42-50,
 * docs/src/guide.md:21-52 plot the solution; [UPSTREAM-UNVERIFIED] `interpolate`, the contract is this project's) --------- *
 * z: nodal values, n x S row-major.  Elements are the row blocks of the geometry: 1-D block 2 (P1), 2-D block 7 (P2 + cubic
 * bubble, rows 3..6 = edge midpoints and centroid of rows 0..2), 3-D block (k+1)^3 (Q_k on the axis-aligned box of the first
 * and last row), k = 1..3; any other element shape is MGB_E_ARG at creation.
 * Containment, in reference coordinates with tau = 1e-12: inside when min(lambda) >= -tau (2-D), every xi_a in
 * [-tau, 1 + tau] (1-D, 3-D); of all elements containing a point the lowest index wins; a point in no element or with a
 * non-finite coordinate is outside: every output column NaN, element -1, no error.
 * The locator uses x, dim, block and n of the geometry alone: a uniform bin grid over the bounding box (about one cell per
 * element, CSR cell -> ascending elements), built on the host, resident on the device together with x and the quadrature
 * weights w (mgb_field_norms). */
int mgb_locator_create(mgb_ctx ctx, mgb_geo g, mgb_locator* out);
int mgb_locator_destroy(mgb_locator loc);
/* one launch on the context stream, one thread per point: pts m x dim, z n x S, vals m x S, grads (nullable) m x S x dim, all
 * row-major device vectors of the locator's context; elem_host_or_null: m element indices copied to the host (the call then
 * waits for the launch).  m = 0 returns at once. */
int mgb_interpolate(mgb_locator loc, int m, mgb_vec pts, int S, mgb_vec z, mgb_vec vals, mgb_vec grads_or_null,
                    int32_t* elem_host_or_null);
/* host restatement (no context, no GPU): the same bins, containment rule and bases on host arrays */
int mgb_geo_interpolate_host(mgb_geo g, int m, const double* pts, int S, const double* z, double* vals,
                             double* grads_or_null, int32_t* elem_or_null);

/* ---- norms and errors of nodal fields by the nodal quadrature rule (the convergence study after a solve) ---------------- *
 * A field is an n x S row-major nodal matrix on a geometry whose elements are its row blocks, as for mgb_interpolate; node i
 * belongs to element e = i / block; integrals are the nodal rule of that geometry, int phi ~ sum_i w_i phi(x_i).  At node i a
 * field is evaluated in its OWN element e, never in a neighbour sharing the point: the value is z[i], the gradient is the
 * physical gradient of e's nodal basis at x_i (what the dx / dy / dz operator rows give).
 * The difference field d = a - r and its gradient are taken at every node of a's geometry; r is exactly one of
 *   nothing:                      d = a, the norms of a itself;
 *   ref_vals (n x S) [, ref_grads (n x S x dim)]:  d_i = a_i - ref_vals_i; with ref_grads grad d_i = grad a(x_i) - ref_grads_i
 *                                 (the exact gradient of an exact solution), without it the element gradient of the nodal
 *                                 field a - ref_vals;
 *   other + z_other (n_other x S): a field on another geometry of the same dimension and element degree, evaluated at x_i by
 *                                 the other mesh's polynomial.  Its element is the one that CONTAINS the nudged point
 *                                 x_i + theta (c_e - x_i), theta = 2^-20, c_e = mean of the nodes of i's own element (the
 *                                 containment rule above: tau, lowest index wins); that element's polynomial and gradient
 *                                 are then evaluated at x_i itself.  The nudge decides on which side of a coarse edge a
 *                                 fine node takes the (discontinuous) coarse gradient: the side its own element lies on.  A
 *                                 node whose nudged point lies in no element of the other mesh contributes nothing to any
 *                                 sum or maximum and is counted in `outside`.  other == loc is allowed.
 * Output: for every column s one row of MGB_NORM_COLS doubles
 *   [0] sum w_i d_i (signed)  [1] sum w_i |d_i|^q  [2] sum w_i |grad d_i|_2^q  [3] max_i |d_i|  [4] max_i |grad d_i|_2
 * -- the raw power sums, not their roots.  q: any finite real >= 1 (q = 2 and q = 1 take no pow; |d| = 0 contributes 0).
 * A non-finite d_i or grad d_i makes the affected entries of THAT column non-finite (a NaN term makes the sum and the
 * maximum NaN, it is never dropped); other columns are unaffected, bit for bit.
 * MGB_E_ARG: a null loc, z or out; S < 1; q not finite or < 1; a vector whose length is not exactly what the shapes above
 * say; ref_grads without ref_vals; both ref_vals and other; other without z_other or z_other without other; other of another
 * context, dimension or element degree. */
#define MGB_NORM_COLS 5
/* two launches on the context stream (partial rows per workgroup and column, then one workgroup that combines them in
 * ascending workgroup order: no atomics, bitwise reproducible); the results are copied to the host and the call waits */
int mgb_field_norms(mgb_locator loc, int S, mgb_vec z, double q, mgb_vec ref_vals_or_null, mgb_vec ref_grads_or_null,
                    mgb_locator other_or_null, mgb_vec z_other_or_null, double* out_host /* S x MGB_NORM_COLS */,
                    long long* outside_host_or_null);
/* host restatement (no context, no GPU): the same per-node routine, summed serially in ascending node order */
int mgb_geo_field_norms_host(mgb_geo g, int S, const double* z, double q, const double* ref_vals_or_null,
                             const double* ref_grads_or_null, mgb_geo other_or_null, const double* z_other_or_null,
                             double* out, long long* outside_or_null);

/* ---- energy, flux and cone margin of p-Laplace solutions (what one reports, plots and monitors after a solve) ------------ *
 * A field is an n x S row-major nodal matrix on the geometry of a locator, as for mgb_field_norms; single-GPU contexts, fp64.
 * At node i, in i's OWN element e = i / block:
 *   g_i  the physical gradient of column u at x_i (what the dx / dy / dz operator rows give),   a_i = |g_i|_2,
 *   p_i  the exponent: the scalar p, or p_nodal[i] where p_nodal (n values) is given (p is then only checked),
 *   P_i  = a_i^p_i  (p = 2 and p = 1 take no pow; 0 at a = 0),   s_i = column s,   f_i = nodal forcing (no f: 0),   w_i the weight.
 * Per field one row of MGB_ENERGY_COLS doubles
 *   [0] sum w P / p       the gradient energy  int (1/p) |grad u|^p
 *   [1] sum w f u         the load             int f u
 *   [2] sum w (s - P) / p the slack gap, summed term by term (it is not the difference of two sums)
 *   [3] max a^(p-1)       the largest flux magnitude; at p = 1 it is 1 where a > 0 and 0 where a = 0
 *   [4] max (P - s)       its negative is the cone margin; a positive value means a node outside the cone
 * A non-finite u_i, s_i, f_i or gradient makes all five contributions of node i NaN, and so does an entry of a DEVICE p_nodal
 * that is not a finite real >= 1 (the host restatement checks its p_nodal and returns MGB_E_ARG).  A NaN term makes its sum
 * and its maximum NaN; it is never dropped and never turned into a maximum.  Other fields of the batch are unaffected, bit for bit.
 * Flux: sigma_i = a_i^(p_i - 2) g_i, n x dim row-major -- g_i bit for bit at p = 2, g_i / a_i at p = 1, exactly 0 where a_i = 0
 * for every p.
 * Batching: B >= 1 fields on the same geometry (the snapshots of a parabolic run) are reduced by ONE pair of launches: partials
 * on a grid (ceil(n / 256), B) of 256 threads, then one workgroup per field that combines its partials in ascending workgroup
 * order.  No atomics; the result of a field depends on n alone, not on B or on its place in the batch: a batch returns the bits
 * of B calls with B = 1.  The fields are B separate vectors (a device table of their B pointers is uploaded with every
 * call; no field is copied).  f: f_rows = 1 -- n values shared by all fields -- or f_rows = B -- B x n, row b
 * for field b.  The per-node arithmetic is compiled with fp contraction off (the products and the sums behind them are not
 * fused), in the kernels and in the host restatement.
 * MGB_E_ARG, before anything is launched: a null argument or field; B < 1 (device: B > 65535); S < 1; p not finite or < 1;
 * u or s outside [0, S); u == s; a vector whose length is not exactly what the shapes above say; f_rows neither 1 nor B;
 * vectors of another context; a sharded context (world > 1). */
#define MGB_ENERGY_COLS 5
/* two launches on the context stream; the B x MGB_ENERGY_COLS results are copied to the host and the call waits for them */
int mgb_geo_field_energy(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, int s, double p,
                         mgb_vec p_nodal_or_null, mgb_vec f_or_null, int f_rows, double* out_host /* B x MGB_ENERGY_COLS */);
/* host restatement (no context, no GPU): the same per-node routine on host arrays, field after field, summed serially in
 * ascending node order; flux_or_null: B x n x dim */
int mgb_geo_field_energy_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, int s, double p,
                              const double* p_nodal_or_null, const double* f_or_null, int f_rows,
                              double* out /* B x MGB_ENERGY_COLS */, double* flux_or_null);
/* one launch on the context stream, one thread per node; flux: a caller-owned device vector of n x dim values, not z; the call
 * does not wait on the host (there is no slack column here: the u == s rule does not apply) */
int mgb_geo_field_flux(mgb_locator loc, mgb_vec z, int S, int u, double p, mgb_vec p_nodal_or_null, mgb_vec flux);

/* ---- level sets of nodal fields: where a solution takes a given value (contours, areas, fronts in time) ---------------- *
 * Fields as for mgb_geo_field_energy: B >= 1 vectors of n x S row-major nodal values on the geometry of a locator, column u is
 * contoured; single-GPU contexts, fp64.  Levels: nl >= 1 finite doubles.  Row r = b nl + l of every output belongs to field b
 * and level c = levels[l].
 * 2-D (block 7: v1 v2 v3 m12 m23 m31 centroid).  Every element is cut into simplices ("items"); the field is taken as LINEAR
 * on an item, from its three lattice values.
 *   Fan.  ring = [v1, m12, v2, m23, v3, m31], C the centroid: macro triangle k = 0..5 has corners A = ring[k],
 *     B = ring[(k+1) % 6], C.
 *   Refinement.  refine = r in {0,1,2,3}, N = 2^r.  Lattice points P(a,b) = A + (a/N)(B-A) + (b/N)(C-A), a, b >= 0, a + b <= N.
 *     Small triangle j = 0..N^2-1: i the largest integer with i^2 <= j, q = j - i^2, b = N-1-i;
 *       q even, a = q/2:      corners (P(a,b), P(a+1,b), P(a,b+1));
 *       q odd,  a = (q-1)/2:  corners (P(a+1,b), P(a+1,b+1), P(a,b+1)).
 *   Item index.  item = (e 6 + k) N^2 + j;  6 4^r nel items per field and level (at most INT_MAX).
 *   Lattice values.  r = 0: the nodal values of A, B, C, loaded and never recomputed, at their coordinates, loaded as well.
 *     r > 0: the P2 + bubble function of the element at the lattice point's reference coordinates, which come from the
 *     reference coordinates of A, B, C by the formula of P; the sum runs over the seven nodes in ascending order.  Physical
 *     positions come from the coordinates of A, B, C in x by the formula of P.
 *   Classification.  A corner is ABOVE when v > c, by comparison only; k_above in {0,1,2,3}.
 *   Non-finite values.  An item with a non-finite lattice value contributes NaN to all five columns of its row and emits
 *     nothing; other rows stay bit for bit.  A NaN is never dropped.
 *   Crossing point.  On an edge with one corner above and one not, ALWAYS from the below corner to the above corner:
 *     t = (c - v_lo) / (v_hi - v_lo),  Q = P_lo + t (P_hi - P_lo).  Two elements that share an edge and hold the same nodal
 *     values there compute the same bits at r = 0: the contour is watertight.
 *   Segments.  k_above in {1,2}: one segment (Q0, Q1) between the crossings on the two edges at the lone corner, ordered so that
 *     the above side lies to its LEFT in physical coordinates (swapped when cross(Q1-Q0, P_above - Q0) < 0, P_above the lone
 *     corner for k_above = 1 and the corner after it for k_above = 2), whatever the sign of the element's determinant.  It is
 *     not emitted, and not counted, exactly when k_above = 2 and the lone corner's value == c (the zero-length case).  An item
 *     with k_above = 1 whose two other corners lie on the level emits that whole edge; an edge on the level may so be emitted
 *     by each of its two triangles.
 *   Per-item terms, A_it the item's area, a_s the area of the corner triangle (P_lone, Q0, Q1):
 *     k_above = 3:  above A_it,        excess A_it ((v0+v1+v2)/3 - c);
 *     k_above = 1:  above a_s,         excess a_s (v_lone - c)/3;
 *     k_above = 2:  above A_it - a_s,  excess A_it ((v0+v1+v2)/3 - c) - a_s (v_lone - c)/3;      length |Q1 - Q0|.
 * 1-D (block 2).  One item per element, refine must be 0; classification and the below-to-above rule as above.  A crossing is a
 *   point x with a direction, +1 when u rises through c in +x.  Above length (1-t) h or h; excess (1-t) h (v_hi - c) / 2 or
 *   h ((v_l+v_r)/2 - c).  A node on the level between an element that rises to it and one that is above beyond it is one
 *   crossing of the one element only; between two elements that are above on both sides it is a crossing of each.
 * 3-D: MGB_E_ARG (isosurfaces are not covered).
 * Per (field, level) one row of MGB_LEVELSET_COLS doubles
 *   [0] measure of {u > c}      [1] measure of {u = c}: length in 2-D, number of crossings in 1-D      [2] int_{u>c} (u - c)
 *   [3] max (v - c) over all lattice values      [4] max (c - v)      -- NaN-sticky maxima; a level outside the range of the
 *                                                                        field shows as a negative entry
 * and one long long, the number of emitted segments (1-D: crossings).
 * Launches: the measure on a grid (ceil(items / 256), nl, B) of 256 threads, one item per thread, one partial row and one
 * count per workgroup; then one workgroup per row, which folds the row's partials in the order of the other field reductions
 * (but from an identity whose two maxima are both -inf: either may be negative here) and turns the row's per-workgroup counts
 * into exclusive offsets.  The rows and the counts reach the host in ONE copy and the call waits.  With
 * segs non-null the total is allocated exactly and a third launch on the measure's grid recomputes every item and writes
 * [x0, y0, x1, y1] (1-D: [x, direction]) and the int32 item to slot row_offset + workgroup offset + rank in the workgroup.
 * No atomics: the output order is ascending item index within a row, rows in ascending order; a call repeated returns the same
 * bits, and a row does not depend on B, nl or its place in the batch.  The per-item arithmetic is compiled with fp contraction
 * off, in the kernels and in the host restatement.
 * MGB_E_ARG, before anything is launched: a null argument or field; B < 1, nl < 1, B or nl > 65535 (device); S < 1; u outside
 * [0, S); refine outside 0..3 (1-D: not 0); a non-finite level; vectors of the wrong length or of another context; a sharded
 * context; more than INT_MAX items per row; a 3-D geometry. */
#define MGB_LEVELSET_COLS 5
typedef struct mgb_levelset_s* mgb_levelset;   /* the emitted segments of one call, device resident; a handle made by
                                                * mgb_geo_isosurfaces (below) holds triangles instead: rows of 9 doubles;
                                                * one made by mgb_geo_sections the pieces of cuts: rows of 6 or 12 doubles */
int mgb_geo_level_sets(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, int nl,
                       const double* levels_host, int refine, double* out_host /* B nl x MGB_LEVELSET_COLS */,
                       long long* counts_host /* B nl */, mgb_levelset* segs_or_null);
/* copies to the host, each where non-null: row_offsets (B nl + 1, the total last), seg (total x 4, 1-D: total x 2; a handle of
 * mgb_geo_isosurfaces: total x 9, x0 y0 z0 x1 y1 z1 x2 y2 z2; a handle of mgb_geo_sections: total x 6 or total x 12), item
 * (total) */
int mgb_levelset_get(mgb_levelset segs, long long* row_offsets, double* seg, int32_t* item);
int mgb_levelset_destroy(mgb_levelset segs);
/* host restatement (no context, no GPU): the same per-item routine on host arrays, row after row, summed serially in ascending
 * item order; the three sums are compensated (Neumaier), because the equal item areas of a refined mesh round a plain running
 * sum the same way every time (1e-12 of the sum near 2e5 items).  row_offsets_or_null: B nl + 1; seg_or_null and item_or_null come together and hold `capacity` rows: MGB_E_ARG
 * when more segments are emitted (call once without them, size them by the counts, call again). */
int mgb_geo_level_sets_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, int nl,
                            const double* levels, int refine, double* out /* B nl x MGB_LEVELSET_COLS */,
                            long long* counts /* B nl */, long long* row_offsets_or_null, double* seg_or_null,
                            int32_t* item_or_null, long long capacity);

/* ---- isosurfaces of 3-D nodal fields ------------------------------------------------------------------------------------ *
 * What level_sets is in 1-D and 2-D, for 3-D geometries: per field and level the volume of {u > c}, the area of {u = c},
 * int_{u > c} (u - c), and the surface itself as oriented triangles.  mgb_geo_level_sets keeps refusing 3-D; this is its own
 * entry point.  (csrc/isosurface.hpp is the rule, run by the gfx950 kernels and by the host restatement.)
 *   Geometry.  block = (k+1)^3, k = 1..3: equispaced tensor nodes, x fastest, on the axis-aligned box spanned by the element's
 *     first node A and last node B (what mgb_geo_interpolate assumes).  Any other block: MGB_E_ARG.
 *   Lattice.  N = 2^refine, refine = 0..2, M = k N.  An element has M^3 cells of the lattice (a, b, c), 0 <= a, b, c <= M.
 *     refine = 0: the lattice points are the nodes, (a, b, c) is local node a + (k+1)(b + (k+1) c); values and coordinates are
 *     loaded and never recomputed.  refine > 0: the value is the tensor Lagrange function at (a, b, c) / M,
 *     sum_c sum_b (sum_a l_a(a/M) z_abc) (l_b(b/M) l_c(c/M)), innermost sum first, each in ascending order, the one-dimensional
 *     bases as in mgb_geo_interpolate; the position is A_d + (index_d / M)(B_d - A_d) per axis d.  Both depend on the lattice
 *     index alone: two items of one element that share a lattice point hold the same bits there.
 *   Items.  Every cell is cut into the six Kuhn tetrahedra around its diagonal O = (a, b, c) -> O + (1, 1, 1), one per permutation
 *     (p0, p1, p2) of the axes, t = 0..5 in lexicographic order (abc, acb, bac, bca, cab, cba): corners 0..3 are
 *     O, O + e_p0, O + e_p0 + e_p1, O + (1, 1, 1).  Every cell is cut the same way, so neighbouring cells and neighbouring
 *     elements of the structured cube agree on every face diagonal.  item = (e M^3 + cell) 6 + t, cell = a + M (b + M c);
 *     items per row = 6 M^3 nel <= INT_MAX.  The field is taken as linear on an item, from its four lattice values v0..v3.
 *   Classification, non-finite values and the crossing point are those of the level sets above: a corner is ABOVE when v > c;
 *     an item with a non-finite lattice value gives NaN in all five columns of its row and emits nothing; a crossing always
 *     runs from the below corner to the above corner, t = (c - v_lo) / (v_hi - v_lo), Q = P_lo + t (P_hi - P_lo).
 *   Pieces.  vol(p0, p1, p2, p3) = |(p1 - p0) . ((p2 - p0) x (p3 - p0))| / 6; V = vol of the item; a piece contributes its volume
 *     to [0] and its volume x the mean of its four corner excesses v - c (0 at a crossing) to [2].
 *     k_above = 4: the item, V and V ((v0 + v1 + v2 + v3) / 4 - c).      k_above = 0: nothing.
 *     k_above = 1 or 3: L = the lone corner (the one above, or the one not above), o1 < o2 < o3 the others, Q_i the crossing on
 *       the edge between L and o_i; the corner piece (P_L, Q1, Q2, Q3) has V_s = vol and X_s = V_s ((v_L - c) / 4).
 *       k_above = 1: V_s and X_s;      k_above = 3: V - V_s and V ((v0 + v1 + v2 + v3) / 4 - c) - X_s.      Triangle (Q1, Q2, Q3).
 *     k_above = 2: A0 < A1 the corners above, B0 < B1 the others, Q_ij the crossing from B_j to A_i.  The wedge
 *       (A0, Q00, Q01) - (A1, Q10, Q11) is the three tetrahedra w1 = (A0, Q00, Q01, A1), w2 = (Q00, Q01, A1, Q10),
 *       w3 = (Q01, A1, Q10, Q11): [0] = w1 + w2 + w3, [2] = w1 ((e0 + e1) / 4) + w2 (e1 / 4) + w3 (e1 / 4), e_i = v_Ai - c.
 *       The quadrilateral Q00 Q01 Q11 Q10 is split along its diagonal Q01 - Q10: triangles (Q00, Q01, Q10), then (Q01, Q11, Q10).
 *   Triangles.  A triangle two of whose vertices are the same point (all three coordinates compare equal: a corner exactly on
 *     the level) is neither emitted nor counted and adds no area.  Every other triangle (q0, q1, q2) adds |n| / 2,
 *     n = (q1 - q0) x (q2 - q0), to [1] and is emitted as (P0, P1, P2) = (q0, q1, q2) or (q0, q2, q1), so that
 *     (P1 - P0) x (P2 - P0) points to the BELOW side, the outward normal of {u > c}, in physical coordinates whatever the
 *     orientation of the tetrahedron or the box: q1 and q2 are exchanged when n . (R - q0) > 0 for R = P_L (k_above = 1) or
 *     R = P_A0 (k_above = 2), and when n . (P_L - q0) < 0 for k_above = 3.  A face of an item that lies on the level is emitted
 *     by every tetrahedron whose fourth corner is above, so possibly twice.  An item emits 0, 1 or 2 triangles; its two
 *     triangles are adjacent in the output, in the order above.  At refine = 0 on a mesh whose elements hold the same nodal
 *     values at shared nodes the surface is watertight: every edge not on the boundary occurs twice, in opposite directions.
 * Per (field, level) one row of MGB_LEVELSET_COLS doubles
 *   [0] volume of {u > c}      [1] area of {u = c}      [2] int_{u>c} (u - c)      [3] max (v - c)      [4] max (c - v)
 * over all lattice values, NaN-sticky, both maxima started from -inf, and one long long, the number of emitted triangles.
 * Launches, as for the level sets: the measure on a grid (ceil(items / 256), nl, B) of 256 threads, one item per thread, one
 * partial row and one count (0..2 per thread) per workgroup; the SAME finish launch; rows and counts in ONE copy.  With
 * tris non-null a third launch on the measure's grid recomputes every item, ranks it by the exclusive prefix sum of the counts
 * in its workgroup and writes its first triangle [x0 y0 z0 x1 y1 z1 x2 y2 z2] and the int32 item to slot row offset + workgroup
 * offset + rank, its second one to the next slot.  No atomics: ascending item order within a row, rows in ascending order; a
 * call repeated returns the same bits, a row does not depend on B, nl or its place in the batch.  The per-item arithmetic is
 * compiled with fp contraction off on both sides.  The triangles come back through mgb_levelset_get / mgb_levelset_destroy.
 * MGB_E_ARG, before anything is launched: a null argument or field; B < 1, nl < 1, B or nl > 65535 (device); S < 1; u outside
 * [0, S); refine outside 0..2; a non-finite level; vectors of the wrong length or of another context; a sharded context; more
 * than INT_MAX items per row; a 1-D or 2-D geometry (the message names level_sets). */
int mgb_geo_isosurfaces(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, int nl,
                        const double* levels_host, int refine, double* out_host /* B nl x MGB_LEVELSET_COLS */,
                        long long* counts_host /* B nl */, mgb_levelset* tris_or_null);
/* host restatement (no context, no GPU), shaped like mgb_geo_level_sets_host: serial, ascending item order, the three sums
 * compensated (Neumaier); tri_or_null (capacity x 9) and item_or_null come together, MGB_E_ARG when more triangles are emitted. */
int mgb_geo_isosurfaces_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, int nl,
                             const double* levels, int refine, double* out /* B nl x MGB_LEVELSET_COLS */,
                             long long* counts /* B nl */, long long* row_offsets_or_null, double* tri_or_null,
                             int32_t* item_or_null, long long capacity);

/* ---- plane sections of nodal fields: cuts, means, flow rates -------------------------------------------------------------- *
 * What a field looks like on the cut of the domain by a plane n . x = c (a line in 2-D), and how much flows through it: per
 * field and plane the measure of the cut, int u over it, the flow rate int sigma . nu with sigma = |grad u|^(p-2) grad u and
 * nu = n / |n|, the extrema of u over the quadrature points, and the cut itself as oriented pieces with the values of u at
 * their vertices.  B fields (n x S, row-major, column u) on one 2-D (block 7) or 3-D (block (k+1)^3, k = 1..3) geometry, nc
 * planes, one exponent p per call; single-GPU contexts, fp64.  Row r = b nc + l of every output belongs to field b and
 * plane l.  (csrc/section.hpp is the rule, run by the gfx950 kernels and by the host restatement.)
 *   Planes.  Row l of planes is (n_0 .. n_{dim-1}, c): dim + 1 doubles.  The side function is
 *     d(x) = (n_0 x_0 + n_1 x_1 [+ n_2 x_2]) - c, the products summed in that order, then c subtracted.  A corner is ABOVE
 *     when d > 0, by comparison only.  nu_a = n_a / sqrt(n_0^2 + n_1^2 [+ n_2^2]).  A crossing is the level sets': on an edge
 *     with one corner above and one not, ALWAYS from the below corner to the above corner, t = (0 - d_lo) / (d_hi - d_lo),
 *     Q = P_lo + t (P_hi - P_lo): the elements on both sides of an edge or a face compute the same bits.
 *   The elements are straight-sided triangles and axis-aligned boxes (what mgb_geo_interpolate assumes), so the plane cuts an
 *     element in an exact segment or polygon and u on the cut is a polynomial: no refinement exists here.
 *   2-D.  One item per element, item = e; corners: the local rows 0, 1, 2, coordinates loaded.  With 0 or 3 corners above the
 *     item contributes nothing.  Else L = the lone corner (the one above, or the one not above), o1 = (L + 1) % 3,
 *     o2 = (o1 + 1) % 3, Q0 and Q1 the crossings on the edges L - o1 and L - o2.  Where Q0 and Q1 are the same point (both
 *     coordinates compare equal) the item contributes nothing.  The segment is (Q0, Q1), exchanged when
 *     cross(Q1 - Q0, P_above - Q0) < 0 (P_above = P_L for one corner above, P_o1 for two): the above side lies to its LEFT.
 *     An element edge that lies in the line is so cut by the element on its above side alone.
 *     Quadrature: 4-point Gauss-Legendre, x_q = S0 + s_q (S1 - S0) per coordinate, weight w_q |S1 - S0|, in ascending q; u on
 *     a line through a P2 + bubble element is a cubic, so int u is exact up to rounding.
 *   3-D.  item = e 6 + t.  The box of element e is spanned by its eight corner nodes (local node K a + (K+1)(K b + (K+1) K c)
 *     for the corner (a, b, c) in {0,1}^3), loaded and never recomputed; it is cut into the six Kuhn tetrahedra of
 *     mgb_geo_isosurfaces (corners O, O + e_p0, O + e_p0 + e_p1, O + (1,1,1) for the t-th permutation of the axes).  Every box
 *     is cut the same way, so neighbours agree on every face diagonal.  Cases and orientation are those of the isosurfaces,
 *     applied to d with the level 0: one or three corners above give the triangle (Q1, Q2, Q3) of the crossings at the lone
 *     corner; two above give the quadrilateral Q00 Q01 Q11 Q10 split along Q01 - Q10 into (Q00, Q01, Q10) and (Q01, Q11, Q10).
 *     A triangle two of whose vertices are the same point is dropped: it contributes nothing.  Every other triangle is
 *     oriented so that (P1 - P0) x (P2 - P0) points to the BELOW side (towards -n).  A face of a tetrahedron that lies exactly
 *     in the plane is emitted by the tetrahedron whose fourth corner is above, so exactly once; values and gradients on such
 *     a face therefore come from the element on the ABOVE side (for a broken field the two sides differ).
 *     Quadrature on each emitted triangle (P0, P1, P2): the collapsed tensor Gauss-Legendre rule with n_K x n_K points,
 *     n_K = 3, 4, 6 for k = 1, 2, 3; point (i, j), i outer, both ascending: b0 = 1 - s_i, b1 = s_i (1 - s_j), b2 = s_i s_j,
 *     x = (b0 P0 + b1 P1) + b2 P2 per coordinate, weight ((w_i w_j) s_i) (2 area), area = |(P1 - P0) x (P2 - P0)| / 2.  The
 *     rule is exact for total degree 2 n_K - 2 >= 3 k, the degree of a Q_k function on a plane.
 *   Gauss nodes and weights on [0, 1] are the 17-digit constants of csrc/section.hpp.
 *   At a quadrature point x_q of an item of element e: v and g = value and physical gradient of column u of e's own polynomial
 *     (the bases and the operations of mgb_geo_flow_lines' val and grad; no locator is involved).  sigma = a^(p-2) g with
 *     a = |g|_2: g itself (bit for bit) at p = 2, g / a at p = 1, pow(a, p - 2) g otherwise, exactly 0 where a = 0.
 *     sigma . nu is summed over the axes in ascending order.
 * Per (field, plane) one row of MGB_LEVELSET_COLS doubles
 *   [0] sum w: the measure of the cut      [1] sum w v: int u      [2] sum w (sigma . nu): the flow rate in the direction of n
 *   [3] max v      [4] max (-v)      -- over the quadrature points; NaN-sticky, both started from -inf
 * and one long long, the number of emitted pieces.  The sums of a piece run in ascending point order from 0, those of an item
 * in piece order.  An item the plane does not cut reads no field value: a NaN in an uncut element is not seen.  A cut item
 * with a non-finite v or g at any quadrature point gives NaN in all five columns of its row and emits nothing; other rows stay
 * bit for bit.  A plane that cuts nothing gives 0, 0, 0, -inf, -inf and the count 0.
 * Pieces.  One row per emitted piece, in ascending item order within a row (the two triangles of an item adjacent), rows in
 * ascending order: 2-D 6 doubles x0 y0 x1 y1 | u0 u1, 3-D 12 doubles x0 y0 z0 x1 y1 z1 x2 y2 z2 | u0 u1 u2, u_m = the value
 * of the element's polynomial at vertex m (what a slice plot colours by), and the int32 item.  They come back through the
 * level sets' handle: mgb_levelset carries its row width, mgb_levelset_get copies total x 6 or total x 12 doubles for a handle
 * made here and keeps its behaviour for every other handle; mgb_levelset_destroy frees it.
 * Launches, as for the isosurfaces: the measure on a grid (ceil(items / 256), nc, B) of 256 threads, one item per thread, one
 * partial row and one count (0..2 per thread) per workgroup; the SAME finish launch; rows and counts in ONE copy.  With
 * pieces non-null a third launch on the measure's grid recomputes every item, ranks it by the exclusive prefix sum of the
 * counts in its workgroup and writes its pieces to slot row offset + workgroup offset + rank (and the next).  No atomics: a
 * call repeated returns the same bits, a row does not depend on B, nc or its place in the batch.  The per-item arithmetic is
 * compiled with fp contraction off on both sides; device and host restatement differ in the order of the three sums and, for
 * p other than 1 and 2, in pow.
 * MGB_E_ARG, before anything is launched: a null argument or field; a 1-D geometry (the message names interpolate); 3-D
 * elements other than (k+1)^3 nodes, k = 1..3; B < 1, nc < 1, B or nc > 65535 (device); B nc or the items per row beyond
 * INT_MAX; S < 1; u outside [0, S); a plane whose normal is zero or not finite or whose c is not finite; p not a finite real
 * >= 1 (one scalar per call: an exponent field p(x) is not supported); vectors of the wrong length or of another context; a
 * sharded context. */
int mgb_geo_sections(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, int nc,
                     const double* planes_host /* nc x (dim + 1) */, double p, double* out_host /* B nc x MGB_LEVELSET_COLS */,
                     long long* counts_host /* B nc */, mgb_levelset* pieces_or_null);
/* host restatement (no context, no GPU), shaped like mgb_geo_isosurfaces_host: serial, ascending item order, the three sums
 * compensated (Neumaier); piece_or_null (capacity x 6 or 12) and item_or_null come together, MGB_E_ARG when more pieces are
 * emitted (call once without them, size them by the counts, call again). */
int mgb_geo_sections_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, int nc,
                          const double* planes /* nc x (dim + 1) */, double p, double* out /* B nc x MGB_LEVELSET_COLS */,
                          long long* counts /* B nc */, long long* row_offsets_or_null, double* piece_or_null,
                          int32_t* item_or_null, long long capacity);

/* ---- flow lines of nodal fields: paths, lengths, travel times ------------------------------------------------------------ *
 * The curves that follow grad u through the broken polynomial field of column u of B fields (n x S, row-major) on one 2-D
 * (block 7) or 3-D (block (k+1)^3, k = 1..3) geometry, from m seeds, by the explicit midpoint rule in ARC LENGTH: the
 * exponent p of sigma = |grad u|^(p-2) grad u enters the travel time int ds / |sigma| only, never the geometry.
 * Notation.  val(e, q), grad(e, q): value and physical gradient of element e's polynomial at q by the bases of
 *   mgb_interpolate; q need not lie in e.  locate(e, q) = e if q is inside e by the containment rule above (tau = 1e-12), else
 *   the lowest element that contains q, -1 when none does or a coordinate is not finite.  sgn = direction, +1 (up the
 *   gradient) or -1.  |.| = the square root of the sum of squares taken in index order.
 * For seed x_0: e_0 = the lowest element that contains x_0; if there is none the status is OUTSIDE, the count 0, the end element
 * -1 and every double of the row NaN.  Otherwise the seed is recorded and for k = 0, 1, ...:
 *   1. v = val(e_k, x_k), g = grad(e_k, x_k); at k = 0 v is u_start.  Any of them non-finite: stop, NONFINITE.
 *   2. a = |g|.  Not a > gmin: stop, STALLED (a NaN cannot pass this comparison).
 *   3. k == max_steps: stop, MAXSTEPS.
 *   4. d = sgn g / a, q_m = x_k + (ds / 2) d, e_m = locate(e_k, q_m).  e_m < 0: exit along x_k -> q_m.
 *   5. g_m = grad(e_m, q_m).  Non-finite: stop, NONFINITE, at x_k.  a_m = |g_m|.  Not a_m > gmin: stop, STALLED, at x_k.
 *   6. d_m = sgn g_m / a_m, q_n = x_k + ds d_m, e_n = locate(e_m, q_n).  e_n < 0: exit along x_k -> q_n.
 *   7. length += ds; time += ds a_m^(1-p) (exactly 1 for p = 1 and 1 / a_m for p = 2, pow otherwise); x_{k+1} = q_n,
 *      e_{k+1} = e_n, and the point is recorded.
 * Exit along x_k -> q: lo = 0, hi = 1, the remembered element e_k; forty times th = (lo + hi) / 2, r = x_k + th (q - x_k),
 *   e = locate(e_k, r); e >= 0: lo = th and e is remembered, else hi = th.  The end point x_k + lo (q - x_k), in the remembered
 *   element, is recorded only if lo > 0; length += lo |q - x_k|, time += lo |q - x_k| a^(1-p) with the a of step 2; EXIT.
 * u_end = val at the end point in its element.  Every sum runs serially in step order.  A line that slides along an edge whose
 * two sides both point at it zigzags until MAXSTEPS: documented behaviour, not an error.
 * Per row r = b m + i (field b, seed i): MGB_FLOW_COLS doubles [length, time, u_start, u_end]; the end point (dim doubles);
 * int32 status, count (the points recorded, the seed included, at most max_steps + 1) and end element.
 * ds_or_null: the step; null takes a quarter of the smallest element extent (the extent of an element is the largest side of
 * its bounding box; computed from x once per geometry and kept with the locator); ds_used_or_null receives the step taken.
 * workgroup: 0 (the default, 64), 64, 128 or 256 threads; the result does not depend on it.
 * Launches: ONE, a grid (ceil(m / workgroup), B), one thread per (seed, field), no atomics, no LDS, no barrier; with
 * paths_or_null non-null every thread also records its points and their elements in its own row of max_steps + 2 slots (a slot
 * beyond that is never written), and after the counts have reached the host a second launch, one workgroup per row, gathers the
 * rows into CSR arrays behind the handle: offsets (B m + 1), points (total x dim), elements (total).  A call repeated returns
 * the same bits; a row does not depend on B, m or its place in the batch.  The rule is compiled with fp contraction off on both
 * sides: device and host restatement agree bit for bit except in `time` for p other than 1 and 2 (pow).
 * MGB_E_ARG, before anything is launched or written: a null argument or field; a 1-D geometry; ds not finite or <= 0;
 * max_steps < 1; gmin not finite or < 0; direction not +1 or -1; p not finite or < 1; S < 1; u outside [0, S); B < 1 or
 * B > 65535; m < 0; more than INT_MAX rows; vectors of the wrong length or of another context; a sharded context; another
 * workgroup size; with paths, B m (max_steps + 2) dim beyond 2^31 - 1.  m = 0 returns at once (an empty handle with paths). */
#define MGB_FLOW_COLS 4
#define MGB_FLOW_EXIT 0
#define MGB_FLOW_STALLED 1
#define MGB_FLOW_MAXSTEPS 2
#define MGB_FLOW_OUTSIDE 3
#define MGB_FLOW_NONFINITE 4
typedef struct mgb_flowpath_s* mgb_flowpath;   /* the recorded points of one call, device resident, in CSR form */
int mgb_geo_flow_lines(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, int m,
                       const double* seeds_host /* m x dim */, double p, int direction, const double* ds_or_null, int max_steps,
                       double gmin, int workgroup, double* rows_host /* B m x MGB_FLOW_COLS */, double* end_host /* B m x dim */,
                       int32_t* status_host /* B m */, int32_t* count_host /* B m */, int32_t* end_element_host /* B m */,
                       double* ds_used_or_null, mgb_flowpath* paths_or_null);
/* copies out what is asked for (null: skipped): offsets (B m + 1), pts (total x dim), elem (total) */
int mgb_flowpath_get(mgb_flowpath paths, long long* offsets, double* pts, int32_t* elem);
int mgb_flowpath_destroy(mgb_flowpath paths);
/* host restatement (no context, no GPU): the same routine, row after row.  offsets_or_null (B m + 1), pts_or_null
 * (capacity x dim) and elem_or_null (capacity) come together; MGB_E_ARG when more points are recorded than they hold. */
int mgb_geo_flow_lines_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, int m,
                            const double* seeds /* m x dim */, double p, int direction, const double* ds_or_null, int max_steps,
                            double gmin, double* rows /* B m x MGB_FLOW_COLS */, double* end /* B m x dim */, int32_t* status,
                            int32_t* count, int32_t* end_element, double* ds_used_or_null, long long* offsets_or_null,
                            double* pts_or_null, int32_t* elem_or_null, long long capacity);

/* ---- path lines through a field that changes in time: tracers, streaklines ------------------------------------------------ *
 * Where a particle released at a seed at snapshot time ts[release] is at ts[stop], what it passes through and when it leaves
 * the domain: m particles carried through B >= 2 snapshots z_0 .. z_{B-1} (n x S, column u) of one 2-D or 3-D geometry at
 * strictly increasing finite times ts[0 .. B-1], by the explicit midpoint rule in TIME.  (csrc/pathline.hpp is the rule, run
 * by the gfx950 kernel and by the host restatement.)  Notation (val, grad, locate, |.|, sgn) as for mgb_geo_flow_lines.
 * Field in time.  In slab j, [ts[j], ts[j+1]], at the fraction th, in element e at q: (v_a, g_a) = (val, grad) of z_j and
 *   (v_b, g_b) of z_{j+1}, both at (e, q); v = v_a + th (v_b - v_a), g[d] = g_a[d] + th (g_b[d] - g_a[d]), as written.  Two
 *   equal snapshots give bit for bit the stationary field; th = 0 gives snapshot j.  th is never formed from times: with
 *   n = substeps it is (double) i / n at the start of step i of a slab and (double) (2 i + 1) / (2 n) at its midpoint.
 * Velocity w(g), a = |g|: not a > gmin: w = 0, the particle rests (a NaN cannot pass this comparison).  Else
 *   p == 1: w[d] = speed (sgn g[d] / a);  p == 2: w[d] = speed (sgn g[d]);  p == 1.5: w[d] = speed (sgn g[d] / sqrt(a));
 *   otherwise w[d] = speed (sgn g[d] pow(a, p - 2)).  The first three use IEEE operations only.
 * For seed x_0 with release index rel: e_0 = the lowest element that contains x_0; if there is none the status is OUTSIDE, the
 * count 0, the end element -1, rested 0 and every double of the row NaN.  Otherwise the seed is recorded and for the slabs
 * j = rel .. stop - 1, with dt = (ts[j+1] - ts[j]) / n, for i = 0 .. n - 1, t_k = ts[j] + i dt:
 *   1. v, g at (x_k, e_k, th_i); at the very first step v is u_start.  Any of them non-finite: stop, NONFINITE.
 *   2. q_m = x_k + (0.5 dt) w(g), e_m = locate(e_k, q_m).  e_m < 0: exit along x_k -> q_m with the time span 0.5 dt.
 *   3. g_m at (q_m, e_m, th_mid).  Non-finite: stop, NONFINITE, at x_k.
 *   4. q_n = x_k + dt w(g_m), e_n = locate(e_m, q_n).  e_n < 0: exit along x_k -> q_n with the time span dt.
 *   5. s = dt |w(g_m)|; length += s; max_step = max(max_step, s); rested += 1 when w(g_m) was the zero of the rest rule;
 *      x_{k+1} = q_n, e_{k+1} = e_n, and the point is recorded, a resting one too: the path is a time series.
 * Exit along x_k -> q with span: the forty bisections of mgb_geo_flow_lines with locate from e_k; the end point
 *   x_k + lo (q - x_k), in the remembered element, is recorded only if lo > 0; length += lo |q - x_k|; time = t_k + lo span;
 *   u_end = the blended value there at th_i + lo span / (ts[j+1] - ts[j]); EXIT.
 * After the last step: DONE, time = ts[stop], u_end = val(z_stop) at the end point, from that snapshot alone.  On NONFINITE
 * time = t_k and u_end is the non-finite v, or NaN where only a gradient was non-finite.
 * Per seed: MGB_PATH_COLS doubles [length, time, u_start, u_end, max_step]; the end point (dim doubles); int32 status, count
 * (the points recorded, the seed included), end element and rested.  Every sum runs serially in step order; a row depends on its
 * seed, its release index and the fields alone, not on m, the workgroup size or its place in the batch.
 * workgroup: 0 (the default, 64), 64, 128 or 256 threads.  Launches: ONE, a grid ceil(m / workgroup), one thread per seed, no
 * atomics, no LDS, no barrier; with paths_or_null non-null every thread records into its own row of
 * (stop - min release) substeps + 2 slots, and the gather launch of mgb_geo_flow_lines fills the handle (mgb_flowpath_get /
 * mgb_flowpath_destroy; offsets m + 1).  The rule is compiled with fp contraction off on both sides: device and host
 * restatement agree bit for bit for p = 1, 1.5 and 2; for another p they differ by pow.
 * MGB_E_ARG, before anything is allocated, launched or written: a null argument or field; a 1-D geometry; B < 2 or B > 65535;
 * ts not finite or not strictly increasing; stop outside [1, B - 1]; a release index outside [0, stop); substeps < 1; p not
 * finite or < 1; speed not finite or <= 0; gmin not finite or < 0; direction not +1 or -1; S < 1; u outside [0, S); m < 0;
 * another workgroup size; vectors of the wrong length or of another context; a sharded context; with paths, m slots dim beyond
 * 2^31 - 1.  m = 0 returns at once (an empty handle with paths). */
#define MGB_PATH_COLS 5
#define MGB_PATH_DONE 0
#define MGB_PATH_EXIT 1
#define MGB_PATH_OUTSIDE 2
#define MGB_PATH_NONFINITE 3
int mgb_geo_path_lines(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, const double* ts_host /* B */, int S,
                       int u, int m, const double* seeds_host /* m x dim */, const int32_t* release_host /* m */, int stop,
                       int substeps, double p, int direction, double speed, double gmin, int workgroup,
                       double* rows_host /* m x MGB_PATH_COLS */, double* end_host /* m x dim */, int32_t* status_host /* m */,
                       int32_t* count_host /* m */, int32_t* end_element_host /* m */, int32_t* rested_host /* m */,
                       mgb_flowpath* paths_or_null);
/* host restatement (no context, no GPU): the same routine, row after row.  offsets_or_null (m + 1), pts_or_null
 * (capacity x dim) and elem_or_null (capacity) come together; MGB_E_ARG when more points are recorded than they hold. */
int mgb_geo_path_lines_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, const double* ts /* B */, int S,
                            int u, int m, const double* seeds /* m x dim */, const int32_t* release /* m */, int stop,
                            int substeps, double p, int direction, double speed, double gmin, double* rows /* m x MGB_PATH_COLS */,
                            double* end /* m x dim */, int32_t* status, int32_t* count, int32_t* end_element, int32_t* rested,
                            long long* offsets_or_null, double* pts_or_null, int32_t* elem_or_null, long long capacity);

/* ---- line integrals of nodal fields: chords, gates, projections (2-D and 3-D geometries; single-GPU contexts, fp64) -------- *
 * Segment i is x(t) = a_i + t (b_i - a_i), t in [0, 1], l = |b - a|, tdir = (b - a) / l and in 2-D the left normal
 * nu = (-tdir_y, tdir_x).  The field is the broken polynomial field of column u of z (n x S row-major), as for
 * mgb_geo_interpolate.  What one segment collects (csrc/ray.hpp: integrate, run by the kernels and by the host restatement):
 *   1. Clip.  For element e the reference coordinates of a and of b (the inverse maps of mgb_geo_interpolate) make every
 *      constraint function -- lambda_0, lambda_1, lambda_2 in 2-D; xi_d and 1 - xi_d in 3-D -- affine along the segment:
 *      g_j(t) = alpha_j + t beta_j, alpha_j = g_j(a), beta_j = g_j(b) - g_j(a).  e's interval is {t in [0, 1] : g_j(t) >= -tau
 *      for all j}, tau = 1e-12: beta_j > 0 raises t0 to -(alpha_j + tau) / beta_j, beta_j < 0 lowers t1 to the same quotient,
 *      beta_j == 0 with alpha_j + tau < 0 empties it.  Comparisons only, never fmin / fmax.  A piece needs t1 > t0.
 *   2. Ownership.  With m = x((t0 + t1) / 2) the piece counts iff the element of m by the containment rule of
 *      mgb_geo_interpolate -- the LOWEST element containing m -- is e.  A segment in a face, an edge or through a vertex is
 *      integrated once, in the lowest of the elements that share it; elements that only touch the segment drop out.
 *      Neighbouring pieces overlap by at most tau / |beta_j| in t at each end; this is not corrected.
 *   3. Walk.  The segment is clipped to the bounding box of the bin grid grown by 1e-9 x its diagonal (the slack).  The major
 *      axis M maximises |b_d - a_d| x (cells per unit length of axis d).  For each cell layer along M between the layers of
 *      the entry and the exit point (each moved outwards by the slack), in the direction of travel: the t-range of the layer
 *      grown by the slack, the segment's coordinates on the other axes at both ends of that range -/+ the slack, converted to
 *      cell coordinates (monotone), give a rectangle of cells, visited in ascending order.  In cell c the ascending
 *      candidate list is walked; element e is processed there iff it has a piece and the cell of its midpoint is c.  Every
 *      cell and every element is visited once.  a == b, a non-finite end point or a segment beside the box give no pieces.
 *   4. Quadrature.  Gauss-Legendre on [t0, t1] with 4 points in 2-D and 3, 4, 6 points in 3-D for k = 1, 2, 3 (exact for
 *      int u, of degree 3 k <= 2 N - 1 along a line).  At a point: value and gradient of e's own polynomial, sigma =
 *      |grad u|^(p - 2) grad u (grad u itself at p = 2, grad u / |grad u| at p = 1, exactly 0 where grad u = 0).  Maximum and
 *      minimum over the Gauss points and both piece ends.
 *   5. Per row r = b m + i (field b, segment i) MGB_RAY_COLS doubles and an int32 count of owned pieces:
 *        [0] length    sum (t1 - t0) l            [4] max   as in 4.
 *        [1] integral  int u ds                   [5] min   as in 4.
 *        [2] along     int sigma . tdir ds        [6] enter the smallest t0
 *        [3] across    int sigma . nu ds; 0 (3-D) [7] leave the largest t1
 *      Plain (uncompensated) sums in walk order.  No pieces: 0, 0, 0, 0, -inf, +inf, NaN, NaN and count 0.  A non-finite value
 *      or gradient at any point of an owned piece makes [1] .. [5] of that row NaN; [0], [6], [7] and count are unaffected;
 *      an element without an owned piece is never read.  A row depends on its segment and field alone: not on m, B, the
 *      workgroup size or its place in the batch.
 *   6. Pieces (pieces_or_null non-null): per row, in walk order, the element (int32) and t0, t1, int u of every owned piece,
 *      in CSR form.  The counts come from the measure launch, the host forms the offsets, a second launch walks again and
 *      writes at its offsets.  They come back through mgb_levelset_get / mgb_levelset_destroy, unchanged: row_offsets B m + 1,
 *      seg total x 3, item = the element.
 * workgroup: 0 (the default, 64), 64, 128 or 256 lanes; one lane per (segment, field) on a grid (ceil(m / workgroup), B).
 * The rule is compiled with fp contraction off on both sides: device and host restatement agree bit for bit for p = 1 and 2;
 * for another p, along and across differ by pow.
 * MGB_E_ARG, before anything is allocated, launched or written: a null argument or field; a 1-D geometry; B < 1 or B > 65535;
 * p not finite or < 1; S < 1; u outside [0, S); m < 0; B m beyond 2^31 - 1; another workgroup size; vectors of the wrong
 * length or of another context; a sharded context.  m = 0 returns at once (an empty handle with pieces). */
#define MGB_RAY_COLS 8
int mgb_geo_line_integrals(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, int m,
                           const double* a_host /* m x dim */, const double* b_host /* m x dim */, double p, int workgroup,
                           double* rows_host /* B m x MGB_RAY_COLS */, int32_t* count_host /* B m */,
                           mgb_levelset* pieces_or_null);
/* host restatement (no context, no GPU): the same routine, row after row.  offsets_or_null (B m + 1), piece_or_null
 * (capacity x 3) and elem_or_null (capacity) come together; MGB_E_ARG when there are more pieces than they hold. */
int mgb_geo_line_integrals_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, int m,
                                const double* a /* m x dim */, const double* b /* m x dim */, double p,
                                double* rows /* B m x MGB_RAY_COLS */, int32_t* count /* B m */, long long* offsets_or_null,
                                double* piece_or_null, int32_t* elem_or_null, long long capacity);

/* ---- time statistics of a run of snapshots ------------------------------------------------------------------------------ *
 * The one reduction along the TIME axis, per node: for B >= 2 snapshots z[0..B-1] (n x S row-major, column u) at the strictly
 * increasing times ts[0..B-1] of one geometry, what each node saw -- dose, peak, trough, variation -- and, per level c, when
 * the value first rose above c, when it last fell back, for how long and by how much it was above.  (csrc/timestat.hpp is the
 * rule, run by the gfx950 kernel and by the host restatement.)
 * Notation: v_m = z[m][i S + u]; h_m = ts[m+1] - ts[m], ONE subtraction, done once per call on the host and handed to both
 * sides.  A value is ABOVE when v > c (the rule of mgb_geo_level_sets: a value on the level is not above).  Every sum is a
 * plain running sum in ascending m.
 * Node table, n x MGB_TIMESTAT_NODE_COLS:
 *   [0] integral   acc += (0.5 h_m) (v_m + v_{m+1})                  [5] variation  sum |v_{m+1} - v_m|
 *   [1] max_m v_m  [2] ts of the FIRST m that attains it             [6] rate       max_m |v_{m+1} - v_m| / h_m
 *   [3] min_m v_m  [4] its time, likewise                            [7] change     v_{B-1} - v_0
 * Level table, nl x n x MGB_TIMESTAT_LEVEL_COLS (level-major, so that a wave's stores are contiguous):
 *   [0] arrival  [1] left  [2] exposure  [3] excess  [4] entries (a whole number, stored as a double)
 *   start: v_0 > c gives entries = 1, arrival = ts[0].
 *   interval with both ends above:   exposure += h_m;   excess += h_m ((v_m + v_{m+1}) 0.5 - c).
 *   interval with exactly one end above, always parametrised from the not-above end lo to the above end hi:
 *     t = (c - v_lo) / (v_hi - v_lo),  f = 1.0 - t,  e = f h_m;   exposure += e;   excess += e ((v_hi - c) 0.5);
 *     rising (hi = m+1):  where there is no entry yet arrival = ts[m] + t h_m;  entries += 1.
 *     falling:            left = ts[m+1] - t h_m  (the last one stays).
 *   interval with neither end above: nothing.   arrival / left without an event hold `never` (any double, NaN included).
 * A node with a non-finite v_m has NaN in all 8 node columns and all 5 columns of every level (`never` does not apply), and its
 * terms reach the totals as NaN: a NaN is never dropped.
 * Totals, (1 + nl) rows of 5 doubles (three sums, two NaN-sticky maxima), w the nodal weights of the geometry:
 *   row 0      [0] sum w integral       [1] sum w variation   [2] sum w change   [3] max_i max_i        [4] max_i (-min_i)
 *   row 1 + l  [0] sum w [entries > 0]  [1] sum w exposure    [2] sum w excess   [3] max arrival over the nodes with
 *                                                                                    entries > 0        [4] max_i exposure_i
 *   Both maxima of every row start from -inf (the identity of the level sets): row 1 + l holds -inf in [3] where no node was reached.
 * Launches: the statistics on a grid (ceil(n / 256), 1 + ceil(nl / chunk)) of 256 threads, one node per thread, which walks
 * m = 0..B-1 once with several loads in flight and its state in registers -- y = 0 the node columns and row 0, y >= 1 a chunk
 * of levels -- and writes one partial row per workgroup and result row; then one workgroup per row, which folds the partials in
 * the order of the other field reductions.  Two launches, one wait and one copy of the totals whatever B and nl are; the
 * snapshot pointers, h, ts and the levels go up in one copy.  The tables stay on the device.  No atomics.
 *   Cost: every slab of workgroups reads all B snapshots, so a call reads the run 1 + ceil(nl / chunk) times (chunk = 4:
 *   3 passes for 8 levels, 1025 for the 4096 allowed) and writes 40 n bytes per level.  The launches stay two, the traffic
 *   grows with nl: pass the levels that are wanted, not a fine ladder of them.
 *   A repeated call returns the same bits.  Row 1 + l and the level table of level l do not depend on nl, on the other levels or
 *   on the chunk.  The bits depend on the B snapshots and times handed over alone: a window of a longer run is a call of its own.
 *   The rule is compiled with fp contraction off on both sides: device and host restatement agree bit for bit in both tables
 *   and in the maxima; the three sums differ by their order (host: serial, compensated).
 * MGB_E_ARG, before anything is launched or written: a null argument or field (levels and level may be null where nl = 0);
 * B < 2; ts not finite or not strictly increasing; nl < 0 or nl > 4096; a non-finite level; S < 1; u outside [0, S); a vector
 * of the wrong length or of another context; an output that is also an input or the other output; a sharded context. */
#define MGB_TIMESTAT_NODE_COLS 8
#define MGB_TIMESTAT_LEVEL_COLS 5
int mgb_geo_time_stats(mgb_locator loc, int B, const mgb_vec* z /* B vectors of n x S */, const double* ts_host /* B */, int S,
                       int u, int nl, const double* levels_host_or_null, double never,
                       mgb_vec node /* n x MGB_TIMESTAT_NODE_COLS */, mgb_vec level_or_null /* nl x n x MGB_TIMESTAT_LEVEL_COLS */,
                       double* out_host /* (1 + nl) x 5 */);
/* host restatement (no context, no GPU): the same per-node routines, serially in ascending node order; the three sums are
 * compensated (Neumaier) as in the other _host functions. */
int mgb_geo_time_stats_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, const double* ts /* B */, int S,
                            int u, int nl, const double* levels_or_null, double never,
                            double* node /* n x MGB_TIMESTAT_NODE_COLS */, double* level_or_null /* nl x n x MGB_TIMESTAT_LEVEL_COLS */,
                            double* out /* (1 + nl) x 5 */);

/* ---- boundary facets of a geometry and boundary integrals of p-Laplace solutions --------------------------------------- *
 * The elements are broken and their quadrature is nodal: every node of a boundary facet is a row of x and z already, so the
 * boundary rule of a geometry is a list of nf facets of q nodes each: q global rows, q weights omega, the outward unit normal n,
 * the measure and the centre of the facet, and its own element.  Built once per geometry, on the host.
 * Finding the boundary: a facet of an element is a boundary facet when the sorted tuple of the continuous dofs of its CORNER
 * nodes occurs in exactly one element.  The dofs are the columns of subspaces "full" at the finest level, which must have
 * exactly one entry of value 1 per row.  Facets come in ascending (element, local facet) order:
 *   1-D  local facets = local nodes 0, 1              q = 1          omega = 1                  n = sign(x - element centre)
 *   2-D  edge i = local rows i, 3 + i, (i + 1) % 3    q = 3          |e| (1/6, 4/6, 1/6)        n perpendicular to v_a -> v_b,
 *        (v_i, m_{i,i+1}, v_{i+1}), i = 0..2                         (Simpson)                  n . (midpoint - centroid) > 0
 *   3-D  x-, x+, y-, y+, z-, z+: the (k+1)^2 nodes    q = (k+1)^2    area x the tensor of the   n = +- the axis, by
 *        of the side in ascending local index                        closed Newton-Cotes        sign(face coordinate - element
 *                                                                    weights of degree k        centre)
 * The measure of a facet is 1, |e|, the face area; its centre the node, the edge midpoint, the face centre.
 * MGB_E_ARG: a null argument; a geometry without a full subspace, or whose finest full subspace has not one row per node with
 * exactly one entry 1; a corner tuple that occurs more than twice (non-manifold mesh); elements the locator refuses.
 *
 * Boundary integrals.  At facet node j of facet f, row i = nodes[f q + j], of a field z (n x S row-major, as for
 * mgb_geo_field_energy; single-GPU contexts, fp64):
 *   sigma_i = |grad u|^(p_i - 2) grad u at x_i in i's OWN element (the arithmetic of mgb_geo_field_flux),
 *   sn = sigma_i . n_f,   t = sigma_i - sn n_f   (the tangential part).
 * Per field one row of MGB_BOUNDARY_COLS doubles
 *   [0] sum omega sn      the flow through the selected facets,   int sigma . n ds
 *   [1] sum omega u_i     int u ds  (divide by [2] for the mean of the trace)
 *   [2] sum omega         the measure of the selected facets
 *   [3] max |sn|          the largest normal flux
 *   [4] max |t|_2         the largest tangential flux
 * mask (nf bytes on the HOST, copied on the context stream; null: every facet): a facet whose byte is 0 is left out of every
 * sum and maximum.  An empty selection gives five zeros.  facet_flux (host, B x nf; null: not wanted): sum_j omega sn of every
 * facet, its q terms added in ascending j; 0 for a facet left out.
 * A SELECTED node whose u_i or sigma_i is not finite, or whose exponent is not a finite real >= 1, makes all five results of
 * that field NaN (and the value of its facet); it is never dropped.  Nodes off the selected facets are not looked at.  Other
 * fields of the batch are unaffected, bit for bit.
 * Batching: B >= 1 fields are reduced by ONE pair of launches: partials on a grid (ceil(nf / (256 / q)), B) of 256 threads, one
 * thread per (facet, facet node), whole facets per workgroup; then one workgroup per field that combines its partials in
 * ascending workgroup order.  No atomics; a field's result depends on the facet list and the mask alone, not on B or on its place
 * in the batch: a batch returns the bits of B calls with B = 1, and a call repeated returns the same bits.  The per-node
 * arithmetic is compiled with fp contraction off, in the kernels and in the host restatement.
 * MGB_E_ARG, before anything is launched: a null argument or field; B < 1 (device: B > 65535); S < 1; p not finite or < 1;
 * u outside [0, S); a vector whose length is not n x S (p_nodal: n); vectors of another context; a sharded context. */
#define MGB_BOUNDARY_COLS 5
typedef struct mgb_boundary_s* mgb_boundary;   /* boundary facets of a geometry, device resident */
/* the locator must be the one of geometry g and must outlive the boundary */
int mgb_boundary_create(mgb_locator loc, mgb_geo g, mgb_boundary* out);
int mgb_boundary_destroy(mgb_boundary b);
int mgb_boundary_dims(mgb_boundary b, int* nf, int* q, int* dim);
/* host arrays, each nullable: element nf, nodes nf x q, weights nf x q, normal nf x dim, measure nf, centre nf x dim */
int mgb_boundary_get(mgb_boundary b, int32_t* element, int32_t* nodes, double* weights, double* normal, double* measure,
                     double* centre);
/* two launches on the context stream; the results are copied to the host and the call waits for them */
int mgb_boundary_flux(mgb_boundary b, int B, const mgb_vec* z /* B vectors of n x S */, int S, int u, double p,
                      mgb_vec p_nodal_or_null, const unsigned char* mask_host_or_null, double* facet_flux_host_or_null /* B x nf */,
                      double* out_host /* B x MGB_BOUNDARY_COLS */);
/* host only (no context, no GPU): the facet list of a geometry ... */
int mgb_geo_boundary_dims(mgb_geo g, int* nf, int* q, int* dim);
int mgb_geo_boundary_get(mgb_geo g, int32_t* element, int32_t* nodes, double* weights, double* normal, double* measure,
                         double* centre);
/* ... and the host restatement: the same per-node routine on host arrays, field after field, summed serially in ascending
 * (facet, facet node) order */
int mgb_geo_boundary_flux_host(mgb_geo g, int B, const double* const* z /* B arrays of n x S */, int S, int u, double p,
                               const double* p_nodal_or_null, const unsigned char* mask_or_null,
                               double* facet_flux_or_null /* B x nf */, double* out /* B x MGB_BOUNDARY_COLS */);

/* ---- residual error indicators ------------------------------------------------------------------- *
 * Single-GPU contexts, fp64.  Where the error of a solve sits: per element three numbers, and five totals.
 * Interior facets.  A facet whose sorted corner dofs occur in exactly two elements.  The first side is the one with the smaller
 * (element, local facet); the facets come in ascending (element, local facet) order of their first side.  Per facet: the two
 * elements; the q rows of the first side in the order of the boundary facets' nodes, then the q rows of the second side permuted
 * so that node j of both sides has the same continuous dof; weights, measure, centre and the unit normal pointing out of the
 * first side, by the formulas of the boundary facets.  elem_facet (nel x nlf, nlf = 2 / 3 / 6): the interior facet of (element,
 * local facet), or -1 - f for boundary facet f; every local facet is one or the other.  MGB_E_ARG: a mesh that
 * mgb_geo_boundary_get refuses, or two sides that cannot be matched node by node.
 * Indicator.  Sigma (n x dim) is the nodal flux of mgb_geo_field_flux (the same launch, the same bits).  lambda_i is `scale`
 * when own_scale != 0, else the exponent p_i (the problem  min int f u + s, s >= |grad u|^p  has the strong form
 * f - p div sigma = 0  and the natural condition  p sigma . n + h = 0;  scale = 1 is the convention of mgb_geo_field_energy).
 *   node i:            rho_i = f_i - lambda_i sum_k d_k (I Sigma_k)(x_i), the divergence of the element interpolant of Sigma in
 *                      i's own element, k ascending (f null: 0)
 *   interior facet F:  J_Fj = lambda_a ((Sigma_a - Sigma_b) . n_F) with rows a, b of the two sides;  J_F = sum_j omega_Fj |J_Fj|^r
 *   Neumann facet F:   N_F = sum_j omega_Fj |lambda_i (Sigma_i . n_F) + h_Fj|^r; h is nf x q as mgb_boundary_load takes it, null:
 *                      the boundary contributes nothing; a facet the mask leaves out gives 0 and its h is not read
 *   element e:         h_e = (sum_{i in e} w_i)^(1/dim);  vol = h_e^r sum_i w_i |rho_i|^r;  jump = (h_e / 2) sum J_F over its
 *                      interior facets;  neu = h_e sum N_F over its boundary facets;  eta_e^r = (vol + jump) + neu
 * All inner sums run in ascending order (local node, facet node, local facet).  eta holds nel x 3: vol, jump, neu.  The
 * MGB_ESTIMATE_COLS totals: sum vol | sum jump | sum neu | max_e eta_e^r | max |J_Fj|.  A non-finite u, sigma, f or h, or an
 * exponent that is not a finite real >= 1, makes every number it feeds NaN -- the element's three numbers, those of its facet
 * neighbours where a jump is hit, and the totals; the maxima are NaN-sticky.  fp contraction is off in the kernels and in the
 * host restatement; powers go through the rule of mgb_field_norms (no pow for r = 2 and r = 1).
 * mgb_estimate: the flux launch, then facet_terms_kernel (one thread per facet node, 256 / q whole facets per workgroup; left
 * out when there is no facet), element_indicator_kernel (one thread per node, 256 / block whole elements per workgroup) and
 * estimate_finish (one workgroup, partials in ascending workgroup order) on the context stream; h and the mask are copied on
 * that stream; the call waits and copies the totals to the host.  No atomics; a repeated call repeats bit for bit.
 * MGB_E_ARG, before anything is launched or written: a null argument; S < 1; u outside [0, S); p or r not finite or < 1; a
 * non-finite scale; a vector of the wrong length or of another context; eta == z; a sharded context. */
#define MGB_ESTIMATE_COLS 5
int mgb_geo_interior_dims(mgb_geo g, int* nif, int* q, int* dim, int* nel, int* nlf);
/* host arrays, each nullable: elements nif x 2, nodes nif x 2 x q, weights nif x q, normal nif x dim, measure nif, centre
 * nif x dim, elem_facet nel x nlf */
int mgb_geo_interior_get(mgb_geo g, int32_t* elements, int32_t* nodes, double* weights, double* normal, double* measure,
                         double* centre, int32_t* elem_facet);
/* the tables live in the mgb_boundary of the geometry */
int mgb_estimate(mgb_boundary b, mgb_vec z /* n x S */, int S, int u, double p, mgb_vec p_nodal_or_null, mgb_vec f_or_null, double r,
                 int own_scale, double scale, const double* h_host_or_null /* nf x q */, const unsigned char* mask_host_or_null,
                 mgb_vec eta /* nel x 3 */, double* out_host /* MGB_ESTIMATE_COLS */);
/* host only: the same per-node, per-facet and per-element routines, serially; J (nif), N (nf) and sigma (n x dim) nullable */
int mgb_geo_estimate_host(mgb_geo g, const double* z /* n x S */, int S, int u, double p, const double* p_nodal_or_null,
                          const double* f_or_null, double r, int own_scale, double scale, const double* h_or_null,
                          const unsigned char* mask_or_null, double* eta /* nel x 3 */, double* J_or_null, double* N_or_null,
                          double* sigma_or_null, double* out /* MGB_ESTIMATE_COLS */);

/* ---- error indicators of the steps of a parabolic run --------------------------------------------- *
 * Single-GPU contexts, fp64.  A run has snapshots Z_0 .. Z_B (n x S row-major, B + 1 = len(ts)) at strictly increasing finite
 * times, h_k = ts[k] - ts[k-1].  Step k = 1..B solved  min int (1/2h_k)(s1 - 2 u u_(k-1)) + (1/p) s2 + f_k u,  whose strong form is
 * (u_k - u_(k-1)) / h_k + f_k - div sigma_k = 0  with the natural condition  sigma_k . n + h_k^N = 0  on the free facets: the
 * residual of mgb_estimate with own_scale (lambda = scale, default 1; lambda_i = p_i is not offered) plus one term.  Everything
 * not named here is mgb_estimate's, unchanged: the facet tables, h_e, the power rule, the ascending sum orders, fp contraction
 * off, the NaN rules.
 *   flux          Sigma^m, m = 0..B, the nodal flux of snapshot m, bit for bit what mgb_geo_field_flux gives for it; one launch
 *                 for all B + 1 fields; sigma holds (B + 1) x n x dim
 *   node i        d_i = (u^k_i - u^(k-1)_i) / h_k, a subtraction, then a division;
 *                 rho_i = (f_k,i + d_i) - lambda div(I Sigma^k)(x_i)  (f null: 0);  rate term  w_i |d_i|^r
 *   element e     vol_e, jump_e, neu_e from Sigma^k exactly as in mgb_estimate, the Neumann data those of the step's new time;
 *                 tim_e = sum_{i in e} w_i |Sigma^k_i - Sigma^(k-1)_i|_2^r, the 2-norm a square root of the squares summed in
 *                 ascending component order, local i ascending (at p = 2 this is |grad (u_k - u_(k-1))|, the classical time
 *                 indicator of implicit Euler)
 *   parts         B x nel x 4: vol, jump, neu, tim
 *   out           B x 2 x MGB_ESTIMATE_COLS:  row 0 is mgb_estimate's row: sum vol | sum jump | sum neu | max eta_e^r | max |J_Fj|;
 *                 row 1 is  sum tim | sum_i w_i |d_i|^r | 0 | max_e tim_e | max_i |d_i|  (the rate sum per element in ascending
 *                 local order, then over the elements)
 * f: f_rows = 1 -- n values for every step -- or f_rows = B -- row k - 1 for step k.  h (host): h_rows x nf x q, h_rows 1 or B,
 * null: the boundary contributes nothing; mask (host, nf bytes) as for mgb_estimate.
 * A non-finite u^k_i, u^(k-1)_i, Sigma^k, Sigma^(k-1), f or h makes what it feeds NaN, and the maxima are NaN-sticky: a NaN in
 * snapshot m reaches steps m and m + 1 and no other.
 * Bitwise: a repeated call repeats; what a step's numbers are made of depends on its two snapshots, its f, h and h_k alone, so B
 * steps in one call give the bits of B calls with B = 1; sigma[m] is mgb_geo_field_flux of snapshot m; where the two snapshots of
 * a step hold the same values, row 0 and vol, jump, neu are the bits of mgb_estimate on that snapshot with own_scale = 1 and the
 * same scale, f, h and mask, and tim, the rate and both maxima of row 1 are exactly 0.
 * mgb_estimate_steps: four launches whatever B is -- the flux on grid (ceil(n / 256), B + 1), then the kernels of mgb_estimate
 * with the step in blockIdx.y: facet_terms_kernel on (workgroups, B) (left out when there is no facet), element_indicator_kernel
 * on (workgroups, B), estimate_finish on 2 B workgroups, one per row of totals.  No atomics.  The table of the snapshots, the
 * step sizes, h and the mask are copied up per call; the per-facet values and the partials live with the boundary handle and
 * grow on demand.  One wait, one copy of 10 B doubles to the host.
 * MGB_E_ARG, before anything is launched or written: a null argument or field; B < 1 or B + 1 > 65535; ts not finite or not
 * strictly increasing; S < 1; u outside [0, S); p or r not finite or < 1; a non-finite scale; f_rows or h_rows neither 1 nor B; a
 * vector of the wrong length or of another context; an output (sigma, parts) that is also an input or the other output; a sharded
 * context. */
int mgb_estimate_steps(mgb_boundary b, int B, const mgb_vec* z /* B + 1 vectors of n x S */, const double* ts_host /* B + 1 */,
                       int S, int u, double p, mgb_vec p_nodal_or_null, mgb_vec f_or_null, int f_rows, double r, double scale,
                       const double* h_host_or_null /* h_rows x nf x q */, int h_rows, const unsigned char* mask_host_or_null,
                       mgb_vec sigma /* (B + 1) x n x dim */, mgb_vec parts /* B x nel x 4 */,
                       double* out_host /* B x 2 x MGB_ESTIMATE_COLS */);
/* host only: the same routines, serially, step after step; sigma ((B + 1) x n x dim), J (B x nif) and N (B x nf) nullable */
int mgb_geo_estimate_steps_host(mgb_geo g, int B, const double* const* z /* B + 1 arrays of n x S */, const double* ts /* B + 1 */,
                                int S, int u, double p, const double* p_nodal_or_null, const double* f_or_null, int f_rows, double r,
                                double scale, const double* h_or_null, int h_rows, const unsigned char* mask_or_null,
                                double* sigma_or_null, double* parts /* B x nel x 4 */, double* J_or_null, double* N_or_null,
                                double* out /* B x 2 x MGB_ESTIMATE_COLS */);

/* ---- mixed boundary conditions: Dirichlet on part of the boundary, Neumann data on the rest ------- *
 * Single-GPU contexts, fp64.
 * Dirichlet subspace.  mgb_geo_dirichlet_on adds "sub:<name>:<l>" for every level l (read back with mgb_geo_matrix_info / _get;
 * name it in the state variables of mgb_amg_create*).  The pinned rows are the rows of the selected boundary facets (the facet
 * list of mgb_geo_boundary_get; facet_mask nf bytes, null = every facet); the set is closed, facet end points belong to it.  Per
 * level, a column of "sub:full:<l>" is dropped when it has a non-zero value in a pinned row of the finest mesh (stored zeros do
 * not count); kept columns keep their order and their bits, stored zeros included.  Every facet selected gives the matrices of
 * "dirichlet", none those of "full".  MGB_E_ARG, nothing added: a null argument; the name is full, dirichlet or fixed, is
 * already present, is empty or holds ':'; the geometry has no full subspace; a level of it is missing; a mesh that
 * mgb_geo_boundary_get refuses.
 * Neumann load.  The objective is sum_i w_i c_i . (Dz)_i, so  int_Gamma h u ds  is the addition of
 *     l_i = (sum over the facet nodes (f, j) whose row is i of  omega_fj h_fj) / w_i
 * to the (u, id) column of c at the boundary rows.  The facet list carries a row-sorted incidence table: the nb distinct rows of
 * the facet nodes in ascending order, nb + 1 row starts, and the facet-node indices f q + j in ascending order within a row.
 * For boundary row r the kernel and the host restatement add omega h over its incidences in table order, skipping the facets
 * the mask leaves out (their h is not read: a NaN there is not seen), then divide once by w_r; a row with no selected incidence
 * gives exactly 0.  fp contraction is off in both.  h holds B fields (time levels) of nf x q doubles in HOST memory, copied on
 * the context stream like the mask; the output is compact, B x nb.  One launch on grid (ceil(nb / 256), B), one thread per
 * distinct row; no atomics, no LDS; a batch returns the bits of its singles and a repeated call repeats.
 * mgb_boundary_load_add: y[rows[j] stride + offset] += alpha load[k nb + j], one thread per j (the rows are distinct);
 * (stride, offset) = (1, 0) adds to a forcing vector of n values.  mgb_amg_add_cost_rows does the same into column col of the
 * AMG's cost, (stride, offset) = (K, col), on the context stream behind mgb_amg_set_c: only values of the cost buffer change.
 * None of the three waits for the device.  MGB_E_ARG, before anything is launched: a null argument; B outside [1, 65535]; a
 * vector of the wrong length or of another context; k outside [0, B); a bad stride, offset or column; a row outside y; a
 * non-finite alpha; a sharded context. */
int mgb_geo_dirichlet_on(mgb_geo g, const char* name, const uint8_t* facet_mask_or_null /* nf bytes */);
/* host arrays, each nullable: nb, the number of incidences nf q, rows nb, start nb + 1, idx nf q */
int mgb_geo_boundary_incidence(mgb_geo g, int* nb, int* ninc, int32_t* rows, int32_t* start, int32_t* idx);
int mgb_boundary_incidence(mgb_boundary b, int* nb, int* ninc, int32_t* rows, int32_t* start, int32_t* idx);
/* host only: the serial restatement of the load, out B x nb */
int mgb_geo_boundary_load_host(mgb_geo g, int B, const double* h /* B x nf x q */, const uint8_t* facet_mask_or_null, double* out);
int mgb_boundary_load(mgb_boundary b, int B, const double* h_host /* B x nf x q */, const uint8_t* mask_host_or_null,
                      mgb_vec out /* B x nb */);
int mgb_boundary_load_add(mgb_boundary b, mgb_vec load /* B x nb */, int k, double alpha, mgb_vec y, long long stride,
                          long long offset);
int mgb_amg_add_cost_rows(mgb_amg a, mgb_boundary b, mgb_vec load /* B x nb */, int k, double alpha, int col);

/* ---- host-only symbolic helpers (no GPU needed; used by the CPU test-suite) ----------------- */

typedef struct mgb_plan_s* mgb_plan;  /* symbolic products of one level: R, B=D*R, B', Hessian plan T */
int mgb_plan_create(mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D, int nq,
                    const int* idx_q, int idx_s, int level, mgb_plan* out);
/* host-only: doubles of reduction scratch an AMG with n_local rows and at most max_level_unknowns (global, replicated)
 * Newton unknowns per level allocates; the CPU suite checks it covers the 8-rank, 3-state-variable configurations */
int mgb_reduction_scratch_doubles(int n_local, int max_level_unknowns, long long* out);
int mgb_plan_destroy(mgb_plan p);
/* host-only: P with R_fine P = R_coarse from two level plans (what mgb_prolong applies); sizes first, then the arrays */
int mgb_plan_prolongation(mgb_plan fine, mgb_plan coarse, int* rows, int* cols, int* nnz, int32_t* rowptr, int32_t* colidx,
                          double* vals);
int mgb_plan_sizes(mgb_plan p, int* N, int* nnz_lower, int* nnz_T, int* nnz_B);
int mgb_plan_pattern(mgb_plan p, int32_t* rowptr, int32_t* colidx);
/* lower_vals = T * vec(Y) evaluated on the host: checks the plan against the reference's Hessian
 * recipe (test/test_matrix_addition.jl:39-95) in the CPU test-suite; not used by the product path */
int mgb_plan_eval_host(mgb_plan p, const double* Y /* n x nY */, double* lower_vals);
/* host-only timing of the multifrontal factorisation/solve of T*vec(Y) on this level's pattern */
/* host-only: the shard of a level plan that rank `rank` of `world` keeps (rows of B / R, columns of BT / T; the
 * pattern stays global), and host products with its B / BT -- the CPU test-suite checks with them that the
 * shards' contributions sum to the unsharded result */
int mgb_plan_shard(mgb_plan p, int S, int K, int rank, int world, int block, mgb_plan* out, int* r0, int* r1);
int mgb_plan_apply_B_host(mgb_plan p, const double* s /* N */, double* Bs /* n_local K */);
int mgb_plan_apply_BT_host(mgb_plan p, const double* v /* n_local K */, double* g /* N */);
int mgb_plan_chol_bench(mgb_plan p, const double* Y, int dim, int reps, double* seconds_per_factor,
                        double* seconds_per_solve, double* flops, double* front_doubles, double* residual);
/* host-only: the product's HOST multifrontal Cholesky (csrc/mfchol.cpp, what solver="host" factors with; worker threads
 * from the affinity mask) on this level's pattern, without a GPU: analyse once, then x = A \ g per Newton matrix.
 * bench.py's cpu_baseline times the Newton path on the host cores with it.  MGB_E_NUMERIC if a pivot is not positive. */
typedef struct mgb_hostchol_s* mgb_hostchol;
int mgb_plan_hostchol_create(mgb_plan p, int dim, mgb_hostchol* out);
int mgb_hostchol_destroy(mgb_hostchol c);
int mgb_hostchol_info(mgb_hostchol c, int* n, int* threads, double* flops);
int mgb_hostchol_factor_solve(mgb_hostchol c, const double* lower_vals, const double* g, double* x);
/* The factorisation split over the ranks of a sharded job (the reference's MUMPS is distributed over its MPI ranks,
 * README.md:23, tools/profile_ops.jl:117-126): the `world` subtrees log2(world) levels below the root of the elimination
 * tree go to one rank each, the separators above them are factored redundantly from the subtree roots' Schur complements.
 * partition: *split_world = ranks really used (1 = tree not splittable, everything replicated), owner[t] = rank of tree
 * node t (postorder, as mgb_plan_chol_tree), -1 = top.  factor_solve_dist: the host mirror of the device scheme; `fn`
 * sum-allreduces HOST doubles in place here.  Every rank passes the same values and right-hand side and gets all of x. */
int mgb_hostchol_partition(mgb_hostchol c, int world, int* split_world, int cap, int* nnodes, int* owner);
int mgb_hostchol_factor_solve_dist(mgb_hostchol c, int rank, int world, mgb_allreduce_fn fn, void* user,
                                   const double* lower_vals, const double* g, double* x);
/* Reduce-to-owner for the matrix entries (row (e); the reference's MUMPS takes distributed entries the same way): analysed
 * with the row partition of a `world`-rank job (`p` = the UNSHARDED plan, K = rows of D, block = rows per element), the top
 * log2(world) levels of the dissection follow the row blocks, subtree r is the interior of rank r's rows and all its matrix
 * entries are complete on rank r.  rank_aligned: *aligned = 1 if that held for every split (else the caller must sum the
 * values over the ranks as before), *top_values = entries among separator unknowns, the only ones that still travel.
 * factor_solve_dist_local: as factor_solve_dist, but `local_lower_vals` holds only THIS rank's row-block contributions
 * (mgb_plan_eval_host of its shard); the top entries ride in the Schur-complement collective.  g is replicated. */
int mgb_plan_hostchol_create_ranked(mgb_plan p, int dim, int K, int world, int block, mgb_hostchol* out);
int mgb_hostchol_rank_aligned(mgb_hostchol c, int world, int* aligned, int* top_values);
int mgb_hostchol_factor_solve_dist_local(mgb_hostchol c, int rank, int world, mgb_allreduce_fn fn, void* user,
                                         const double* local_lower_vals, const double* g, double* x);
/* host-only: the nested-dissection elimination tree of this level's pattern in postorder (children first):
 * own size, front size and parent (-1 = root) of the first min(cap, *nnodes) nodes */
int mgb_plan_chol_tree(mgb_plan p, int dim, int cap, int* nnodes, int* ns, int* nf, int* parent);
/* host-only: the tables of the fused backward sweep (csrc/bwd_fused.hpp) for this level's tree: cut = subtree height,
 * top_nf = largest front of a height the fused launch takes (<= 0: no limit), threads = its workgroup size.
 * info[12] = h_top, h_cut, workgroups, ints per workgroup record, levels per record, LDS solution entries, LDS reduction
 * doubles, LDS slot ints, LDS bytes, boundary entries, nodes, heights (workgroups = 0: no fused launch).  wg: the workgroup
 * records; bdry / slots: the concatenated boundary lists and the LDS slot of each entry; bofs / first: per node the offset
 * of its boundary list and its first own unknown.  Each array is filled up to its capacity. */
int mgb_plan_chol_bwd_fused(mgb_plan p, int dim, int cut, int top_nf, int threads, int* info, int cap_wg, int* wg, int cap_bdry,
                            int* bdry, int* slots, int cap_nodes, int* bofs, int* first);
/* host-only: the tables of the pre-mapped child contributions (csrc/chol_premap.hpp) for this level's tree under the
 * given knobs: leaf / single = MGB_CHOL_LEAF / MGB_CHOL_SINGLE, mode = MGB_CHOL_PREMAP, tiles = MGB_CHOL_PREMAP_TILES.
 * info[5] = nodes, heights, forward-map entries, inverse-map entries, slab doubles.  Per node (cap_nodes): height,
 * producer flag, soff (2 per node: slab offset per child slot, -1 = none), eoff (slab it stores into, -1 = its own front),
 * fofs (start of its forward map: nb + 1 entries, boundary row -> parent front row, the last one the parent's
 * right-hand-side row; -1 = root), iofs (start of its two (nf + 1)-long inverse maps, -1 = no children).  Per height
 * (cap_heights): hkind (0 Leaf, 1 Single*, 2 Start + panels), hwg (workgroups of its first launch), hconsumer (that launch
 * reads the slabs).  fwd / pinv: the maps.  Each array is nullable and filled up to its capacity. */
int mgb_plan_chol_premap(mgb_plan p, int dim, int leaf, int single, int mode, int tiles, long long* info, int cap_nodes, int* height,
                         int* producer, long long* soff, long long* eoff, int* fofs, int* iofs, int cap_heights, int* hkind, int* hwg,
                         int* hconsumer, int cap_fwd, int* fwd, int cap_pinv, int* pinv);
/* host-only: the whole plan of the device chain (csrc/chol_plan.hpp, plan_chain) for this level's tree: every launch and
 * every job, as GpuChol::build would upload them.  knobs (nullable: the values this process reads from the environment):
 * 16 ints in CholKnobs order -- graph, prof, leaf, single, step2, wide, start_pivot, step2_tiles, dense_tiles,
 * bwd_split_nf, bwd_fused, bwd_cut, bwd_fused_nf, bwd_fused_threads, premap, premap_tiles.  world / rank: the subtree
 * split (1, 0: the unsplit chain).  info[10] = launches, first own backward launch, first top launch, list entries,
 * start jobs, tiles, single tiles, rect jobs, assembly entries, world the tree was split over (1: not splittable).
 * launch: 10 ints per launch -- kind (codes of mgb_amg_chol_schedule), job offset, job count (= workgroups), block size,
 * LDS bytes, first panel p, leading pivot jobs npiv, rect, pre-map consumer flag, pre-map producers.  lists: the node
 * lists (Leaf, Bwd*); starts: node, chunk, rb (-1: pivot job), a0, a1 per job; tiles / singles: node, ti, tj per job;
 * rects: node, chunk per job; apos / asrc (cap_asm each): the assembly lists.  Each array is nullable and filled up to
 * its capacity. */
int mgb_plan_chol_schedule(mgb_plan p, int dim, const int* knobs, int world, int rank, int* info, int cap_launch, int* launch,
                           int cap_lists, int* lists, int cap_starts, int* starts, int cap_tiles, int* tiles, int cap_singles,
                           int* singles, int cap_rects, int* rects, int cap_asm, int* apos, int* asrc);
int mgb_chol_selftest(int nx, int ny, double* max_residual, double* flops, double* seconds);
/* test hook: the finish launch of the two-stage field reductions (csrc/reduce.hpp) alone, on the context's stream.
 * partials_host: rows x nwg x 5 (three sums, two NaN-sticky maxima per partial); out_host: rows x 5. */
int mgb_reduce_selftest(mgb_ctx ctx, int rows, int nwg, const double* partials_host, double* out_host);

#ifdef __cplusplus
}
#endif
#endif /* MGB_HIP_H */
