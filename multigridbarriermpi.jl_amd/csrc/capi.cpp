// C ABI of libmgb_hip.so (include/mgb_hip.h): exception firewall + handle plumbing.
#include "../../include/mgb_hip.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "amg.hpp"
#include "boundary.hpp"
#include "interp.hpp"
#include "isosurface.hpp"
#include "energy.hpp"
#include "estimate.hpp"
#include "flowline.hpp"
#include "pathline.hpp"
#include "ray.hpp"
#include "levelset.hpp"
#include "mixed.hpp"
#include "norms.hpp"
#include "section.hpp"
#include "timestat.hpp"

using namespace mgb;

struct mgb_ctx_s {
  Ctx ctx;
  explicit mgb_ctx_s(int dev) : ctx(dev) {}
};
struct mgb_geo_s {
  GeometryHost g;
};
struct mgb_vec_s {
  mgb_ctx_s* ctx;
  DevBuf<double> buf;
  int n;
};
struct mgb_csr_s {
  mgb_ctx_s* ctx;
  DevCsrOwned A;
  Csr host;      // structure + values as uploaded: SparseMatrixCSC(x) gathers (src:371) and the setup-time sparse algebra
};
struct mgb_amg_s {
  mgb_ctx_s* ctx;
  std::unique_ptr<Amg> amg;
  SolveStats stats;
  bool schedule_all = false;
  bool host_solve = false;
  bool pcg = false;
  bool upstream_stop = false;
  bool exact_centering = true;
  bool time_kernels = true;
};
struct mgb_locator_s {
  mgb_ctx_s* ctx;
  interp::Locator loc;
  DevBuf<int> cellptr, cellelem;
  DevBuf<double> x, w;
  DevBuf<double> norm_scratch;      // mgb_field_norms: partials and results, grown on demand
  DevBuf<long long> norm_counts;
  DevBuf<double> energy_scratch;                   // mgb_geo_field_energy: partials and results, grown on demand
  DevBuf<const double*> energy_table;              // ... and the device table of field pointers, uploaded per call
  DevBuf<double> ls_scratch, ls_levels;            // mgb_geo_level_sets: partials, results and totals; the levels of the call
  DevBuf<long long> ls_counts, ls_row_base;        // ... per-workgroup counts and offsets; the first slot of every row
  DevBuf<const double*> ls_table;                  // ... and the device table of field pointers, uploaded per call
  DevBuf<double> fl_seeds, fl_out, fl_pts;         // mgb_geo_flow_lines: seeds; rows and end points; the fixed-stride paths
  DevBuf<int32_t> fl_int, fl_pelem;                // ... status, count, end element; the elements of the path points
  DevBuf<long long> fl_offsets;                    // ... the first point of every row in the compacted paths
  DevBuf<const double*> fl_table;                  // ... and the device table of field pointers, uploaded per call
  DevBuf<double> pl_ts;                            // mgb_geo_path_lines (which shares the fl_ buffers): the snapshot times ...
  DevBuf<int32_t> pl_release;                      // ... and the release indices of the call
  DevBuf<double> ry_ab, ry_rows;                   // mgb_geo_line_integrals: start and end points; the rows of the call
  DevBuf<int32_t> ry_count;                        // ... the owned pieces of every row
  DevBuf<long long> ry_offsets;                    // ... the first piece of every row
  DevBuf<const double*> ry_table;                  // ... and the device table of field pointers, uploaded per call
  DevBuf<double> tst_scratch;                      // mgb_geo_time_stats: partials and results, grown on demand
  DevBuf<uint64_t> tst_uniform;                    // ... snapshot pointers, steps, times and levels of the call, uploaded in one copy
};
struct mgb_flowpath_s {
  mgb_ctx_s* ctx;
  int dim;
  std::vector<long long> offsets;                  // B m + 1
  DevBuf<double> pts;                              // total x dim
  DevBuf<int32_t> elem;                            // total
};
struct mgb_levelset_s {
  mgb_ctx_s* ctx;
  int width;                                       // doubles per row: segments 4 in 2-D and 2 in 1-D, triangles (mgb_geo_isosurfaces) 9,
                                                   // pieces of a cut (mgb_geo_sections) 6 in 2-D and 12 in 3-D, pieces of a
                                                   // segment (mgb_geo_line_integrals) 3
  std::vector<long long> row_offsets;              // B nl + 1
  DevBuf<double> seg;
  DevBuf<int32_t> item;
};
struct mgb_boundary_s {
  mgb_locator_s* loc;      // not owned: the locator (x, w, context) must outlive the boundary
  boundary::Facets F;
  DevBuf<int> nodes;
  DevBuf<double> weights, normal;
  DevBuf<unsigned char> mask;                      // mgb_boundary_flux: the facet mask of the call
  DevBuf<double> scratch, facet_scratch;           // ... partials and results, per-facet values, grown on demand
  DevBuf<const double*> table;                     // ... and the device table of field pointers, uploaded per call
  boundary::Incidence inc;                         // mgb_boundary_load: the row-sorted incidence table, built with the facets
  DevBuf<int> inc_rows, inc_start, inc_idx;
  DevBuf<double> load_h;                           // ... the B x nf x q data of the call, grown on demand
  boundary::Interior I;                            // mgb_estimate: the interior facets and the element -> facet table, built with the facets
  DevBuf<int> inodes, elem_facet;
  DevBuf<double> iweights, inormal;
  DevBuf<double> est_sigma, est_J, est_N, est_scratch, est_h;      // ... flux, per-facet values, partials, Neumann data: grown on demand
  DevBuf<double> est_dt;                           // mgb_estimate_steps: the step sizes of the call ...
  DevBuf<const double*> est_table;                 // ... and the device table of its snapshots, uploaded per call
};
struct mgb_plan_s {
  LevelPlan plan;
  int n, nY;
};
struct mgb_hostchol_s {
  MfChol ch;
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// exception firewall: the status code comes from the exception TYPE (errors.hpp), never from its message
template <class F>
int guard(F&& fn) {
  try {
    fn();
    return MGB_OK;
  } catch (const HipError& e) {
    return fail(MGB_E_HIP, e.what());
  } catch (const NumericError& e) {
    return fail(MGB_E_NUMERIC, e.what());
  } catch (const std::invalid_argument& e) {      // ArgError and need()
    return fail(MGB_E_ARG, e.what());
  } catch (const std::out_of_range& e) {
    return fail(MGB_E_ARG, e.what());
  } catch (const std::bad_alloc&) {
    return fail(MGB_E_INTERNAL, "out of host memory");
  } catch (const std::exception& e) {
    return fail(MGB_E_INTERNAL, e.what());
  } catch (...) {
    return fail(MGB_E_INTERNAL, "unknown exception");
  }
}

void need(bool cond, const char* msg) {
  if (!cond) throw std::invalid_argument(msg);
}

Csr make_csr(int rows, int cols, const int32_t* rowptr, const int32_t* colidx, const double* vals, const char* what) {
  need(rows >= 0 && cols >= 0 && rowptr, "CSR: null rowptr or negative size");
  Csr A(rows, cols);
  A.rowptr.assign(rowptr, rowptr + rows + 1);
  const int nnz = rowptr[rows];
  need(nnz >= 0 && (nnz == 0 || (colidx && vals)), "CSR: null colidx/vals");
  A.colidx.assign(colidx, colidx + nnz);
  A.vals.assign(vals, vals + nnz);
  check_csr(A, what);
  return A;
}

// "sub:dirichlet:2" -> parts
std::vector<std::string> split(const std::string& s) {
  std::vector<std::string> out;
  size_t p = 0;
  for (;;) {
    size_t q = s.find(':', p);
    out.push_back(s.substr(p, q == std::string::npos ? q : q - p));
    if (q == std::string::npos) break;
    p = q + 1;
  }
  return out;
}

Csr* find_matrix(GeometryHost& g, const std::string& name, bool create) {
  auto parts = split(name);
  if (parts.size() == 2 && parts[0] == "op") {
    if (create) return &g.operators[parts[1]];
    auto it = g.operators.find(parts[1]);
    return it == g.operators.end() ? nullptr : &it->second;
  }
  if (parts.size() == 3 && parts[0] == "sub") {
    int l = atoi(parts[2].c_str());
    if (l < 0 || l >= g.L) return nullptr;
    if (create) {
      auto& v = g.subspaces[parts[1]];
      if ((int)v.size() < g.L) v.resize(g.L);
      return &v[l];
    }
    auto it = g.subspaces.find(parts[1]);
    if (it == g.subspaces.end() || l >= (int)it->second.size()) return nullptr;
    return &it->second[l];
  }
  if (parts.size() == 2 && (parts[0] == "refine" || parts[0] == "coarsen")) {
    int l = atoi(parts[1].c_str());
    if (l < 0 || l >= g.L) return nullptr;
    auto& v = parts[0] == "refine" ? g.refine : g.coarsen;
    if (create && (int)v.size() < g.L) v.resize(g.L);
    if (l >= (int)v.size()) return nullptr;
    return &v[l];
  }
  return nullptr;
}

AmgSpec make_spec(int S, const char* const* sv, int K, const char* const* D) {
  need(S >= 1 && K >= 1 && sv && D, "amg: empty state_variables or D");
  AmgSpec spec;
  for (int i = 0; i < S; ++i) {
    need(sv[2 * i] && sv[2 * i + 1], "amg: null string");
    spec.state_variables.emplace_back(sv[2 * i], sv[2 * i + 1]);
  }
  for (int k = 0; k < K; ++k) {
    need(D[2 * k] && D[2 * k + 1], "amg: null string");
    spec.D.emplace_back(D[2 * k], D[2 * k + 1]);
  }
  return spec;
}

BarrierParams make_params_cones(int K, int ncones, const int* nq, const int* idx_q, const int* idx_s,
                                const int* idx_s2, const double* p) {
  need(ncones >= 1 && ncones <= 2 && nq && idx_q && idx_s && p, "barrier: 1 or 2 cones expected");
  BarrierParams P;
  P.K = K;
  P.ncones = ncones;
  for (int c = 0; c < ncones; ++c) {
    ConeSpec& S = P.cone[c];
    need(nq[c] >= 1 && nq[c] <= 3, "barrier: nq must be 1..3");
    need(p[c] >= 1.0 && std::isfinite(p[c]), "barrier: p must be >= 1");
    S.nq = nq[c];
    for (int i = 0; i < nq[c]; ++i) {
      need(idx_q[3 * c + i] >= 0 && idx_q[3 * c + i] < K, "barrier: idx_q out of range");
      S.iq[i] = idx_q[3 * c + i];
    }
    need(idx_s[c] >= 0 && idx_s[c] < K, "barrier: idx_s out of range");
    S.is = idx_s[c];
    S.is2 = idx_s2 ? idx_s2[c] : -1;
    need(S.is2 < K, "barrier: idx_s2 out of range");
    if (S.is2 < 0) S.is2 = -1;
    // the active columns q_1..q_nq, s [, s2] must be distinct: expand_hessian_rows_kernel and the assembly give every pair of
    // active columns ONE off-diagonal slot, which is only right when the pair names two different rows of D
    for (int a = 0; a < S.nact(); ++a)
      for (int b = 0; b < a; ++b) need(S.col(a) != S.col(b), "barrier: repeated column in a power cone");
    S.a = 2.0 / p[c];
    S.mu = (p[c] == 2.0) ? 0.0 : (p[c] < 2.0 ? 1.0 : 2.0);
  }
  return P;
}

// general menu: term c is a power cone (kind 0: nq, idx_q, idx_s, idx_s2, p as above) or a half space (kind 1: columns
// idx_q[3c .. 3c + nq), coefficients coef[3c ..], constant offset off[c]; idx_s / p ignored)
BarrierParams make_params_terms(int K, int nterms, const int* kind, const int* nq, const int* idx_q, const int* idx_s,
                                const int* idx_s2, const double* p, const double* coef, const double* off) {
  need(nterms >= 1 && nterms <= kMaxCones && kind && nq && idx_q, "barrier: 1 to 3 terms expected");
  BarrierParams P;
  P.K = K;
  P.ncones = nterms;
  for (int c = 0; c < nterms; ++c) {
    if (kind[c] == 0) {
      need(idx_s && p, "barrier: power cone needs idx_s and p");
      const int is2 = idx_s2 ? idx_s2[c] : -1;
      BarrierParams one = make_params_cones(K, 1, nq + c, idx_q + 3 * c, idx_s + c, &is2, p + c);
      P.cone[c] = one.cone[0];
    } else {
      need(kind[c] == 1, "barrier: unknown term kind");
      need(coef && off && nq[c] >= 1 && nq[c] <= 3, "barrier: half space needs 1..3 columns, coef and off");
      ConeSpec& S = P.cone[c];
      S.kind = 1;
      S.nq = nq[c];
      bool any = false;
      for (int i = 0; i < nq[c]; ++i) {
        need(idx_q[3 * c + i] >= 0 && idx_q[3 * c + i] < K, "barrier: idx_q out of range");
        for (int j = 0; j < i; ++j) need(idx_q[3 * c + j] != idx_q[3 * c + i], "barrier: repeated column in a half space");
        need(std::isfinite(coef[3 * c + i]), "barrier: coefficient not finite");
        S.iq[i] = idx_q[3 * c + i];
        S.coef[i] = coef[3 * c + i];
        any = any || coef[3 * c + i] != 0.0;
      }
      need(any && std::isfinite(off[c]), "barrier: half space needs a nonzero coefficient and a finite offset");
      S.is = S.iq[0];      // unused by kind 1; keep indices in range
      S.is2 = -1;
      S.off = off[c];
      S.a = 1.0;
      S.mu = 0.0;
    }
  }
  return P;
}

BarrierParams make_params(int K, int nq, const int* idx_q, int idx_s, double p) {
  need(nq >= 1 && nq <= 3 && idx_q, "barrier: nq must be 1..3");
  int iq3[3] = {0, 0, 0};
  for (int i = 0; i < nq; ++i) iq3[i] = idx_q[i];
  return make_params_cones(K, 1, &nq, iq3, &idx_s, nullptr, &p);
}

mgb_csr_s* new_csr(mgb_ctx_s* ctx, Csr&& A) {
  hip_check(hipSetDevice(ctx->ctx.device), "hipSetDevice");
  auto* m = new mgb_csr_s{ctx, {}, {}};
  try {
    m->A.upload(A);
    m->host = std::move(A);
  } catch (...) {
    delete m;
    throw;
  }
  return m;
}

// one scalar reduction of a device vector through `launch` (dot / sum), result on the host
template <class Launch>
double reduce_scalar(mgb_vec x, Launch&& launch) {
  if (x->n == 0) return 0.0;
  hipStream_t st = x->ctx->ctx.stream;
  const int nb = f0_blocks(x->n);
  DevBuf<double> scratch;
  scratch.alloc((size_t)kReductionHeader + nb + 1);      // ticket words | partials | result
  hip_check(hipMemsetAsync(scratch.p, 0, kReductionHeader * sizeof(double), st), "memset ticket");
  launch(st, scratch.p, scratch.p + kReductionHeader + nb);
  hip_check(hipGetLastError(), "reduction launch");
  hip_check(hipStreamSynchronize(st), "sync reduction");
  double out = 0.0;
  hip_check(hipMemcpy(&out, scratch.p + kReductionHeader + nb, sizeof(double), hipMemcpyDeviceToHost), "D2H");
  return out;
}

}  // namespace

extern "C" {

const char* mgb_last_error(void) { return g_err.c_str(); }
int mgb_version(void) { return 100; }
int mgb_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int mgb_ctx_create(int device_id, mgb_ctx* out) {
  return guard([&] {
    need(out, "null out");
    *out = new mgb_ctx_s(device_id);
  });
}
int mgb_ctx_destroy(mgb_ctx ctx) {
  return guard([&] { delete ctx; });
}
int mgb_ctx_synchronize(mgb_ctx ctx) {
  return guard([&] {
    need(ctx, "null ctx");
    hip_check(hipStreamSynchronize(ctx->ctx.stream), "sync");
  });
}

int mgb_ctx_set_comm(mgb_ctx ctx, int rank, int world, mgb_allreduce_fn fn, void* user) {
  return guard([&] {
    need(ctx && world >= 1 && rank >= 0 && rank < world && (world == 1 || fn), "ctx_set_comm: bad arguments");
    ctx->ctx.drop_comm();
    ctx->ctx.rank = rank;
    ctx->ctx.world = world;
    ctx->ctx.allreduce = fn;
    ctx->ctx.allreduce_user = user;
  });
}
int mgb_rccl_unique_id(char* out128) {
  return guard([&] {
    need(out128, "rccl_unique_id: null output");
    rccl_unique_id(out128);
  });
}
int mgb_ctx_set_comm_rccl(mgb_ctx ctx, const char* unique_id128, int rank, int world) {
  return guard([&] {
    need(ctx, "null ctx");
    ctx->ctx.set_comm_rccl(unique_id128, rank, world);
  });
}
int mgb_ctx_comm_stats(mgb_ctx ctx, long long* calls, double* bytes) {
  return guard([&] {
    need(ctx, "null ctx");
    if (calls) *calls = ctx->ctx.n_allreduce;
    if (bytes) *bytes = ctx->ctx.allreduce_bytes;
  });
}
int mgb_shard_rows(int rank, int world, int n, int block, int* r0, int* r1) {
  return guard([&] {
    need(r0 && r1, "shard_rows: null output");
    shard_rows(rank, world, n, block, r0, r1);
  });
}

int mgb_fem1d_native(int L, mgb_geo* out) {
  return guard([&] {
    need(out, "null out");
    auto* g = new mgb_geo_s;
    try {
      g->g = fem1d_native(L);
    } catch (...) {
      delete g;
      throw;
    }
    *out = g;
  });
}
int mgb_fem2d_native(int L, const double* K, int nK_rows, mgb_geo* out) {
  return guard([&] {
    need(out, "null out");
    auto* g = new mgb_geo_s;
    try {
      g->g = fem2d_native(L, K, nK_rows);
    } catch (...) {
      delete g;
      throw;
    }
    *out = g;
  });
}
int mgb_fem3d_native(int L, int k, mgb_geo* out) {
  return guard([&] {
    need(out, "null out");
    auto* g = new mgb_geo_s;
    try {
      g->g = fem3d_native(L, k);
    } catch (...) {
      delete g;
      throw;
    }
    *out = g;
  });
}
int mgb_geo_create(int n, int dim, int L, int block, const double* x, const double* w, mgb_geo* out) {
  return guard([&] {
    need(out && x && w && n > 0 && dim >= 1 && dim <= 3 && L >= 1 && block >= 1, "geo_create: bad arguments");
    auto* g = new mgb_geo_s;
    g->g.n = n;
    g->g.dim = dim;
    g->g.L = L;
    g->g.block = block;
    g->g.x.assign(x, x + (size_t)n * dim);
    g->g.w.assign(w, w + n);
    *out = g;
  });
}
int mgb_geo_set_matrix(mgb_geo g, const char* name, int rows, int cols, const int32_t* rowptr, const int32_t* colidx,
                       const double* vals) {
  return guard([&] {
    need(g && name, "null argument");
    Csr A = make_csr(rows, cols, rowptr, colidx, vals, name);
    Csr* dst = find_matrix(g->g, name, true);
    need(dst != nullptr, "geo_set_matrix: unknown matrix name");
    *dst = std::move(A);
  });
}
int mgb_geo_destroy(mgb_geo g) {
  return guard([&] { delete g; });
}
int mgb_geo_dims(mgb_geo g, int* n, int* dim, int* L, int* block) {
  return guard([&] {
    need(g, "null geo");
    if (n) *n = g->g.n;
    if (dim) *dim = g->g.dim;
    if (L) *L = g->g.L;
    if (block) *block = g->g.block;
  });
}
int mgb_geo_get_xw(mgb_geo g, double* x, double* w) {
  return guard([&] {
    need(g, "null geo");
    if (x) std::copy(g->g.x.begin(), g->g.x.end(), x);
    if (w) std::copy(g->g.w.begin(), g->g.w.end(), w);
  });
}
int mgb_geo_matrix_info(mgb_geo g, const char* name, int* rows, int* cols, int* nnz) {
  return guard([&] {
    need(g && name, "null argument");
    Csr* A = find_matrix(g->g, name, false);
    need(A != nullptr, "geo_matrix_info: unknown matrix name");
    if (rows) *rows = A->rows;
    if (cols) *cols = A->cols;
    if (nnz) *nnz = A->nnz();
  });
}
int mgb_geo_matrix_get(mgb_geo g, const char* name, int32_t* rowptr, int32_t* colidx, double* vals) {
  return guard([&] {
    need(g && name, "null argument");
    Csr* A = find_matrix(g->g, name, false);
    need(A != nullptr, "geo_matrix_get: unknown matrix name");
    if (rowptr) std::copy(A->rowptr.begin(), A->rowptr.end(), rowptr);
    if (colidx) std::copy(A->colidx.begin(), A->colidx.end(), colidx);
    if (vals) std::copy(A->vals.begin(), A->vals.end(), vals);
  });
}

// ---- device vectors / matrices
int mgb_vec_create(mgb_ctx ctx, int n, const double* host, mgb_vec* out) {
  return guard([&] {
    need(ctx && out && n >= 0, "vec_create: bad arguments");
    hip_check(hipSetDevice(ctx->ctx.device), "hipSetDevice");
    auto* v = new mgb_vec_s{ctx, {}, n};
    try {
      v->buf.alloc(n);
      if (host) v->buf.upload(host, n);
      else if (n)  // stream-ordered: a null-stream memset is not ordered against the non-blocking context stream
        hip_check(hipMemsetAsync(v->buf.p, 0, (size_t)n * sizeof(double), ctx->ctx.stream), "memset");
    } catch (...) {
      delete v;
      throw;
    }
    *out = v;
  });
}
int mgb_vec_free(mgb_vec v) {
  return guard([&] { delete v; });
}
int mgb_vec_len(mgb_vec v, int* n) {
  return guard([&] {
    need(v && n, "null argument");
    *n = v->n;
  });
}
int mgb_vec_upload(mgb_vec v, const double* host) {
  return guard([&] {
    need(v && host, "null argument");
    hip_check(hipStreamSynchronize(v->ctx->ctx.stream), "sync");
    v->buf.upload(host, v->n);
  });
}
int mgb_vec_download(mgb_vec v, double* host) {
  return guard([&] {
    need(v && host, "null argument");
    hip_check(hipStreamSynchronize(v->ctx->ctx.stream), "sync");
    v->buf.download(host, v->n);
  });
}
int mgb_csr_create(mgb_ctx ctx, int rows, int cols, const int32_t* rowptr, const int32_t* colidx, const double* vals,
                   mgb_csr* out) {
  return guard([&] {
    need(ctx && out, "null argument");
    hip_check(hipSetDevice(ctx->ctx.device), "hipSetDevice");
    Csr A = make_csr(rows, cols, rowptr, colidx, vals, "mgb_csr_create");
    *out = new_csr(ctx, std::move(A));
  });
}
int mgb_csr_free(mgb_csr A) {
  return guard([&] { delete A; });
}
int mgb_csr_dims(mgb_csr A, int* rows, int* cols, int* nnz) {
  return guard([&] {
    need(A, "null argument");
    if (rows) *rows = A->host.rows;
    if (cols) *cols = A->host.cols;
    if (nnz) *nnz = A->host.nnz();
  });
}
int mgb_csr_get(mgb_csr A, int32_t* rowptr, int32_t* colidx, double* vals) {
  return guard([&] {
    need(A, "null argument");
    if (rowptr) std::copy(A->host.rowptr.begin(), A->host.rowptr.end(), rowptr);
    if (colidx) std::copy(A->host.colidx.begin(), A->host.colidx.end(), colidx);
    if (vals) std::copy(A->host.vals.begin(), A->host.vals.end(), vals);
  });
}
int mgb_csr_spgemm(mgb_csr A, mgb_csr B, mgb_csr* out) {
  return guard([&] {
    need(A && B && out, "null argument");
    *out = new_csr(A->ctx, spgemm(A->host, B->host));
  });
}
int mgb_csr_transpose(mgb_csr A, mgb_csr* out) {
  return guard([&] {
    need(A && out, "null argument");
    *out = new_csr(A->ctx, transpose(A->host));
  });
}
int mgb_csr_add(mgb_csr A, double alpha, mgb_csr B, mgb_csr* out) {
  return guard([&] {
    need(A && B && out, "null argument");
    *out = new_csr(A->ctx, add(A->host, alpha, B->host));
  });
}
static std::vector<const Csr*> host_list(int count, const mgb_csr* mats) {
  need(count >= 1 && mats, "empty matrix list");
  std::vector<const Csr*> v;
  for (int i = 0; i < count; ++i) {
    need(mats[i] != nullptr, "null matrix in list");
    v.push_back(&mats[i]->host);
  }
  return v;
}
int mgb_csr_hcat(int count, const mgb_csr* mats, mgb_csr* out) {
  return guard([&] {
    need(out, "null argument");
    auto v = host_list(count, mats);
    *out = new_csr(mats[0]->ctx, hcat(v));
  });
}
int mgb_csr_blockdiag(int count, const mgb_csr* mats, mgb_csr* out) {
  return guard([&] {
    need(out, "null argument");
    auto v = host_list(count, mats);
    *out = new_csr(mats[0]->ctx, blockdiag(v));
  });
}
int mgb_diag(mgb_ctx ctx, mgb_vec z, int m, int n, mgb_csr* out) {
  return guard([&] {
    need(ctx && z && out && m >= 0 && n >= 0, "diag: bad arguments");
    const int d = std::min(std::min(m, n), z->n);
    std::vector<double> h(z->n);
    hip_check(hipStreamSynchronize(ctx->ctx.stream), "sync");
    z->buf.download(h.data(), z->n);
    Csr A(m, n);
    for (int i = 0; i < m; ++i) {
      if (i < d) {
        A.colidx.push_back(i);
        A.vals.push_back(h[i]);
      }
      A.rowptr[i + 1] = (int)A.colidx.size();
    }
    *out = new_csr(ctx, std::move(A));
  });
}
int mgb_spmv_add(mgb_csr A, mgb_vec x, mgb_vec y0, mgb_vec y) {
  return guard([&] {
    need(A && x && y, "null argument");
    need(A->A.view.cols == x->n && A->A.view.rows == y->n && (!y0 || y0->n == y->n), "spmv: shape mismatch");
    launch_spmv(A->ctx->ctx.stream, A->A.view, x->buf.p, y0 ? y0->buf.p : nullptr, y->buf.p);
    hip_check(hipGetLastError(), "spmv launch");
  });
}
int mgb_spmv(mgb_csr A, mgb_vec x, mgb_vec y) { return mgb_spmv_add(A, x, nullptr, y); }
int mgb_dot(mgb_vec x, mgb_vec y, double* out) {
  return guard([&] {
    need(x && y && out && x->n == y->n, "dot: shape mismatch");
    *out = reduce_scalar(x, [&](hipStream_t st, double* parts, double* res) { launch_dot(st, x->n, x->buf.p, y->buf.p, parts, res); });
  });
}
int mgb_norm(mgb_vec x, double* out) {
  return guard([&] {
    need(x && out, "null argument");
    *out = std::sqrt(reduce_scalar(x, [&](hipStream_t st, double* parts, double* res) { launch_dot(st, x->n, x->buf.p, x->buf.p, parts, res); }));
  });
}
int mgb_sum(mgb_vec x, double* out) {
  return guard([&] {
    need(x && out, "null argument");
    *out = reduce_scalar(x, [&](hipStream_t st, double* parts, double* res) { launch_sum(st, x->n, x->buf.p, parts, res); });
  });
}
int mgb_col_extract(mgb_vec M, int n, int K, int k, mgb_vec out) {
  return guard([&] {
    need(M && out && n >= 0 && K >= 1 && k >= 0 && k < K, "col_extract: bad arguments");
    need((long long)n * K == M->n && out->n == n, "col_extract: shape mismatch");
    launch_col_extract(M->ctx->ctx.stream, n, K, k, M->buf.p, out->buf.p);
    hip_check(hipGetLastError(), "col_extract launch");
  });
}
int mgb_map_rows_barrier(int which, int K, int nterms, const int* kind, const int* nq, const int* idx_q, const int* idx_s,
                         const int* idx_s2, const double* p, const double* coef, const double* off, int n, mgb_vec Dz,
                         mgb_vec out) {
  return guard([&] {
    need(Dz && out && n >= 0 && K >= 1 && K <= 8 && which >= 0 && which <= 2, "map_rows_barrier: bad arguments");
    BarrierParams P = make_params_terms(K, nterms, kind, nq, idx_q, idx_s, idx_s2, p, coef, off);
    const long long want = which == 0 ? n : (which == 1 ? (long long)n * K : (long long)n * K * K);
    need((long long)n * K == Dz->n && out->n == want, "map_rows_barrier: shape mismatch");
    hipStream_t st = Dz->ctx->ctx.stream;
    hip_check(hipSetDevice(Dz->ctx->ctx.device), "hipSetDevice");
    if (which == 0) {
      launch_barrier_rows_F(st, n, P, Dz->buf.p, out->buf.p);
    } else {
      // the fused kernels of the Newton path with unit weights: F1 = barrier_f1(w = 1, c = 0), F2 = barrier_f2(w = 1)
      std::vector<double> ones((size_t)std::max(n, 1), 1.0);
      DevBuf<double> w;
      w.upload(ones.data(), ones.size());
      if (which == 1) {
        DevBuf<double> c;
        c.alloc((size_t)std::max(n, 1) * K);
        hip_check(hipMemsetAsync(c.p, 0, c.n * sizeof(double), st), "memset");
        if (n) launch_barrier_f1(st, n, P, Dz->buf.p, w.p, c.p, 0.0, out->buf.p);
        hip_check(hipStreamSynchronize(st), "sync");      // c, w die with this scope
      } else {
        DevBuf<double> Y;
        Y.alloc((size_t)std::max(n, 1) * P.nY());
        if (n) launch_barrier_f2(st, n, P, Dz->buf.p, w.p, Y.p);
        launch_expand_hessian_rows(st, n, P, Y.p, out->buf.p);
        hip_check(hipStreamSynchronize(st), "sync");
      }
    }
    hip_check(hipGetLastError(), "map_rows_barrier launch");
  });
}
int mgb_mul(mgb_vec x, mgb_vec y, mgb_vec out) {
  return guard([&] {
    need(x && y && out && x->n == y->n && x->n == out->n, "mul: shape mismatch");
    launch_mul(x->ctx->ctx.stream, x->n, x->buf.p, y->buf.p, out->buf.p);
  });
}
int mgb_axpy(mgb_vec x, double alpha, mgb_vec y, mgb_vec out) {
  return guard([&] {
    need(x && y && out && x->n == y->n && x->n == out->n, "axpy: shape mismatch");
    launch_waxpby(x->ctx->ctx.stream, x->n, x->buf.p, alpha, y->buf.p, out->buf.p);
  });
}
int mgb_vec_allreduce_sum(mgb_vec x) {
  return guard([&] {
    need(x, "null argument");
    x->ctx->ctx.allreduce_sum(x->buf.p, x->n, /*even_single=*/true);
    hip_check(hipStreamSynchronize(x->ctx->ctx.stream), "sync allreduce");      // a library-owned communicator works on the stream
  });
}
int mgb_all_isfinite(mgb_vec x, int* out) {
  return guard([&] {
    need(x && out, "null argument");
    hipStream_t st = x->ctx->ctx.stream;
    DevBuf<int> flag;
    flag.alloc(1);
    launch_all_isfinite(st, x->n, x->buf.p, flag.p);
    hip_check(hipStreamSynchronize(st), "sync");
    int h = 0;
    flag.download(&h, 1);
    *out = h != 0;
  });
}

// ---- AMG
int mgb_amg_create(mgb_ctx ctx, mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D, int nq,
                   const int* idx_q, int idx_s, double p, mgb_amg* out) {
  return guard([&] {
    need(ctx && g && out, "null argument");
    AmgSpec spec = make_spec(S, state_vars, K, D);
    BarrierParams P = make_params(K, nq, idx_q, idx_s, p);
    auto* a = new mgb_amg_s{ctx, nullptr, {}};
    try {
      const auto t0 = std::chrono::steady_clock::now();
      a->amg.reset(new Amg(ctx->ctx, g->g, spec, P));
      a->stats.t_setup = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) {
      delete a;
      throw;
    }
    *out = a;
  });
}
int mgb_amg_create_cones(mgb_ctx ctx, mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D,
                         int ncones, const int* nq, const int* idx_q, const int* idx_s, const int* idx_s2,
                         const double* p, mgb_amg* out) {
  return guard([&] {
    need(ctx && g && out, "null argument");
    AmgSpec spec = make_spec(S, state_vars, K, D);
    BarrierParams P = make_params_cones(K, ncones, nq, idx_q, idx_s, idx_s2, p);
    auto* a = new mgb_amg_s{ctx, nullptr, {}};
    try {
      const auto t0 = std::chrono::steady_clock::now();
      a->amg.reset(new Amg(ctx->ctx, g->g, spec, P));
      a->stats.t_setup = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) {
      delete a;
      throw;
    }
    *out = a;
  });
}
int mgb_amg_create_terms(mgb_ctx ctx, mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D, int nterms,
                         const int* kind, const int* nq, const int* idx_q, const int* idx_s, const int* idx_s2, const double* p,
                         const double* coef, const double* off, mgb_amg* out) {
  return guard([&] {
    need(ctx && g && out, "null argument");
    AmgSpec spec = make_spec(S, state_vars, K, D);
    BarrierParams P = make_params_terms(K, nterms, kind, nq, idx_q, idx_s, idx_s2, p, coef, off);
    auto* a = new mgb_amg_s{ctx, nullptr, {}};
    try {
      const auto t0 = std::chrono::steady_clock::now();
      a->amg.reset(new Amg(ctx->ctx, g->g, spec, P));
      a->stats.t_setup = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } catch (...) {
      delete a;
      throw;
    }
    *out = a;
  });
}
int mgb_amg_destroy(mgb_amg a) {
  return guard([&] { delete a; });
}
int mgb_amg_dims(mgb_amg a, int* n, int* S, int* K, int* L, int* nY) {
  return guard([&] {
    need(a, "null amg");
    if (n) *n = a->amg->n();
    if (S) *S = a->amg->S();
    if (K) *K = a->amg->K();
    if (L) *L = a->amg->L();
    if (nY) *nY = a->amg->params().nY();
  });
}
int mgb_amg_local_rows(mgb_amg a, int* n_global, int* row0, int* n_local) {
  return guard([&] {
    need(a, "null amg");
    if (n_global) *n_global = a->amg->n_global();
    if (row0) *row0 = a->amg->row0();
    if (n_local) *n_local = a->amg->n();
  });
}
int mgb_amg_prepare(mgb_amg a, int level) {
  return guard([&] {
    need(a && level >= -1 && level < a->amg->L(), "level out of range");
    a->amg->prepare(level);
  });
}
int mgb_amg_set_exponents(mgb_amg a, int term, const double* p_nodes) {
  return guard([&] {
    need(a && p_nodes, "set_exponents: null argument");
    a->amg->set_exponents(term, p_nodes);
  });
}
int mgb_amg_set_term_mask(mgb_amg a, const unsigned char* mask) {
  return guard([&] {
    need(a && mask, "set_term_mask: null argument");
    a->amg->set_term_mask(mask);
  });
}
int mgb_amg_set_early_stop(mgb_amg a, int col) {
  return guard([&] {
    need(a && col >= -1, "set_early_stop: bad arguments");
    a->amg->set_early_stop(col);
  });
}
int mgb_amg_f0_f32(mgb_amg a, int level, const float* s, float t, double* f0) {
  return guard([&] {
    need(a && s && f0 && level >= 0 && level < a->amg->L(), "f0_f32: bad arguments");
    *f0 = a->amg->f0_f32(level, s, t);
  });
}
int mgb_amg_f1_f32(mgb_amg a, int level, const float* s, float t, float* g) {
  return guard([&] {
    need(a && s && g && level >= 0 && level < a->amg->L(), "f1_f32: bad arguments");
    a->amg->f1_f32(level, s, t, g);
  });
}
int mgb_amg_f2_f32(mgb_amg a, int level, const float* s, float t, float* lower_vals) {
  return guard([&] {
    need(a && s && lower_vals && level >= 0 && level < a->amg->L(), "f2_f32: bad arguments");
    a->amg->f2_f32(level, s, t, lower_vals);
  });
}
int mgb_amg_f1_template_f64(mgb_amg a, int level, const double* s, double t, double* g) {
  return guard([&] {
    need(a && s && g && level >= 0 && level < a->amg->L(), "f1_template_f64: bad arguments");
    a->amg->f1_tpl64(level, s, t, g);
  });
}
int mgb_amg_f2_template_f64(mgb_amg a, int level, const double* s, double t, double* lower_vals) {
  return guard([&] {
    need(a && s && lower_vals && level >= 0 && level < a->amg->L(), "f2_template_f64: bad arguments");
    a->amg->f2_tpl64(level, s, t, lower_vals);
  });
}
int mgb_amg_trial_set(mgb_amg a, int level, const double* s, const double* nstep, int na, const double* alpha,
                      const double* phi_ref, int mode, double* sums_host, double* sums_dev, double* s_out, double* dz,
                      double* phi) {
  return guard([&] {
    need(a && s && alpha && sums_host && sums_dev && s_out && dz && phi && level >= 0 && level < a->amg->L(),
         "trial_set: bad arguments");
    need(na >= 1 && na <= 3, "trial_set: na must be 1, 2 or 3");
    need(mode >= 0 && mode <= 2, "trial_set: mode must be 0, 1 or 2");
    a->amg->trial_set(level, s, nstep, na, alpha, phi_ref, mode, sums_host, sums_dev, s_out, dz, phi);
  });
}
int mgb_amg_chol_info(mgb_amg a, int level, int* split_world, double* exchange_doubles, int* launches) {
  return guard([&] {
    need(a && level >= 0 && level < a->amg->L(), "level out of range");
    a->amg->chol_info(level, split_world, exchange_doubles, launches);
  });
}
int mgb_amg_chol_premap(mgb_amg a, int level, int cap, int* consumer, int* producers, double* slab_bytes) {
  return guard([&] {
    need(a, "chol_premap: null handle");
    a->amg->chol_premap(level, cap, consumer, producers, slab_bytes);
  });
}
int mgb_amg_chol_schedule(mgb_amg a, int level, int cap, int* nlaunch, int* kind, int* workgroups, int* unknown_node,
                          int* unknown_col) {
  return guard([&] {
    need(a && level >= 0 && level < a->amg->L(), "level out of range");
    a->amg->chol_schedule(level, cap, nlaunch, kind, workgroups, unknown_node, unknown_col);
  });
}
int mgb_amg_chol_tree(mgb_amg a, int level, int cap, int* nnodes, int* ns, int* nf, int* parent) {
  return guard([&] {
    need(a && level >= 0 && level < a->amg->L(), "level out of range");
    a->amg->chol_tree(level, cap, nnodes, ns, nf, parent);
  });
}
int mgb_amg_chol_values_local(mgb_amg a, int level, int* yes) {
  return guard([&] {
    need(a && yes && level >= 0 && level < a->amg->L(), "level out of range");
    *yes = a->amg->chol_values_local(level) ? 1 : 0;
  });
}
int mgb_amg_level_size(mgb_amg a, int level, int* N, int* nnz_lower) {
  return guard([&] {
    need(a && level >= 0 && level < a->amg->L(), "level out of range");
    if (N) *N = a->amg->plan(level).N;
    if (nnz_lower) *nnz_lower = a->amg->plan(level).Apat.nnz();
  });
}
int mgb_amg_hessian_pattern(mgb_amg a, int level, int32_t* rowptr, int32_t* colidx) {
  return guard([&] {
    need(a && level >= 0 && level < a->amg->L(), "level out of range");
    const Csr& A = a->amg->plan(level).Apat;
    if (rowptr) std::copy(A.rowptr.begin(), A.rowptr.end(), rowptr);
    if (colidx) std::copy(A.colidx.begin(), A.colidx.end(), colidx);
  });
}
int mgb_amg_set_c(mgb_amg a, const double* c) {
  return guard([&] {
    need(a && c, "null argument");
    a->amg->set_c(c);
  });
}
int mgb_amg_set_z(mgb_amg a, const double* z) {
  return guard([&] {
    need(a && z, "null argument");
    a->amg->set_z(z);
  });
}
int mgb_amg_get_z(mgb_amg a, double* z) {
  return guard([&] {
    need(a && z, "null argument");
    a->amg->get_z(z);
  });
}
int mgb_amg_get_c(mgb_amg a, double* c) {
  return guard([&] {
    need(a && c, "null argument");
    a->amg->get_c(c);
  });
}

// ---- time loop of parabolic_solve (parabolic.hpp / parabolic.hip)
int mgb_amg_parabolic_begin(mgb_amg a, int nb, const int32_t* bidx) {
  return guard([&] {
    need(a, "parabolic_begin: null amg");
    a->amg->parabolic_begin(nb, bidx);
  });
}
int mgb_amg_parabolic_step(mgb_amg a, double h, double p, mgb_vec f_nodes, mgb_vec gb, double* lift2) {
  return guard([&] {
    need(a && f_nodes, "parabolic_step: null argument");
    need(a->amg->parabolic_nb() >= 0, "parabolic_step: call mgb_amg_parabolic_begin first");
    need(f_nodes->ctx == a->ctx && (!gb || gb->ctx == a->ctx), "parabolic_step: vectors of another context");
    need(f_nodes->n == a->amg->n(), "parabolic_step: f_nodes must hold n values");
    need(!gb || gb->n == a->amg->parabolic_nb(), "parabolic_step: gb must hold one value per boundary node");
    a->amg->parabolic_step(h, p, f_nodes->buf.p, gb ? gb->buf.p : nullptr, lift2);
  });
}
int mgb_amg_parabolic_lifts(mgb_amg a, double* lift2) {
  return guard([&] {
    need(a && lift2, "parabolic_lifts: null argument");
    a->amg->parabolic_lifts(lift2);
  });
}
int mgb_amg_snapshot(mgb_amg a, mgb_vec out) {
  return guard([&] {
    need(a && out, "snapshot: null argument");
    need(out->ctx == a->ctx, "snapshot: vector of another context");
    need(a->ctx->ctx.world == 1, "snapshot: single-GPU contexts only");
    need(out->n == (long long)a->amg->n() * a->amg->S(), "snapshot: out must hold n x S values");
    a->amg->snapshot(out->buf.p);
  });
}

int mgb_amg_apply_D(mgb_amg a, int level, const double* s, double* Dz) {
  return guard([&] {
    need(a && s && Dz && level >= 0 && level < a->amg->L(), "apply_D: bad arguments");
    a->amg->apply_D(level, s, Dz);
  });
}
int mgb_amg_f0(mgb_amg a, int level, const double* s, double t, double* y, double* parts2) {
  return guard([&] {
    need(a && s && y && level >= 0 && level < a->amg->L(), "f0: bad arguments");
    *y = a->amg->f0(level, s, t, parts2);
  });
}
int mgb_amg_f0_trial(mgb_amg a, int level, const double* s_ref, const double* s, double t, double* y) {
  return guard([&] {
    need(a && s_ref && s && y && level >= 0 && level < a->amg->L(), "f0_trial: bad arguments");
    *y = a->amg->f0_trial(level, s_ref, s, t);
  });
}
int mgb_amg_f1(mgb_amg a, int level, const double* s, double t, double* g) {
  return guard([&] {
    need(a && s && g && level >= 0 && level < a->amg->L(), "f1: bad arguments");
    a->amg->f1(level, s, t, g);
  });
}
int mgb_amg_f2(mgb_amg a, int level, const double* s, double t, double* lower_vals) {
  return guard([&] {
    need(a && s && lower_vals && level >= 0 && level < a->amg->L(), "f2: bad arguments");
    a->amg->f2(level, s, t, lower_vals);
  });
}
int mgb_amg_solve_linear(mgb_amg a, int level, const double* lower_vals, const double* g, double* x) {
  return guard([&] {
    need(a && lower_vals && g && x && level >= 0 && level < a->amg->L(), "solve_linear: bad arguments");
    if (!a->amg->solve_host(level, lower_vals, g, x)) throw NumericError("MfChol: matrix is not positive definite");
  });
}
int mgb_amg_solve_linear_gpu(mgb_amg a, int level, const double* lower_vals, const double* g, double* x) {
  return guard([&] {
    need(a && lower_vals && g && x && level >= 0 && level < a->amg->L(), "solve_linear_gpu: bad arguments");
    if (!a->amg->solve_device(level, lower_vals, g, x)) throw NumericError("MfChol: matrix is not positive definite");
  });
}
int mgb_amg_f1_owner(mgb_amg a, int level, const double* s, double t, double* g, double* gg, int32_t* kind) {
  return guard([&] {
    need(a && s && g && level >= 0 && level < a->amg->L(), "f1_owner: bad arguments");
    a->amg->f1_owner(level, s, t, g, gg, kind);
  });
}
int mgb_amg_f2_local(mgb_amg a, int level, const double* s, double t, double* lower_vals) {
  return guard([&] {
    need(a && s && lower_vals && level >= 0 && level < a->amg->L(), "f2_local: bad arguments");
    a->amg->f2_local(level, s, t, lower_vals);
  });
}
int mgb_amg_solve_linear_local(mgb_amg a, int level, const double* local_vals, const double* g, double* x, double* inc, int* flag,
                               double* vals_after) {
  return guard([&] {
    need(a && local_vals && g && x && level >= 0 && level < a->amg->L(), "solve_linear_local: bad arguments");
    a->amg->solve_linear_local(level, local_vals, g, x, inc, flag, vals_after);
  });
}
int mgb_amg_set_solver(mgb_amg a, int solver) {
  return guard([&] {
    need(a && solver >= 0 && solver <= 2, "set_solver: 0 (device Cholesky), 1 (host Cholesky) or 2 (V-cycle-preconditioned CG)");
    a->host_solve = solver == 1;
    a->pcg = solver == 2;
    a->amg->set_pcg(a->pcg);
  });
}
int mgb_amg_set_pcg(mgb_amg a, double rtol, int maxit, int degree, int power_its, double lo_frac, double hi_frac, int chunk,
                    int fallback, int assembled_top, int giveup) {
  return guard([&] {
    need(a, "null amg");
    PcgOptions& o = a->amg->pcg_opt;
    if (rtol > 0) o.rtol = rtol;
    if (maxit > 0) o.maxit = maxit;
    if (degree > 0) {
      need(degree <= kChebMaxDegree, "set_pcg: smoothing degree must be 1..7");
      o.degree = degree;
    }
    if (power_its > 0) o.power_its = power_its;
    if (lo_frac > 0 && hi_frac > lo_frac) {
      o.lo_frac = lo_frac;
      o.hi_frac = hi_frac;
    }
    if (chunk > 0) o.chunk = chunk;
    if (fallback >= 0) o.fallback = fallback != 0;
    if (assembled_top >= 0) o.assembled_top = assembled_top != 0;
    if (giveup >= 0) o.giveup = giveup;
  });
}
int mgb_amg_sol_pcg(mgb_amg a, long long* counts4, double* time_s) {
  return guard([&] {
    need(a, "null amg");
    if (counts4) {
      counts4[0] = a->stats.pcg_solves;
      counts4[1] = a->stats.pcg_iters;
      counts4[2] = a->stats.pcg_fallbacks;
      counts4[3] = a->stats.pcg_gaveup_at;
    }
    if (time_s) *time_s = a->stats.time_pcg;
  });
}
int mgb_hessian_apply(mgb_amg a, int level, const double* s, const double* v, double* Hv, int matrix_free) {
  return guard([&] {
    need(a && s && v && Hv && level >= 0 && level < a->amg->L(), "hessian_apply: bad arguments");
    a->amg->hessian_apply(level, s, v, Hv, matrix_free != 0);
  });
}
int mgb_smooth(mgb_amg a, int level, const double* s, const double* b, double* x, int degree, int sweeps, double lmax,
               int matrix_free, double* lmax_used) {
  return guard([&] {
    need(a && s && b && x && sweeps >= 1 && level >= 0 && level < a->amg->L(), "smooth: bad arguments");
    const double used = a->amg->mg_smooth(level, s, b, x, degree, sweeps, lmax, matrix_free != 0);
    if (lmax_used) *lmax_used = used;
  });
}
int mgb_prolong(mgb_amg a, int level, const double* xc, double* xf) {
  return guard([&] {
    need(a && xc && xf && level >= 0 && level + 1 < a->amg->L(), "prolong: bad arguments");
    a->amg->mg_prolong(level, xc, xf);
  });
}
int mgb_restrict(mgb_amg a, int level, const double* rf, double* rc) {
  return guard([&] {
    need(a && rf && rc && level >= 0 && level + 1 < a->amg->L(), "restrict: bad arguments");
    a->amg->mg_restrict(level, rf, rc);
  });
}
int mgb_amg_prolongation(mgb_amg a, int level, int* rows, int* cols, int* nnz, int32_t* rowptr, int32_t* colidx, double* vals) {
  return guard([&] {
    need(a && level >= 0 && level + 1 < a->amg->L(), "prolongation: bad arguments");
    const Csr& P = a->amg->prolongation_host(level);
    if (rows) *rows = P.rows;
    if (cols) *cols = P.cols;
    if (nnz) *nnz = P.nnz();
    if (rowptr) std::copy(P.rowptr.begin(), P.rowptr.end(), rowptr);
    if (colidx) std::copy(P.colidx.begin(), P.colidx.end(), colidx);
    if (vals) std::copy(P.vals.begin(), P.vals.end(), vals);
  });
}
int mgb_amg_pcg_solve_linear(mgb_amg a, int level, const double* s, const double* g, double* x, int* iters, double* relres,
                             int* converged) {
  return guard([&] {
    need(a && s && g && x && level >= 0 && level < a->amg->L(), "pcg_solve_linear: bad arguments");
    const bool ok = a->amg->pcg_solve_linear(level, s, g, x, iters, relres);
    if (converged) *converged = ok ? 1 : 0;
  });
}
int mgb_amg_mg_pin_lmax(mgb_amg a, int level, double lmax) {
  return guard([&] {
    need(a && level >= 0 && level < a->amg->L(), "mg_pin_lmax: bad arguments");
    a->amg->mg_pin_lmax(level, lmax);
  });
}
int mgb_amg_vcycle(mgb_amg a, int top, const double* s, const double* b, double* x, double* lmax_used) {
  return guard([&] {
    need(a && s && b && x && lmax_used && top >= 0 && top < a->amg->L(), "vcycle: bad arguments");
    a->amg->vcycle(top, s, b, x, lmax_used);
  });
}
int mgb_amg_time_mg_kernels(mgb_amg a, int level, int reps, int nrot, double* ms6, double* bytes6, double* alg6) {
  return guard([&] {
    need(a && ms6 && bytes6 && alg6 && reps > 0 && nrot >= 1 && nrot <= 64 && level >= 0 && level < a->amg->L(),
         "time_mg_kernels: bad arguments");
    Amg::MgKernelTimes k = a->amg->time_mg_kernels(level, reps, nrot);
    std::copy(k.ms, k.ms + 6, ms6);
    std::copy(k.bytes, k.bytes + 6, bytes6);
    std::copy(k.alg, k.alg + 6, alg6);
  });
}
int mgb_amg_mg_info(mgb_amg a, int top, int* coarsest) {
  return guard([&] {
    need(a && top >= 0 && top < a->amg->L(), "mg_info: bad arguments");
    if (coarsest) *coarsest = a->amg->mg_coarsest(top);
  });
}
int mgb_amg_elop_info(mgb_amg a, int level, int* out) {
  return guard([&] {
    need(a && out && level >= 0 && level < a->amg->L(), "elop_info: bad arguments");
    a->amg->elop_info(level, out);
  });
}
int mgb_amg_set_stop_rule(mgb_amg a, int upstream) {
  return guard([&] {
    need(a, "null amg");
    a->upstream_stop = upstream != 0;
  });
}
int mgb_amg_set_centering(mgb_amg a, int exact) {
  return guard([&] {
    need(a, "null amg");
    a->exact_centering = exact != 0;
  });
}
int mgb_amg_set_schedule(mgb_amg a, int all_levels) {
  return guard([&] {
    need(a, "null amg");
    a->schedule_all = all_levels != 0;
  });
}
int mgb_amg_solve(mgb_amg a, double tol, double t0, double kappa, int maxit, int max_newton, int verbose) {
  return guard([&] {
    need(a, "null amg");
    SolveOptions o;
    o.schedule_all = a->schedule_all;
    o.host_solve = a->host_solve;
    o.pcg = a->pcg;
    o.upstream_stop = a->upstream_stop;
    o.exact_centering = a->exact_centering;
    o.time_kernels = a->time_kernels;
    if (tol > 0) o.tol = tol;
    if (t0 > 0) o.t0 = t0;
    if (kappa > 1) o.kappa = kappa;
    if (maxit > 0) o.maxit = maxit;
    if (max_newton > 0) o.max_newton = max_newton;
    o.verbose = verbose;
    const double ts = a->stats.t_setup;
    a->amg->solve(o, a->stats);
    a->stats.t_setup = ts;
  });
}
int mgb_amg_set_time_kernels(mgb_amg a, int on) {
  return guard([&] {
    need(a, "null amg");
    a->time_kernels = on != 0;
  });
}
int mgb_amg_set_trace(mgb_amg a, int max_steps, int keep_vectors) {
  return guard([&] {
    need(a && max_steps >= 0, "set_trace: bad arguments");
    a->amg->set_trace(max_steps, keep_vectors != 0);
  });
}
int mgb_amg_trace_info(mgb_amg a, int* ncentering, int* nsteps, long long* nvec) {
  return guard([&] {
    need(a, "null amg");
    const NewtonTrace& t = a->amg->trace();
    if (ncentering) *ncentering = t.ncenterings();
    if (nsteps) *nsteps = t.nsteps();
    if (nvec) *nvec = (long long)t.vectors.size();
  });
}
int mgb_amg_trace_get(mgb_amg a, double* centerings, double* steps, double* vectors) {
  return guard([&] {
    need(a, "null amg");
    const NewtonTrace& t = a->amg->trace();
    if (centerings) std::copy(t.centerings.begin(), t.centerings.end(), centerings);
    if (steps) std::copy(t.steps.begin(), t.steps.end(), steps);
    if (vectors) std::copy(t.vectors.begin(), t.vectors.end(), vectors);
  });
}
int mgb_amg_sol_info(mgb_amg a, int* nt, double* t_elapsed, double* time_factor, long long* counts4) {
  return guard([&] {
    need(a, "null amg");
    if (nt) *nt = (int)a->stats.ts.size();
    if (t_elapsed) *t_elapsed = a->stats.t_elapsed;
    if (time_factor) *time_factor = a->stats.time_factor;
    if (counts4) {
      counts4[0] = a->stats.n_f0;
      counts4[1] = a->stats.n_f1;
      counts4[2] = a->stats.n_f2;
      counts4[3] = a->stats.n_factor;
    }
  });
}
int mgb_amg_sol_get(mgb_amg a, long long* its, double* ts, double* c_dot_Dz) {
  return guard([&] {
    need(a, "null amg");
    if (its) std::copy(a->stats.its.begin(), a->stats.its.end(), its);
    if (ts) std::copy(a->stats.ts.begin(), a->stats.ts.end(), ts);
    if (c_dot_Dz) std::copy(a->stats.c_dot_Dz.begin(), a->stats.c_dot_Dz.end(), c_dot_Dz);
  });
}
int mgb_amg_sol_kernels(mgb_amg a, double* ms11, double* bytes11, long long* launches11) {
  return guard([&] {
    need(a, "null amg");
    for (int i = 0; i < KC_COUNT; ++i) {
      if (ms11) ms11[i] = a->stats.kern_ms[i];
      if (bytes11) bytes11[i] = a->stats.kern_bytes[i];
      if (launches11) launches11[i] = a->stats.kern_launches[i];
    }
  });
}
int mgb_amg_time_kernels(mgb_amg a, int level, int reps, int nrot, double* ms8, double* bytes8) {
  return guard([&] {
    need(a && ms8 && bytes8 && reps > 0 && nrot >= 1 && nrot <= 64 && level >= 0 && level < a->amg->L(), "time_kernels: bad arguments");
    Amg::KernelTimes k = a->amg->time_kernels(level, reps, nrot);
    const double ms[8] = {k.apply_ms, k.f2_ms, k.assemble_ms, k.f1_ms, k.restrict_ms, k.f0_ms, k.trial_ms, k.apply_csr_ms};
    const double by[8] = {k.apply_bytes, k.f2_bytes, k.assemble_bytes, k.f1_bytes, k.restrict_bytes, k.f0_bytes, k.trial_bytes,
                          k.apply_el};      // last slot: 1 if apply_D (slot 0) ran through the element-local view
    std::copy(ms, ms + 8, ms8);
    std::copy(by, by + 8, bytes8);
  });
}

// ---- evaluation at arbitrary points (interp.hpp / interp.hip)
int mgb_locator_create(mgb_ctx ctx, mgb_geo g, mgb_locator* out) {
  return guard([&] {
    need(ctx && g && out, "locator_create: null argument");
    interp::Locator loc = interp::build_locator(g->g);
    hip_check(hipSetDevice(ctx->ctx.device), "hipSetDevice");
    need(g->g.w.size() == (size_t)g->g.n, "locator_create: the geometry must carry one weight per node");
    auto* l = new mgb_locator_s{ctx, std::move(loc), {}, {}, {}, {}, {}, {}};
    try {
      l->cellptr.upload(l->loc.cellptr.data(), l->loc.cellptr.size());
      l->cellelem.upload(l->loc.cellelem.data(), l->loc.cellelem.size());
      l->x.upload(g->g.x.data(), g->g.x.size());
      l->w.upload(g->g.w.data(), g->g.w.size());
    } catch (...) {
      delete l;
      throw;
    }
    *out = l;
  });
}
int mgb_locator_destroy(mgb_locator loc) {
  return guard([&] { delete loc; });
}
int mgb_interpolate(mgb_locator loc, int m, mgb_vec pts, int S, mgb_vec z, mgb_vec vals, mgb_vec grads, int32_t* elem_host) {
  return guard([&] {
    need(loc && pts && z && vals, "interpolate: null argument");
    need(m >= 0 && S >= 1, "interpolate: m must be >= 0 and S >= 1");
    const interp::Locator& L = loc->loc;
    need(pts->n == (long long)m * L.dim, "interpolate: pts must hold m x dim values");
    need(z->n == (long long)L.n * S, "interpolate: z must hold n x S values");
    need(vals->n == (long long)m * S, "interpolate: vals must hold m x S values");
    need(!grads || grads->n == (long long)m * S * L.dim, "interpolate: grads must hold m x S x dim values");
    need(pts->ctx == loc->ctx && z->ctx == loc->ctx && vals->ctx == loc->ctx && (!grads || grads->ctx == loc->ctx),
         "interpolate: vectors of another context");
    if (m == 0) return;
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    DevBuf<int> elem;
    if (elem_host) elem.alloc(m);
    interp::launch_interpolate(st, L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p), L.dim, L.k, m, pts->buf.p, S, z->buf.p,
                               vals->buf.p, grads ? grads->buf.p : nullptr, elem.p);
    hip_check(hipGetLastError(), "interpolate launch");
    if (elem_host) {
      hip_check(hipStreamSynchronize(st), "sync interpolate");
      elem.download(elem_host, m);
    }
  });
}
int mgb_geo_interpolate_host(mgb_geo g, int m, const double* pts, int S, const double* z, double* vals, double* grads,
                             int32_t* elem) {
  return guard([&] {
    need(g && m >= 0 && S >= 1, "geo_interpolate_host: null geometry, m < 0 or S < 1");
    need(m == 0 || (pts && z && vals), "geo_interpolate_host: null array");
    const interp::Locator loc = interp::build_locator(g->g);
    interp::interpolate_host(loc, g->g.x.data(), m, pts, S, z, vals, grads, elem);
  });
}

// ---- norms and errors by the nodal quadrature rule (norms.hpp / norms.hip)
namespace {
bool good_q(double q) { return q >= 1.0 && (q - q) == 0.0; }
}  // namespace
int mgb_field_norms(mgb_locator loc, int S, mgb_vec z, double q, mgb_vec ref_vals, mgb_vec ref_grads, mgb_locator other,
                    mgb_vec z_other, double* out_host, long long* outside_host) {
  return guard([&] {
    need(loc && z && out_host, "field_norms: null argument");
    need(S >= 1, "field_norms: S must be >= 1");
    need(good_q(q), "field_norms: q must be finite and >= 1");
    const interp::Locator& L = loc->loc;
    need(z->n == (long long)L.n * S, "field_norms: z must hold n x S values");
    need(!ref_grads || ref_vals, "field_norms: ref_grads without ref_vals");
    need(!(ref_vals && other), "field_norms: both ref_vals and another mesh");
    need((other != nullptr) == (z_other != nullptr), "field_norms: other and z_other come together");
    need(!ref_vals || ref_vals->n == (long long)L.n * S, "field_norms: ref_vals must hold n x S values");
    need(!ref_grads || ref_grads->n == (long long)L.n * S * L.dim, "field_norms: ref_grads must hold n x S x dim values");
    need(z->ctx == loc->ctx && (!ref_vals || ref_vals->ctx == loc->ctx) && (!ref_grads || ref_grads->ctx == loc->ctx),
         "field_norms: vectors of another context");
    if (other) {
      need(other->ctx == loc->ctx && z_other->ctx == loc->ctx, "field_norms: the other mesh belongs to another context");
      need(other->loc.dim == L.dim, "field_norms: the other mesh has another dimension");
      need(other->loc.k == L.k, "field_norms: the other mesh has elements of another degree");
      need(z_other->n == (long long)other->loc.n * S, "field_norms: z_other must hold n_other x S values");
    }
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nd = norms::scratch_doubles(L.n, S), nc = norms::scratch_counts(L.n);
    if (loc->norm_scratch.n < nd) loc->norm_scratch.alloc(nd);
    if (loc->norm_counts.n < nc) loc->norm_counts.alloc(nc);
    norms::Args A;
    A.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.w = loc->w.p;
    A.z = z->buf.p;
    A.ref_vals = ref_vals ? ref_vals->buf.p : nullptr;
    A.ref_grads = ref_grads ? ref_grads->buf.p : nullptr;
    if (other) {
      A.other = other->loc.view(other->cellptr.p, other->cellelem.p, other->x.p);
      A.z_other = z_other->buf.p;
      A.cross = true;
    }
    A.n = L.n;
    A.S = S;
    A.q = q;
    norms::launch_field_norms(st, L.dim, L.k, A, loc->norm_scratch.p, loc->norm_counts.p);
    hip_check(hipGetLastError(), "field_norms launch");
    hip_check(hipStreamSynchronize(st), "sync field_norms");
    hip_check(hipMemcpy(out_host, loc->norm_scratch.p + norms::results_offset(L.n, S), (size_t)S * reduce::kCols * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
    if (outside_host)
      hip_check(hipMemcpy(outside_host, loc->norm_counts.p + norms::count_offset(L.n), sizeof(long long), hipMemcpyDeviceToHost), "D2H");
  });
}
int mgb_geo_field_norms_host(mgb_geo g, int S, const double* z, double q, const double* ref_vals, const double* ref_grads,
                             mgb_geo other, const double* z_other, double* out, long long* outside) {
  return guard([&] {
    need(g && z && out, "geo_field_norms_host: null argument");
    need(S >= 1, "geo_field_norms_host: S must be >= 1");
    need(good_q(q), "geo_field_norms_host: q must be finite and >= 1");
    need(!ref_grads || ref_vals, "geo_field_norms_host: ref_grads without ref_vals");
    need(!(ref_vals && other), "geo_field_norms_host: both ref_vals and another mesh");
    need((other != nullptr) == (z_other != nullptr), "geo_field_norms_host: other and z_other come together");
    need(g->g.w.size() == (size_t)g->g.n, "geo_field_norms_host: the geometry must carry one weight per node");
    const interp::Locator L = interp::build_locator(g->g);
    interp::Locator Lo;
    if (other && other != g) Lo = interp::build_locator(other->g);
    const interp::Locator& O = other && other != g ? Lo : L;
    norms::Args A;
    A.own = L.view(L.cellptr.data(), L.cellelem.data(), g->g.x.data());
    A.w = g->g.w.data();
    A.z = z;
    A.ref_vals = ref_vals;
    A.ref_grads = ref_grads;
    if (other) {
      need(O.dim == L.dim, "geo_field_norms_host: the other mesh has another dimension");
      need(O.k == L.k, "geo_field_norms_host: the other mesh has elements of another degree");
      A.other = O.view(O.cellptr.data(), O.cellelem.data(), other->g.x.data());
      A.z_other = z_other;
      A.cross = true;
    }
    A.n = L.n;
    A.S = S;
    A.q = q;
    norms::field_norms_host(L.dim, L.k, A, out, outside);
  });
}

// ---- energy, flux and cone margin of p-Laplace solutions (energy.hpp / energy.hip)
namespace {
// what the entry points of energy, boundary flux and estimate check alike: B fields of S columns, column u, exponent p
void need_field_shape(const std::string& w, int B, int S, int u, double p) {
  if (B < 1) throw std::invalid_argument(w + ": B must be >= 1");
  if (S < 1) throw std::invalid_argument(w + ": S must be >= 1");
  if (!good_q(p)) throw std::invalid_argument(w + ": p must be finite and >= 1");
  if (u < 0 || u >= S) throw std::invalid_argument(w + ": column u outside [0, S)");
}
// checks every z[b] and collects the table of the B fields of n x S values on the context of `loc`
void field_table(const std::string& w, const mgb_locator_s* loc, int B, const mgb_vec* z, int S, std::vector<const double*>& table) {
  table.resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    if (z[b] == nullptr) throw std::invalid_argument(w + ": null field");
    if (z[b]->n != (long long)loc->loc.n * S) throw std::invalid_argument(w + ": every z must hold n x S values");
    if (z[b]->ctx != loc->ctx) throw std::invalid_argument(w + ": vectors of another context");
    table[b] = z[b]->buf.p;
  }
}
// the slack column and the forcing on top; s < 0: no slack column (flux)
void need_energy_shape(const char* who, int B, int S, int u, int s, double p, int f_rows, bool has_f) {
  const std::string w(who);
  need_field_shape(w, B, S, u, p);
  if (s >= S) throw std::invalid_argument(w + ": column s outside [0, S)");
  if (u == s) throw std::invalid_argument(w + ": u and s are the same column");
  if (has_f && f_rows != 1 && f_rows != B) throw std::invalid_argument(w + ": f must have 1 or B rows");
}
}  // namespace
int mgb_geo_field_energy(mgb_locator loc, int B, const mgb_vec* z, int S, int u, int s, double p, mgb_vec p_nodal, mgb_vec f,
                         int f_rows, double* out_host) {
  return guard([&] {
    need(loc && z && out_host, "geo_field_energy: null argument");
    need_energy_shape("geo_field_energy", B, S, u, s, p, f_rows, f != nullptr);
    need(s >= 0, "geo_field_energy: column s outside [0, S)");
    need(loc->ctx->ctx.world == 1, "geo_field_energy: sharded contexts are not supported");
    const interp::Locator& L = loc->loc;
    std::vector<const double*> table;
    field_table("geo_field_energy", loc, B, z, S, table);
    need(!p_nodal || p_nodal->n == L.n, "geo_field_energy: p_nodal must hold n values");
    need(!f || f->n == (long long)f_rows * L.n, "geo_field_energy: f must hold f_rows x n values");
    need((!p_nodal || p_nodal->ctx == loc->ctx) && (!f || f->ctx == loc->ctx), "geo_field_energy: vectors of another context");
    need(B <= 65535, "geo_field_energy: at most 65535 fields per call");
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nd = energy::scratch_doubles(L.n, B);
    if (loc->energy_scratch.n < nd) loc->energy_scratch.alloc(nd);
    loc->energy_table.upload(table.data(), table.size());      // every earlier launch that read it has been waited for
    energy::Args A;
    A.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.w = loc->w.p;
    A.p_nodal = p_nodal ? p_nodal->buf.p : nullptr;
    A.p = p;
    A.z = loc->energy_table.p;
    A.f = f ? f->buf.p : nullptr;
    A.f_stride = f && f_rows == B && B > 1 ? L.n : 0;
    A.n = L.n, A.S = S, A.u = u, A.s = s, A.B = B;
    energy::launch_field_energy(st, L.dim, L.k, A, loc->energy_scratch.p);
    hip_check(hipGetLastError(), "geo_field_energy launch");
    hip_check(hipStreamSynchronize(st), "sync geo_field_energy");
    hip_check(hipMemcpy(out_host, loc->energy_scratch.p + energy::results_offset(L.n, B), (size_t)B * reduce::kCols * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
  });
}
int mgb_geo_field_energy_host(mgb_geo g, int B, const double* const* z, int S, int u, int s, double p, const double* p_nodal,
                              const double* f, int f_rows, double* out, double* flux) {
  return guard([&] {
    need(g && z && out, "geo_field_energy_host: null argument");
    need_energy_shape("geo_field_energy_host", B, S, u, s, p, f_rows, f != nullptr);
    need(s >= 0, "geo_field_energy_host: column s outside [0, S)");
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_field_energy_host: null field");
    need(g->g.w.size() == (size_t)g->g.n, "geo_field_energy_host: the geometry must carry one weight per node");
    if (p_nodal)
      for (int i = 0; i < g->g.n; ++i) need(good_q(p_nodal[i]), "geo_field_energy_host: every p_nodal must be finite and >= 1");
    const interp::Locator L = interp::build_locator(g->g);
    energy::Args A;
    A.own = L.view(L.cellptr.data(), L.cellelem.data(), g->g.x.data());
    A.w = g->g.w.data();
    A.p_nodal = p_nodal;
    A.p = p;
    A.z = z;
    A.f = f;
    A.f_stride = f && f_rows == B && B > 1 ? L.n : 0;
    A.n = L.n, A.S = S, A.u = u, A.s = s, A.B = B;
    energy::field_energy_host(L.dim, L.k, A, out, flux);
  });
}
int mgb_geo_field_flux(mgb_locator loc, mgb_vec z, int S, int u, double p, mgb_vec p_nodal, mgb_vec flux) {
  return guard([&] {
    need(loc && z && flux, "geo_field_flux: null argument");
    need_energy_shape("geo_field_flux", 1, S, u, -1, p, 1, false);
    need(loc->ctx->ctx.world == 1, "geo_field_flux: sharded contexts are not supported");
    const interp::Locator& L = loc->loc;
    need(z->n == (long long)L.n * S, "geo_field_flux: z must hold n x S values");
    need(flux->n == (long long)L.n * L.dim, "geo_field_flux: flux must hold n x dim values");
    need(!p_nodal || p_nodal->n == L.n, "geo_field_flux: p_nodal must hold n values");
    need(z->ctx == loc->ctx && flux->ctx == loc->ctx && (!p_nodal || p_nodal->ctx == loc->ctx),
         "geo_field_flux: vectors of another context");
    need(z != flux, "geo_field_flux: flux must not be z");
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    energy::Args A;
    A.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.w = loc->w.p;
    A.p_nodal = p_nodal ? p_nodal->buf.p : nullptr;
    A.p = p;
    A.n = L.n, A.S = S, A.u = u, A.B = 1;
    energy::launch_field_flux(loc->ctx->ctx.stream, L.dim, L.k, A, z->buf.p, flux->buf.p);
    hip_check(hipGetLastError(), "geo_field_flux launch");
  });
}

// ---- level sets of nodal fields (levelset.hpp / levelset.hip)
namespace {
void need_levels(const char* who, int B, int S, int u, int nl, const double* levels, int dim, int refine) {
  const std::string w(who);
  if (B < 1) throw std::invalid_argument(w + ": B must be >= 1");
  if (nl < 1) throw std::invalid_argument(w + ": nl must be >= 1");
  if (S < 1) throw std::invalid_argument(w + ": S must be >= 1");
  if (u < 0 || u >= S) throw std::invalid_argument(w + ": column u outside [0, S)");
  if (dim == 3) throw std::invalid_argument(w + ": isosurfaces of 3-D fields are not covered");
  if (refine < 0 || refine > (dim == 2 ? levelset::kMaxRefine : 0))
    throw std::invalid_argument(w + (dim == 2 ? ": refine must be 0, 1, 2 or 3" : ": refine must be 0 in 1-D"));
  for (int l = 0; l < nl; ++l)
    if (!interp::finite(levels[l])) throw std::invalid_argument(w + ": every level must be finite");
}
}  // namespace
int mgb_geo_level_sets(mgb_locator loc, int B, const mgb_vec* z, int S, int u, int nl, const double* levels_host, int refine,
                       double* out_host, long long* counts_host, mgb_levelset* segs) {
  return guard([&] {
    need(loc && z && levels_host && out_host && counts_host, "geo_level_sets: null argument");
    const interp::Locator& L = loc->loc;
    need(B <= 65535 && nl <= 65535, "geo_level_sets: at most 65535 fields and 65535 levels per call");      // before any is read
    need_levels("geo_level_sets", B, S, u, nl, levels_host, L.dim, refine);
    need(loc->ctx->ctx.world == 1, "geo_level_sets: sharded contexts are not supported");
    std::vector<const double*> table;
    field_table("geo_level_sets", loc, B, z, S, table);
    levelset::Args A;
    A.items = levelset::items_per_row(L.dim, L.nel, refine);
    need(A.items <= INT_MAX, "geo_level_sets: more than INT_MAX items per row");
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t rows = (size_t)B * nl, nwg = (size_t)reduce::workgroups(A.items);
    const size_t nd = levelset::scratch_words(rows, nwg), nc = levelset::count_words(rows, nwg);
    if (loc->ls_scratch.n < nd) loc->ls_scratch.alloc(nd);
    if (loc->ls_counts.n < nc) loc->ls_counts.alloc(nc);
    loc->ls_table.upload(table.data(), table.size());      // every earlier launch that read these has been waited for
    loc->ls_levels.upload(levels_host, (size_t)nl);
    A.x = loc->x.p;
    A.z = loc->ls_table.p;
    A.levels = loc->ls_levels.p;
    A.nel = L.nel, A.S = S, A.u = u, A.B = B, A.nl = nl, A.refine = refine;
    levelset::launch_measure(st, L.dim, A, loc->ls_scratch.p, loc->ls_counts.p);
    hip_check(hipGetLastError(), "geo_level_sets launch");
    hip_check(hipStreamSynchronize(st), "sync geo_level_sets");
    // the rows and the totals lie behind each other: one copy
    std::vector<double> both(rows * (reduce::kCols + 1));
    hip_check(hipMemcpy(both.data(), loc->ls_scratch.p + levelset::results_offset(rows, nwg), both.size() * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
    std::copy(both.begin(), both.begin() + rows * reduce::kCols, out_host);
    std::memcpy(counts_host, both.data() + rows * reduce::kCols, rows * sizeof(long long));
    if (!segs) return;
    std::unique_ptr<mgb_levelset_s> out(new mgb_levelset_s{loc->ctx, levelset::seg_width(L.dim), {}, {}, {}});
    out->row_offsets.resize(rows + 1);
    out->row_offsets[0] = 0;
    for (size_t r = 0; r < rows; ++r) out->row_offsets[r + 1] = out->row_offsets[r] + counts_host[r];
    const long long total = out->row_offsets[rows];
    if (total > 0) {
      out->seg.alloc((size_t)total * out->width);
      out->item.alloc((size_t)total);
      loc->ls_row_base.upload(out->row_offsets.data(), rows);
      levelset::launch_emit(st, L.dim, A, loc->ls_counts.p + levelset::offsets_offset(rows, nwg), loc->ls_row_base.p, total,
                            out->seg.p, out->item.p);
      hip_check(hipGetLastError(), "geo_level_sets emit launch");
      hip_check(hipStreamSynchronize(st), "sync geo_level_sets emit");
    }
    *segs = out.release();
  });
}
int mgb_levelset_get(mgb_levelset segs, long long* row_offsets, double* seg, int32_t* item) {
  return guard([&] {
    need(segs != nullptr, "levelset_get: null argument");
    hip_check(hipSetDevice(segs->ctx->ctx.device), "hipSetDevice");
    if (row_offsets) std::copy(segs->row_offsets.begin(), segs->row_offsets.end(), row_offsets);
    if (seg) segs->seg.download(seg, segs->seg.n);
    if (item) segs->item.download(item, segs->item.n);
  });
}
int mgb_levelset_destroy(mgb_levelset segs) {
  return guard([&] { delete segs; });
}
int mgb_geo_level_sets_host(mgb_geo g, int B, const double* const* z, int S, int u, int nl, const double* levels, int refine,
                            double* out, long long* counts, long long* row_offsets, double* seg, int32_t* item, long long capacity) {
  return guard([&] {
    need(g && z && levels && out && counts, "geo_level_sets_host: null argument");
    need_levels("geo_level_sets_host", B, S, u, nl, levels, g->g.dim, refine);
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_level_sets_host: null field");
    need((seg == nullptr) == (item == nullptr), "geo_level_sets_host: seg and item come together");
    need(!seg || capacity >= 0, "geo_level_sets_host: negative capacity");
    const interp::Locator L = interp::build_locator(g->g);
    levelset::Args A;
    A.items = levelset::items_per_row(L.dim, L.nel, refine);
    need(A.items <= INT_MAX, "geo_level_sets_host: more than INT_MAX items per row");
    A.x = g->g.x.data();
    A.z = z;
    A.levels = levels;
    A.nel = L.nel, A.S = S, A.u = u, A.B = B, A.nl = nl, A.refine = refine;
    levelset::level_sets_host(L.dim, A, out, counts, row_offsets, seg, item, capacity);
  });
}

// ---- time statistics of a run of snapshots (timestat.hpp / timestat.hip)
namespace {
// what both entry points check alike (timestat::check), and the steps h_m = ts[m+1] - ts[m] both sides are handed
std::vector<double> time_steps(const char* who, bool null_argument, int B, const double* ts, int S, int u, int nl, const double* levels) {
  timestat::Call c;
  c.null_argument = null_argument;
  c.B = B, c.S = S, c.u = u, c.nl = nl, c.ts = ts, c.levels = levels;
  timestat::check(who, c);
  std::vector<double> h((size_t)B - 1);
  for (int m = 0; m + 1 < B; ++m) h[m] = ts[m + 1] - ts[m];
  return h;
}
}  // namespace
int mgb_geo_time_stats(mgb_locator loc, int B, const mgb_vec* z, const double* ts_host, int S, int u, int nl,
                       const double* levels_host, double never, mgb_vec node, mgb_vec level, double* out_host) {
  return guard([&] {
    const bool null_argument = !(loc && z && ts_host && node && out_host) || (nl > 0 && !(levels_host && level));
    const std::vector<double> h = time_steps("geo_time_stats", null_argument, B, ts_host, S, u, nl, levels_host);
    need(loc->ctx->ctx.world == 1, "geo_time_stats: sharded contexts are not supported");
    const interp::Locator& L = loc->loc;
    std::vector<const double*> table;
    field_table("geo_time_stats", loc, B, z, S, table);
    need(node->n == (long long)L.n * timestat::kNodeCols, "geo_time_stats: node must hold n x 8 values");
    need(nl == 0 || level->n == (long long)nl * L.n * timestat::kLevelCols, "geo_time_stats: level must hold nl x n x 5 values");
    need(node->ctx == loc->ctx && (nl == 0 || level->ctx == loc->ctx), "geo_time_stats: vectors of another context");
    need(nl == 0 || node != level, "geo_time_stats: node and level are the same vector");
    for (int b = 0; b < B; ++b) need(z[b] != node && (nl == 0 || z[b] != level), "geo_time_stats: an output is also an input");
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nwg = (size_t)reduce::workgroups(L.n), rows = 1 + (size_t)nl;
    const size_t nd = timestat::scratch_doubles((size_t)nl, nwg);
    if (loc->tst_scratch.n < nd) loc->tst_scratch.alloc(nd);
    // the uniform data of the call in ONE copy: B pointers | B - 1 steps | B times | nl levels, 8 bytes each
    std::vector<uint64_t> uni((size_t)B + h.size() + (size_t)B + (size_t)nl);
    static_assert(sizeof(const double*) == 8 && sizeof(double) == 8, "8-byte words");
    std::memcpy(uni.data(), table.data(), (size_t)B * 8);
    std::memcpy(uni.data() + B, h.data(), h.size() * 8);
    std::memcpy(uni.data() + B + h.size(), ts_host, (size_t)B * 8);
    if (nl) std::memcpy(uni.data() + B + h.size() + B, levels_host, (size_t)nl * 8);
    loc->tst_uniform.upload(uni.data(), uni.size());      // every earlier launch that read it has been waited for
    timestat::Args A;
    A.z = reinterpret_cast<const double* const*>(loc->tst_uniform.p);
    A.h = reinterpret_cast<const double*>(loc->tst_uniform.p + B);
    A.ts = A.h + h.size();
    A.levels = A.ts + B;
    A.w = loc->w.p;
    A.node = node->buf.p;
    A.level = nl ? level->buf.p : nullptr;
    A.never = never;
    A.n = L.n, A.S = S, A.u = u, A.B = B, A.nl = nl;
    timestat::launch_time_stats(st, A, loc->tst_scratch.p);
    hip_check(hipGetLastError(), "geo_time_stats launch");
    hip_check(hipStreamSynchronize(st), "sync geo_time_stats");
    hip_check(hipMemcpy(out_host, loc->tst_scratch.p + timestat::results_offset((size_t)nl, nwg), rows * reduce::kCols * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
  });
}
int mgb_geo_time_stats_host(mgb_geo g, int B, const double* const* z, const double* ts, int S, int u, int nl, const double* levels,
                            double never, double* node, double* level, double* out) {
  return guard([&] {
    const bool null_argument = !(g && z && ts && node && out) || (nl > 0 && !(levels && level));
    const std::vector<double> h = time_steps("geo_time_stats_host", null_argument, B, ts, S, u, nl, levels);
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_time_stats_host: null field");
    need(g->g.w.size() == (size_t)g->g.n, "geo_time_stats_host: the geometry must carry one weight per node");
    need(nl == 0 || node != level, "geo_time_stats_host: node and level are the same array");
    need(node != out && (nl == 0 || level != out), "geo_time_stats_host: out is also a table");
    for (int b = 0; b < B; ++b)
      need(z[b] != node && z[b] != out && (nl == 0 || z[b] != level), "geo_time_stats_host: an output is also an input");
    timestat::Args A;
    A.z = z, A.h = h.data(), A.ts = ts, A.levels = levels, A.w = g->g.w.data();
    A.node = node, A.level = nl ? level : nullptr, A.never = never;
    A.n = g->g.n, A.S = S, A.u = u, A.B = B, A.nl = nl;
    timestat::time_stats_host(A, out);
  });
}

// ---- flow lines of nodal fields (flowline.hpp / flowline.hip)
namespace {
// the arguments both entry points take alike, checked by flowline::check before anything is launched or written
void flow_args(flowline::Args& A, const char* who, int dim, int B, int S, int u, int m, double p, int direction,
               const double* ds_or_null, double min_extent, int max_steps, double gmin, bool paths) {
  if (dim == 1) throw std::invalid_argument(std::string(who) + ": flow lines need a 2-D or 3-D geometry");
  A.p = p, A.gmin = gmin;
  A.ds = ds_or_null ? *ds_or_null : 0.25 * min_extent;
  A.sgn = direction == 1 ? 1.0 : direction == -1 ? -1.0 : 0.0;
  A.m = m, A.S = S, A.u = u, A.B = B, A.max_steps = max_steps;
  A.stride = (long long)max_steps + 2;
  flowline::check(A, dim, paths);
}
}  // namespace
int mgb_geo_flow_lines(mgb_locator loc, int B, const mgb_vec* z, int S, int u, int m, const double* seeds_host, double p,
                       int direction, const double* ds_or_null, int max_steps, double gmin, int workgroup, double* rows_host,
                       double* end_host, int32_t* status_host, int32_t* count_host, int32_t* end_element_host, double* ds_used,
                       mgb_flowpath* paths) {
  return guard([&] {
    need(loc && z, "geo_flow_lines: null argument");
    const interp::Locator& L = loc->loc;
    flowline::Args A{};
    flow_args(A, "geo_flow_lines", L.dim, B, S, u, m, p, direction, ds_or_null, L.min_extent, max_steps, gmin,
              paths != nullptr);
    need(workgroup == 0 || workgroup == 64 || workgroup == 128 || workgroup == 256,
         "geo_flow_lines: the workgroup size is 0 (default), 64, 128 or 256");
    need(loc->ctx->ctx.world == 1, "geo_flow_lines: sharded contexts are not supported");
    std::vector<const double*> table;
    field_table("geo_flow_lines", loc, B, z, S, table);
    need(m == 0 || (seeds_host && rows_host && end_host && status_host && count_host && end_element_host),
         "geo_flow_lines: null array");
    if (ds_used) *ds_used = A.ds;
    const int dim = L.dim;
    const size_t rows = (size_t)B * m;
    std::unique_ptr<mgb_flowpath_s> out;
    if (paths) {
      out.reset(new mgb_flowpath_s{loc->ctx, dim, {}, {}, {}});
      out->offsets.assign(rows + 1, 0);
    }
    if (m == 0) {
      if (paths) *paths = out.release();
      return;
    }
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nout = rows * (flowline::kRowCols + dim);
    if (loc->fl_out.n < nout) loc->fl_out.alloc(nout);
    if (loc->fl_int.n < 3 * rows) loc->fl_int.alloc(3 * rows);
    if (paths) {
      const size_t slots = rows * (size_t)A.stride;
      if (loc->fl_pts.n < slots * dim) loc->fl_pts.alloc(slots * dim);
      if (loc->fl_pelem.n < slots) loc->fl_pelem.alloc(slots);
    }
    loc->fl_table.upload(table.data(), table.size());      // every earlier launch that read these has been waited for
    loc->fl_seeds.upload(seeds_host, (size_t)m * dim);
    A.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.z = loc->fl_table.p;
    A.seeds = loc->fl_seeds.p;
    A.rows = loc->fl_out.p;
    A.end = loc->fl_out.p + rows * flowline::kRowCols;
    A.status = loc->fl_int.p;
    A.count = loc->fl_int.p + rows;
    A.end_element = loc->fl_int.p + 2 * rows;
    A.pts = paths ? loc->fl_pts.p : nullptr;
    A.pelem = paths ? loc->fl_pelem.p : nullptr;
    flowline::launch_trace(st, dim, L.k, A, workgroup ? workgroup : flowline::kDefaultWorkgroup);
    hip_check(hipGetLastError(), "geo_flow_lines launch");
    hip_check(hipStreamSynchronize(st), "sync geo_flow_lines");
    std::vector<double> dbl(nout);
    std::vector<int32_t> ints(3 * rows);
    hip_check(hipMemcpy(dbl.data(), loc->fl_out.p, nout * sizeof(double), hipMemcpyDeviceToHost), "D2H");
    hip_check(hipMemcpy(ints.data(), loc->fl_int.p, 3 * rows * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H");
    std::copy(dbl.begin(), dbl.begin() + rows * flowline::kRowCols, rows_host);
    std::copy(dbl.begin() + rows * flowline::kRowCols, dbl.end(), end_host);
    std::copy(ints.begin(), ints.begin() + rows, status_host);
    std::copy(ints.begin() + rows, ints.begin() + 2 * rows, count_host);
    std::copy(ints.begin() + 2 * rows, ints.end(), end_element_host);
    if (!paths) return;
    for (size_t r = 0; r < rows; ++r) {
      if (count_host[r] < 0 || count_host[r] > A.stride) throw InternalError("geo_flow_lines: a count outside its row");
      out->offsets[r + 1] = out->offsets[r] + count_host[r];
    }
    const long long total = out->offsets[rows];
    if (total > 0) {
      out->pts.alloc((size_t)total * dim);
      out->elem.alloc((size_t)total);
      loc->fl_offsets.upload(out->offsets.data(), rows + 1);
      flowline::launch_compact(st, dim, A, loc->fl_offsets.p, out->pts.p, out->elem.p);
      hip_check(hipGetLastError(), "geo_flow_lines compact launch");
      hip_check(hipStreamSynchronize(st), "sync geo_flow_lines compact");
    }
    *paths = out.release();
  });
}
int mgb_flowpath_get(mgb_flowpath paths, long long* offsets, double* pts, int32_t* elem) {
  return guard([&] {
    need(paths != nullptr, "flowpath_get: null argument");
    hip_check(hipSetDevice(paths->ctx->ctx.device), "hipSetDevice");
    if (offsets) std::copy(paths->offsets.begin(), paths->offsets.end(), offsets);
    if (pts) paths->pts.download(pts, paths->pts.n);
    if (elem) paths->elem.download(elem, paths->elem.n);
  });
}
int mgb_flowpath_destroy(mgb_flowpath paths) {
  return guard([&] { delete paths; });
}
int mgb_geo_flow_lines_host(mgb_geo g, int B, const double* const* z, int S, int u, int m, const double* seeds, double p,
                            int direction, const double* ds_or_null, int max_steps, double gmin, double* rows, double* end,
                            int32_t* status, int32_t* count, int32_t* end_element, double* ds_used, long long* offsets,
                            double* pts, int32_t* elem, long long capacity) {
  return guard([&] {
    need(g && z, "geo_flow_lines_host: null argument");
    need(g->g.dim != 1, "geo_flow_lines_host: flow lines need a 2-D or 3-D geometry");
    const interp::Locator L = interp::build_locator(g->g);
    flowline::Args A{};
    flow_args(A, "geo_flow_lines_host", L.dim, B, S, u, m, p, direction, ds_or_null, L.min_extent, max_steps, gmin,
              offsets != nullptr);
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_flow_lines_host: null field");
    need(m == 0 || (seeds && rows && end && status && count && end_element), "geo_flow_lines_host: null array");
    need((offsets == nullptr) == (pts == nullptr) && (offsets == nullptr) == (elem == nullptr),
         "geo_flow_lines_host: offsets, points and elements come together");
    need(!offsets || capacity >= 0, "geo_flow_lines_host: negative capacity");
    if (ds_used) *ds_used = A.ds;
    A.own = L.view(L.cellptr.data(), L.cellelem.data(), g->g.x.data());
    A.z = z;
    A.seeds = seeds;
    A.rows = rows, A.end = end, A.status = status, A.count = count, A.end_element = end_element;
    flowline::flow_lines_host(L.dim, L.k, A, offsets, pts, elem, capacity);
  });
}

// ---- path lines through the snapshots of a parabolic run (pathline.hpp / pathline.hip); buffers and handle are the flow lines'
int mgb_geo_path_lines(mgb_locator loc, int B, const mgb_vec* z, const double* ts_host, int S, int u, int m,
                       const double* seeds_host, const int32_t* release_host, int stop, int substeps, double p, int direction,
                       double speed, double gmin, int workgroup, double* rows_host, double* end_host, int32_t* status_host,
                       int32_t* count_host, int32_t* end_element_host, int32_t* rested_host, mgb_flowpath* paths) {
  return guard([&] {
    const bool outputs = rows_host && end_host && status_host && count_host && end_element_host && rested_host;
    pathline::Call c{};
    c.null_argument = !(loc && z && ts_host) || (m > 0 && !(seeds_host && release_host && outputs));
    std::vector<long long> len;
    if (!c.null_argument && B >= 2 && B <= 65535) {
      len.resize((size_t)B);
      for (int b = 0; b < B; ++b) len[b] = z[b] == nullptr ? -1 : z[b]->ctx != loc->ctx ? -2 : (long long)z[b]->n;
      c.field_len = len.data();
    }
    if (loc) {
      c.dim = loc->loc.dim;
      c.world = loc->ctx->ctx.world;
      c.want_len = (long long)loc->loc.n * S;
    }
    c.B = B, c.S = S, c.u = u, c.m = m, c.stop = stop, c.substeps = substeps, c.direction = direction, c.workgroup = workgroup;
    c.p = p, c.speed = speed, c.gmin = gmin, c.ts = ts_host, c.release = release_host, c.paths = paths != nullptr;
    pathline::Args A{};
    pathline::check("geo_path_lines", c, A);
    const interp::Locator& L = loc->loc;
    const int dim = L.dim;
    const size_t rows = (size_t)m;
    std::unique_ptr<mgb_flowpath_s> out;
    if (paths) {
      out.reset(new mgb_flowpath_s{loc->ctx, dim, {}, {}, {}});
      out->offsets.assign(rows + 1, 0);
    }
    if (m == 0) {
      if (paths) *paths = out.release();
      return;
    }
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nout = rows * (pathline::kRowCols + dim);
    if (loc->fl_out.n < nout) loc->fl_out.alloc(nout);
    if (loc->fl_int.n < 4 * rows) loc->fl_int.alloc(4 * rows);
    if (paths) {
      const size_t slots = rows * (size_t)A.stride;
      if (loc->fl_pts.n < slots * dim) loc->fl_pts.alloc(slots * dim);
      if (loc->fl_pelem.n < slots) loc->fl_pelem.alloc(slots);
    }
    std::vector<const double*> table((size_t)B);
    for (int b = 0; b < B; ++b) table[b] = z[b]->buf.p;
    loc->fl_table.upload(table.data(), table.size());      // every earlier launch that read these has been waited for
    loc->fl_seeds.upload(seeds_host, (size_t)m * dim);
    loc->pl_ts.upload(ts_host, (size_t)B);
    loc->pl_release.upload(release_host, (size_t)m);
    A.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.z = loc->fl_table.p;
    A.ts = loc->pl_ts.p;
    A.seeds = loc->fl_seeds.p;
    A.release = loc->pl_release.p;
    A.rows = loc->fl_out.p;
    A.end = loc->fl_out.p + rows * pathline::kRowCols;
    A.status = loc->fl_int.p;
    A.count = loc->fl_int.p + rows;
    A.end_element = loc->fl_int.p + 2 * rows;
    A.rested = loc->fl_int.p + 3 * rows;
    A.pts = paths ? loc->fl_pts.p : nullptr;
    A.pelem = paths ? loc->fl_pelem.p : nullptr;
    pathline::launch_advance(st, dim, L.k, A, workgroup ? workgroup : pathline::kDefaultWorkgroup);
    hip_check(hipGetLastError(), "geo_path_lines launch");
    hip_check(hipStreamSynchronize(st), "sync geo_path_lines");
    std::vector<double> dbl(nout);
    std::vector<int32_t> ints(4 * rows);
    hip_check(hipMemcpy(dbl.data(), loc->fl_out.p, nout * sizeof(double), hipMemcpyDeviceToHost), "D2H");
    hip_check(hipMemcpy(ints.data(), loc->fl_int.p, 4 * rows * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H");
    std::copy(dbl.begin(), dbl.begin() + rows * pathline::kRowCols, rows_host);
    std::copy(dbl.begin() + rows * pathline::kRowCols, dbl.end(), end_host);
    std::copy(ints.begin(), ints.begin() + rows, status_host);
    std::copy(ints.begin() + rows, ints.begin() + 2 * rows, count_host);
    std::copy(ints.begin() + 2 * rows, ints.begin() + 3 * rows, end_element_host);
    std::copy(ints.begin() + 3 * rows, ints.end(), rested_host);
    if (!paths) return;
    for (size_t r = 0; r < rows; ++r) {
      if (count_host[r] < 0 || count_host[r] > A.stride) throw InternalError("geo_path_lines: a count outside its row");
      out->offsets[r + 1] = out->offsets[r] + count_host[r];
    }
    const long long total = out->offsets[rows];
    if (total > 0) {
      out->pts.alloc((size_t)total * dim);
      out->elem.alloc((size_t)total);
      loc->fl_offsets.upload(out->offsets.data(), rows + 1);
      flowline::Args F{};      // what compact_kernel reads: the fixed-stride rows, one "field" of m rows
      F.B = 1, F.m = m, F.stride = A.stride, F.pts = A.pts, F.pelem = A.pelem;
      flowline::launch_compact(st, dim, F, loc->fl_offsets.p, out->pts.p, out->elem.p);
      hip_check(hipGetLastError(), "geo_path_lines compact launch");
      hip_check(hipStreamSynchronize(st), "sync geo_path_lines compact");
    }
    *paths = out.release();
  });
}
int mgb_geo_path_lines_host(mgb_geo g, int B, const double* const* z, const double* ts, int S, int u, int m, const double* seeds,
                            const int32_t* release, int stop, int substeps, double p, int direction, double speed, double gmin,
                            double* rows, double* end, int32_t* status, int32_t* count, int32_t* end_element, int32_t* rested,
                            long long* offsets, double* pts, int32_t* elem, long long capacity) {
  return guard([&] {
    pathline::Call c{};
    c.null_argument = !(g && z && ts) || (m > 0 && !(seeds && release && rows && end && status && count && end_element && rested));
    std::vector<long long> len;
    if (!c.null_argument && B >= 2 && B <= 65535) {
      len.resize((size_t)B);
      for (int b = 0; b < B; ++b) len[b] = z[b] == nullptr ? -1 : (long long)g->g.n * S;
      c.field_len = len.data();
    }
    if (g) {
      c.dim = g->g.dim;
      c.want_len = (long long)g->g.n * S;
    }
    c.world = 1;
    c.B = B, c.S = S, c.u = u, c.m = m, c.stop = stop, c.substeps = substeps, c.direction = direction, c.workgroup = 0;
    c.p = p, c.speed = speed, c.gmin = gmin, c.ts = ts, c.release = release, c.paths = offsets != nullptr;
    pathline::Args A{};
    pathline::check("geo_path_lines_host", c, A);
    need((offsets == nullptr) == (pts == nullptr) && (offsets == nullptr) == (elem == nullptr),
         "geo_path_lines_host: offsets, points and elements come together");
    need(!offsets || capacity >= 0, "geo_path_lines_host: negative capacity");
    const interp::Locator L = interp::build_locator(g->g);
    A.own = L.view(L.cellptr.data(), L.cellelem.data(), g->g.x.data());
    A.z = z;
    A.ts = ts;
    A.seeds = seeds;
    A.release = release;
    A.rows = rows, A.end = end, A.status = status, A.count = count, A.end_element = end_element, A.rested = rested;
    pathline::path_lines_host(L.dim, L.k, A, offsets, pts, elem, capacity);
  });
}

// ---- isosurfaces of 3-D nodal fields (isosurface.hpp / isosurface.hip); the buffers and the handle are the level sets'
namespace {
void need_isosurfaces(const char* who, int B, int S, int u, int nl, const double* levels, int dim, int refine) {
  const std::string w(who);
  if (B < 1) throw std::invalid_argument(w + ": B must be >= 1");
  if (nl < 1) throw std::invalid_argument(w + ": nl must be >= 1");
  if (S < 1) throw std::invalid_argument(w + ": S must be >= 1");
  if (u < 0 || u >= S) throw std::invalid_argument(w + ": column u outside [0, S)");
  if (dim != 3) throw std::invalid_argument(w + ": a 3-D geometry is needed; 1-D and 2-D fields go to level_sets");
  if (refine < 0 || refine > isosurface::kMaxRefine) throw std::invalid_argument(w + ": refine must be 0, 1 or 2");
  for (int l = 0; l < nl; ++l)
    if (!interp::finite(levels[l])) throw std::invalid_argument(w + ": every level must be finite");
}
}  // namespace
int mgb_geo_isosurfaces(mgb_locator loc, int B, const mgb_vec* z, int S, int u, int nl, const double* levels_host, int refine,
                        double* out_host, long long* counts_host, mgb_levelset* tris) {
  return guard([&] {
    need(loc && z && levels_host && out_host && counts_host, "geo_isosurfaces: null argument");
    const interp::Locator& L = loc->loc;
    need(B <= 65535 && nl <= 65535, "geo_isosurfaces: at most 65535 fields and 65535 levels per call");      // before any is read
    need_isosurfaces("geo_isosurfaces", B, S, u, nl, levels_host, L.dim, refine);
    need(loc->ctx->ctx.world == 1, "geo_isosurfaces: sharded contexts are not supported");
    std::vector<const double*> table;
    field_table("geo_isosurfaces", loc, B, z, S, table);
    levelset::Args A;
    A.items = isosurface::items_per_row(L.k, L.nel, refine);
    need(A.items <= INT_MAX, "geo_isosurfaces: more than INT_MAX items per row");
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t rows = (size_t)B * nl, nwg = (size_t)reduce::workgroups(A.items);
    const size_t nd = levelset::scratch_words(rows, nwg), nc = levelset::count_words(rows, nwg);
    if (loc->ls_scratch.n < nd) loc->ls_scratch.alloc(nd);
    if (loc->ls_counts.n < nc) loc->ls_counts.alloc(nc);
    loc->ls_table.upload(table.data(), table.size());      // every earlier launch that read these has been waited for
    loc->ls_levels.upload(levels_host, (size_t)nl);
    A.x = loc->x.p;
    A.z = loc->ls_table.p;
    A.levels = loc->ls_levels.p;
    A.nel = L.nel, A.S = S, A.u = u, A.B = B, A.nl = nl, A.refine = refine;
    isosurface::launch_measure(st, L.k, A, loc->ls_scratch.p, loc->ls_counts.p);
    hip_check(hipGetLastError(), "geo_isosurfaces launch");
    hip_check(hipStreamSynchronize(st), "sync geo_isosurfaces");
    // the rows and the totals lie behind each other: one copy
    std::vector<double> both(rows * (reduce::kCols + 1));
    hip_check(hipMemcpy(both.data(), loc->ls_scratch.p + levelset::results_offset(rows, nwg), both.size() * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
    std::copy(both.begin(), both.begin() + rows * reduce::kCols, out_host);
    std::memcpy(counts_host, both.data() + rows * reduce::kCols, rows * sizeof(long long));
    if (!tris) return;
    std::unique_ptr<mgb_levelset_s> out(new mgb_levelset_s{loc->ctx, isosurface::kTriWidth, {}, {}, {}});
    out->row_offsets.resize(rows + 1);
    out->row_offsets[0] = 0;
    for (size_t r = 0; r < rows; ++r) out->row_offsets[r + 1] = out->row_offsets[r] + counts_host[r];
    const long long total = out->row_offsets[rows];
    if (total > 0) {
      out->seg.alloc((size_t)total * out->width);
      out->item.alloc((size_t)total);
      loc->ls_row_base.upload(out->row_offsets.data(), rows);
      isosurface::launch_emit(st, L.k, A, loc->ls_counts.p + levelset::offsets_offset(rows, nwg), loc->ls_row_base.p, total,
                              out->seg.p, out->item.p);
      hip_check(hipGetLastError(), "geo_isosurfaces emit launch");
      hip_check(hipStreamSynchronize(st), "sync geo_isosurfaces emit");
    }
    *tris = out.release();
  });
}
int mgb_geo_isosurfaces_host(mgb_geo g, int B, const double* const* z, int S, int u, int nl, const double* levels, int refine,
                             double* out, long long* counts, long long* row_offsets, double* tri, int32_t* item, long long capacity) {
  return guard([&] {
    need(g && z && levels && out && counts, "geo_isosurfaces_host: null argument");
    need_isosurfaces("geo_isosurfaces_host", B, S, u, nl, levels, g->g.dim, refine);
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_isosurfaces_host: null field");
    need((tri == nullptr) == (item == nullptr), "geo_isosurfaces_host: tri and item come together");
    need(!tri || capacity >= 0, "geo_isosurfaces_host: negative capacity");
    const interp::Locator L = interp::build_locator(g->g);      // validates the blocks: tensor nodes of the corner box
    levelset::Args A;
    A.items = isosurface::items_per_row(L.k, L.nel, refine);
    need(A.items <= INT_MAX, "geo_isosurfaces_host: more than INT_MAX items per row");
    A.x = g->g.x.data();
    A.z = z;
    A.levels = levels;
    A.nel = L.nel, A.S = S, A.u = u, A.B = B, A.nl = nl, A.refine = refine;
    isosurface::isosurfaces_host(L.k, A, out, counts, row_offsets, tri, item, capacity);
  });
}

// ---- plane sections of nodal fields (section.hpp / section.hip); the buffers and the handle are the level sets'
namespace {
// what both entry points fill alike; section::check, the one place where these arguments are judged, runs on it at once
void section_args(section::Args& A, const char* who, const interp::Locator& L, const double* x, int B, int S, int u, int nc, double p) {
  A.own = L.view(nullptr, nullptr, x);
  A.items = section::items_per_row(L.dim, L.nel);
  A.p = p;
  A.nel = L.nel, A.S = S, A.u = u, A.B = B, A.nc = nc;
  section::check(who, A, L.dim, L.k);
}
}  // namespace
int mgb_geo_sections(mgb_locator loc, int B, const mgb_vec* z, int S, int u, int nc, const double* planes_host, double p,
                     double* out_host, long long* counts_host, mgb_levelset* pieces) {
  return guard([&] {
    need(loc && z && planes_host && out_host && counts_host, "geo_sections: null argument");
    const interp::Locator& L = loc->loc;
    need(B <= 65535 && nc <= 65535, "geo_sections: at most 65535 fields and 65535 planes per call");      // before any is read
    section::Args A;
    section_args(A, "geo_sections", L, loc->x.p, B, S, u, nc, p);
    section::check_planes("geo_sections", L.dim, nc, planes_host);
    need(loc->ctx->ctx.world == 1, "geo_sections: sharded contexts are not supported");
    std::vector<const double*> table;
    field_table("geo_sections", loc, B, z, S, table);
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t rows = (size_t)B * nc, nwg = (size_t)reduce::workgroups(A.items);
    const size_t nd = levelset::scratch_words(rows, nwg), nw = levelset::count_words(rows, nwg);
    if (loc->ls_scratch.n < nd) loc->ls_scratch.alloc(nd);
    if (loc->ls_counts.n < nw) loc->ls_counts.alloc(nw);
    loc->ls_table.upload(table.data(), table.size());      // every earlier launch that read these has been waited for
    loc->ls_levels.upload(planes_host, (size_t)nc * (L.dim + 1));
    A.z = loc->ls_table.p;
    A.planes = loc->ls_levels.p;
    section::launch_measure(st, L.dim, L.k, A, loc->ls_scratch.p, loc->ls_counts.p);
    hip_check(hipGetLastError(), "geo_sections launch");
    hip_check(hipStreamSynchronize(st), "sync geo_sections");
    // the rows and the totals lie behind each other: one copy
    std::vector<double> both(rows * (reduce::kCols + 1));
    hip_check(hipMemcpy(both.data(), loc->ls_scratch.p + levelset::results_offset(rows, nwg), both.size() * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
    std::copy(both.begin(), both.begin() + rows * reduce::kCols, out_host);
    std::memcpy(counts_host, both.data() + rows * reduce::kCols, rows * sizeof(long long));
    if (!pieces) return;
    std::unique_ptr<mgb_levelset_s> out(new mgb_levelset_s{loc->ctx, section::piece_width(L.dim), {}, {}, {}});
    out->row_offsets.resize(rows + 1);
    out->row_offsets[0] = 0;
    for (size_t r = 0; r < rows; ++r) out->row_offsets[r + 1] = out->row_offsets[r] + counts_host[r];
    const long long total = out->row_offsets[rows];
    if (total > 0) {
      out->seg.alloc((size_t)total * out->width);
      out->item.alloc((size_t)total);
      loc->ls_row_base.upload(out->row_offsets.data(), rows);
      section::launch_emit(st, L.dim, L.k, A, loc->ls_counts.p + levelset::offsets_offset(rows, nwg), loc->ls_row_base.p, total,
                           out->seg.p, out->item.p);
      hip_check(hipGetLastError(), "geo_sections emit launch");
      hip_check(hipStreamSynchronize(st), "sync geo_sections emit");
    }
    *pieces = out.release();
  });
}
int mgb_geo_sections_host(mgb_geo g, int B, const double* const* z, int S, int u, int nc, const double* planes, double p,
                          double* out, long long* counts, long long* row_offsets, double* piece, int32_t* item, long long capacity) {
  return guard([&] {
    need(g && z && planes && out && counts, "geo_sections_host: null argument");
    const interp::Locator L = interp::build_locator(g->g);      // validates the blocks: straight triangles, tensor nodes of the corner box
    section::Args A;
    section_args(A, "geo_sections_host", L, g->g.x.data(), B, S, u, nc, p);
    section::check_planes("geo_sections_host", L.dim, nc, planes);
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_sections_host: null field");
    need((piece == nullptr) == (item == nullptr), "geo_sections_host: piece and item come together");
    need(!piece || capacity >= 0, "geo_sections_host: negative capacity");
    A.z = z;
    A.planes = planes;
    section::sections_host(L.dim, L.k, A, out, counts, row_offsets, piece, item, capacity);
  });
}

// ---- line integrals of nodal fields (ray.hpp / ray.hip); the pieces come back through the level sets' handle
int mgb_geo_line_integrals(mgb_locator loc, int B, const mgb_vec* z, int S, int u, int m, const double* a_host, const double* b_host,
                           double p, int workgroup, double* rows_host, int32_t* count_host, mgb_levelset* pieces) {
  return guard([&] {
    ray::Call c{};
    c.null_argument = !(loc && z) || (m > 0 && !(a_host && b_host && rows_host && count_host));
    std::vector<long long> len;
    if (!c.null_argument && B >= 1 && B <= 65535) {
      len.resize((size_t)B);
      for (int b = 0; b < B; ++b) len[b] = z[b] == nullptr ? -1 : z[b]->ctx != loc->ctx ? -2 : (long long)z[b]->n;
      c.field_len = len.data();
    }
    if (loc) {
      c.dim = loc->loc.dim;
      c.world = loc->ctx->ctx.world;
      c.want_len = (long long)loc->loc.n * S;
    }
    c.B = B, c.S = S, c.u = u, c.m = m, c.workgroup = workgroup, c.p = p;
    ray::check("geo_line_integrals", c);
    const interp::Locator& L = loc->loc;
    const int dim = L.dim;
    const size_t rows = (size_t)B * m;
    std::unique_ptr<mgb_levelset_s> out;
    if (pieces) {
      out.reset(new mgb_levelset_s{loc->ctx, ray::kPieceWidth, {}, {}, {}});
      out->row_offsets.assign(rows + 1, 0);
    }
    if (m == 0) {
      if (pieces) *pieces = out.release();
      return;
    }
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t npts = (size_t)m * dim;
    if (loc->ry_ab.n < 2 * npts) loc->ry_ab.alloc(2 * npts);
    if (loc->ry_rows.n < rows * ray::kCols) loc->ry_rows.alloc(rows * ray::kCols);
    if (loc->ry_count.n < rows) loc->ry_count.alloc(rows);
    std::vector<const double*> table((size_t)B);
    for (int b = 0; b < B; ++b) table[b] = z[b]->buf.p;
    loc->ry_table.upload(table.data(), table.size());      // every earlier launch that read these has been waited for
    std::vector<double> ab(2 * npts);
    std::copy(a_host, a_host + npts, ab.begin());
    std::copy(b_host, b_host + npts, ab.begin() + npts);
    hip_check(hipMemcpy(loc->ry_ab.p, ab.data(), 2 * npts * sizeof(double), hipMemcpyHostToDevice), "H2D");
    ray::Args A;
    A.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.z = loc->ry_table.p;
    A.a = loc->ry_ab.p;
    A.b = loc->ry_ab.p + npts;
    A.p = p;
    A.m = m, A.S = S, A.u = u, A.B = B;
    A.rows = loc->ry_rows.p;
    A.count = loc->ry_count.p;
    const int wg = workgroup ? workgroup : ray::kDefaultWorkgroup;
    ray::launch_measure(st, dim, L.k, A, wg);
    hip_check(hipGetLastError(), "geo_line_integrals launch");
    hip_check(hipStreamSynchronize(st), "sync geo_line_integrals");
    hip_check(hipMemcpy(rows_host, loc->ry_rows.p, rows * ray::kCols * sizeof(double), hipMemcpyDeviceToHost), "D2H");
    hip_check(hipMemcpy(count_host, loc->ry_count.p, rows * sizeof(int32_t), hipMemcpyDeviceToHost), "D2H");
    if (!pieces) return;
    for (size_t r = 0; r < rows; ++r) {
      if (count_host[r] < 0) throw InternalError("geo_line_integrals: a negative count");
      out->row_offsets[r + 1] = out->row_offsets[r] + count_host[r];
    }
    const long long total = out->row_offsets[rows];
    if (total > 0) {
      out->seg.alloc((size_t)total * out->width);
      out->item.alloc((size_t)total);
      loc->ry_offsets.upload(out->row_offsets.data(), rows + 1);
      ray::launch_emit(st, dim, L.k, A, wg, loc->ry_offsets.p, out->seg.p, out->item.p);
      hip_check(hipGetLastError(), "geo_line_integrals emit launch");
      hip_check(hipStreamSynchronize(st), "sync geo_line_integrals emit");
    }
    *pieces = out.release();
  });
}
int mgb_geo_line_integrals_host(mgb_geo g, int B, const double* const* z, int S, int u, int m, const double* a, const double* b,
                                double p, double* rows, int32_t* count, long long* offsets, double* piece, int32_t* elem,
                                long long capacity) {
  return guard([&] {
    ray::Call c{};
    c.null_argument = !(g && z) || (m > 0 && !(a && b && rows && count));
    std::vector<long long> len;
    if (!c.null_argument && B >= 1 && B <= 65535) {
      len.resize((size_t)B);
      for (int k = 0; k < B; ++k) len[k] = z[k] == nullptr ? -1 : (long long)g->g.n * S;
      c.field_len = len.data();
    }
    if (g) {
      c.dim = g->g.dim;
      c.want_len = (long long)g->g.n * S;
    }
    c.world = 1;
    c.B = B, c.S = S, c.u = u, c.m = m, c.workgroup = 0, c.p = p;
    ray::check("geo_line_integrals_host", c);
    need((offsets == nullptr) == (piece == nullptr) && (offsets == nullptr) == (elem == nullptr),
         "geo_line_integrals_host: offsets, pieces and elements come together");
    need(!offsets || capacity >= 0, "geo_line_integrals_host: negative capacity");
    if (m == 0) {
      if (offsets) offsets[0] = 0;
      return;
    }
    const interp::Locator L = interp::build_locator(g->g);
    ray::Args A;
    A.own = L.view(L.cellptr.data(), L.cellelem.data(), g->g.x.data());
    A.z = z;
    A.a = a, A.b = b;
    A.p = p;
    A.m = m, A.S = S, A.u = u, A.B = B;
    A.rows = rows, A.count = count;
    ray::line_integrals_host(L.dim, L.k, A, offsets, piece, elem, capacity);
  });
}

// ---- boundary facets and boundary integrals of p-Laplace solutions (boundary.hpp / boundary.hip)
namespace {
void copy_facets(const boundary::Facets& F, int32_t* element, int32_t* nodes, double* weights, double* normal, double* measure,
                 double* centre) {
  if (element) std::copy(F.element.begin(), F.element.end(), element);
  if (nodes) std::copy(F.nodes.begin(), F.nodes.end(), nodes);
  if (weights) std::copy(F.weights.begin(), F.weights.end(), weights);
  if (normal) std::copy(F.normal.begin(), F.normal.end(), normal);
  if (measure) std::copy(F.measure.begin(), F.measure.end(), measure);
  if (centre) std::copy(F.centre.begin(), F.centre.end(), centre);
}
}  // namespace
int mgb_boundary_create(mgb_locator loc, mgb_geo g, mgb_boundary* out) {
  return guard([&] {
    need(loc && g && out, "boundary_create: null argument");
    const interp::Locator& L = loc->loc;
    need(L.n == g->g.n && L.dim == g->g.dim && L.block == g->g.block, "boundary_create: the locator belongs to another geometry");
    auto* b = new mgb_boundary_s();
    try {
      b->loc = loc;
      boundary::build_facet_lists(g->g, &b->F, &b->I);
      hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
      b->nodes.upload(b->F.nodes.data(), b->F.nodes.size());
      b->weights.upload(b->F.weights.data(), b->F.weights.size());
      b->normal.upload(b->F.normal.data(), b->F.normal.size());
      b->inc = boundary::build_incidence(b->F);
      b->inc_rows.upload(b->inc.rows.data(), b->inc.rows.size());
      b->inc_start.upload(b->inc.start.data(), b->inc.start.size());
      b->inc_idx.upload(b->inc.idx.data(), b->inc.idx.size());
      b->inodes.upload(b->I.nodes.data(), b->I.nodes.size());
      b->iweights.upload(b->I.weights.data(), b->I.weights.size());
      b->inormal.upload(b->I.normal.data(), b->I.normal.size());
      b->elem_facet.upload(b->I.elem_facet.data(), b->I.elem_facet.size());
    } catch (...) {
      delete b;
      throw;
    }
    *out = b;
  });
}
int mgb_boundary_destroy(mgb_boundary b) {
  return guard([&] { delete b; });
}
int mgb_boundary_dims(mgb_boundary b, int* nf, int* q, int* dim) {
  return guard([&] {
    need(b, "boundary_dims: null boundary");
    if (nf) *nf = b->F.nf;
    if (q) *q = b->F.q;
    if (dim) *dim = b->F.dim;
  });
}
int mgb_boundary_get(mgb_boundary b, int32_t* element, int32_t* nodes, double* weights, double* normal, double* measure,
                     double* centre) {
  return guard([&] {
    need(b, "boundary_get: null boundary");
    copy_facets(b->F, element, nodes, weights, normal, measure, centre);
  });
}
int mgb_boundary_flux(mgb_boundary bd, int B, const mgb_vec* z, int S, int u, double p, mgb_vec p_nodal,
                      const unsigned char* mask_host, double* facet_flux_host, double* out_host) {
  return guard([&] {
    need(bd && z && out_host, "boundary_flux: null argument");
    need_field_shape("boundary_flux", B, S, u, p);
    mgb_locator_s* loc = bd->loc;
    need(loc->ctx->ctx.world == 1, "boundary_flux: sharded contexts are not supported");
    const interp::Locator& L = loc->loc;
    const boundary::Facets& F = bd->F;
    std::vector<const double*> table;
    field_table("boundary_flux", loc, B, z, S, table);
    need(!p_nodal || p_nodal->n == L.n, "boundary_flux: p_nodal must hold n values");
    need(!p_nodal || p_nodal->ctx == loc->ctx, "boundary_flux: vectors of another context");
    need(B <= 65535, "boundary_flux: at most 65535 fields per call");
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nd = boundary::scratch_doubles(F.nf, F.q, B);
    if (bd->scratch.n < nd) bd->scratch.alloc(nd);
    const size_t nfac = (size_t)B * F.nf;
    if (facet_flux_host && bd->facet_scratch.n < nfac) bd->facet_scratch.alloc(nfac);
    bd->table.upload(table.data(), table.size());      // every earlier launch that read it has been waited for
    if (mask_host && F.nf) {
      if (bd->mask.n < (size_t)F.nf) bd->mask.alloc((size_t)F.nf);
      hip_check(hipMemcpyAsync(bd->mask.p, mask_host, (size_t)F.nf, hipMemcpyHostToDevice, st), "H2D mask");
    }
    boundary::Args A;
    A.E.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    A.E.w = loc->w.p;
    A.E.p_nodal = p_nodal ? p_nodal->buf.p : nullptr;
    A.E.p = p;
    A.E.z = bd->table.p;
    A.E.n = L.n, A.E.S = S, A.E.u = u, A.E.B = B;
    A.nodes = bd->nodes.p;
    A.weights = bd->weights.p;
    A.normal = bd->normal.p;
    A.mask = mask_host && F.nf ? bd->mask.p : nullptr;
    A.nf = F.nf, A.q = F.q;
    boundary::launch_boundary_flux(st, L.dim, L.k, A, bd->scratch.p, facet_flux_host && nfac ? bd->facet_scratch.p : nullptr);
    hip_check(hipGetLastError(), "boundary_flux launch");
    hip_check(hipStreamSynchronize(st), "sync boundary_flux");
    hip_check(hipMemcpy(out_host, bd->scratch.p + boundary::results_offset(F.nf, F.q, B), (size_t)B * reduce::kCols * sizeof(double),
                        hipMemcpyDeviceToHost), "D2H");
    if (facet_flux_host && nfac)
      hip_check(hipMemcpy(facet_flux_host, bd->facet_scratch.p, nfac * sizeof(double), hipMemcpyDeviceToHost), "D2H");
  });
}
int mgb_geo_boundary_dims(mgb_geo g, int* nf, int* q, int* dim) {
  return guard([&] {
    need(g, "geo_boundary_dims: null geometry");
    const boundary::Facets F = boundary::build_facets(g->g);
    if (nf) *nf = F.nf;
    if (q) *q = F.q;
    if (dim) *dim = F.dim;
  });
}
int mgb_geo_boundary_get(mgb_geo g, int32_t* element, int32_t* nodes, double* weights, double* normal, double* measure,
                         double* centre) {
  return guard([&] {
    need(g, "geo_boundary_get: null geometry");
    copy_facets(boundary::build_facets(g->g), element, nodes, weights, normal, measure, centre);
  });
}
int mgb_geo_boundary_flux_host(mgb_geo g, int B, const double* const* z, int S, int u, double p, const double* p_nodal,
                               const unsigned char* mask, double* facet_flux, double* out) {
  return guard([&] {
    need(g && z && out, "geo_boundary_flux_host: null argument");
    need_field_shape("geo_boundary_flux_host", B, S, u, p);
    for (int b = 0; b < B; ++b) need(z[b] != nullptr, "geo_boundary_flux_host: null field");
    need(g->g.w.size() == (size_t)g->g.n, "geo_boundary_flux_host: the geometry must carry one weight per node");
    const boundary::Facets F = boundary::build_facets(g->g);
    boundary::Args A;
    A.E.own.block = g->g.block;
    A.E.own.nel = g->g.n / g->g.block;
    A.E.own.x = g->g.x.data();
    A.E.w = g->g.w.data();
    A.E.p_nodal = p_nodal;
    A.E.p = p;
    A.E.z = z;
    A.E.n = g->g.n, A.E.S = S, A.E.u = u, A.E.B = B;
    A.nodes = F.nodes.data();
    A.weights = F.weights.data();
    A.normal = F.normal.data();
    A.mask = mask;
    A.nf = F.nf, A.q = F.q;
    boundary::boundary_flux_host(F.dim, F.k, A, out, facet_flux);
  });
}

// ---- residual error indicators (estimate.hpp / estimate.hip)
namespace {
// the power and the scale on top of one field
void need_estimate_shape(const char* who, int S, int u, double p, double r, int own_scale, double scale) {
  const std::string w(who);
  need_field_shape(w, 1, S, u, p);
  if (!good_q(r)) throw std::invalid_argument(w + ": r must be finite and >= 1");
  if (own_scale && !std::isfinite(scale)) throw std::invalid_argument(w + ": the scale must be finite");
}
}  // namespace
int mgb_geo_interior_dims(mgb_geo g, int* nif, int* q, int* dim, int* nel, int* nlf) {
  return guard([&] {
    need(g, "geo_interior_dims: null geometry");
    const boundary::Interior I = boundary::build_interior(g->g);
    if (nif) *nif = I.nif;
    if (q) *q = I.q;
    if (dim) *dim = I.dim;
    if (nel) *nel = I.nel;
    if (nlf) *nlf = I.nlf;
  });
}
int mgb_geo_interior_get(mgb_geo g, int32_t* elements, int32_t* nodes, double* weights, double* normal, double* measure,
                         double* centre, int32_t* elem_facet) {
  return guard([&] {
    need(g, "geo_interior_get: null geometry");
    const boundary::Interior I = boundary::build_interior(g->g);
    if (elements) std::copy(I.elements.begin(), I.elements.end(), elements);
    if (nodes) std::copy(I.nodes.begin(), I.nodes.end(), nodes);
    if (weights) std::copy(I.weights.begin(), I.weights.end(), weights);
    if (normal) std::copy(I.normal.begin(), I.normal.end(), normal);
    if (measure) std::copy(I.measure.begin(), I.measure.end(), measure);
    if (centre) std::copy(I.centre.begin(), I.centre.end(), centre);
    if (elem_facet) std::copy(I.elem_facet.begin(), I.elem_facet.end(), elem_facet);
  });
}
int mgb_estimate(mgb_boundary bd, mgb_vec z, int S, int u, double p, mgb_vec p_nodal, mgb_vec f, double r, int own_scale,
                 double scale, const double* h_host, const unsigned char* mask_host, mgb_vec eta, double* out_host) {
  return guard([&] {
    need(bd && z && eta && out_host, "estimate: null argument");
    need_estimate_shape("estimate", S, u, p, r, own_scale, scale);
    mgb_locator_s* loc = bd->loc;
    need(loc->ctx->ctx.world == 1, "estimate: sharded contexts are not supported");
    const interp::Locator& L = loc->loc;
    const boundary::Facets& F = bd->F;
    const boundary::Interior& I = bd->I;
    need(z->n == (long long)L.n * S, "estimate: z must hold n x S values");
    need(eta->n == (long long)I.nel * estimate::kParts, "estimate: eta must hold nel x 3 values");
    need(!p_nodal || p_nodal->n == L.n, "estimate: p_nodal must hold n values");
    need(!f || f->n == L.n, "estimate: f must hold n values");
    need(z->ctx == loc->ctx && eta->ctx == loc->ctx && (!p_nodal || p_nodal->ctx == loc->ctx) && (!f || f->ctx == loc->ctx),
         "estimate: vectors of another context");
    need(z != eta, "estimate: eta must not be z");
    const bool neu = h_host != nullptr && F.nf > 0;
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const int facets = I.nif + (neu ? F.nf : 0);
    const size_t nsig = (size_t)L.n * L.dim, nd = estimate::scratch_doubles(I.nel, L.block, facets, F.q), nh = (size_t)F.nf * F.q;
    // an earlier call's launches may still read the buffers: wait before any of them is replaced
    if (bd->est_sigma.n < nsig || bd->est_J.n < (size_t)I.nif || bd->est_scratch.n < nd || (neu && (bd->est_N.n < (size_t)F.nf ||
        bd->est_h.n < nh || (mask_host && bd->mask.n < (size_t)F.nf)))) {
      hip_check(hipStreamSynchronize(st), "sync estimate");
      if (bd->est_sigma.n < nsig) bd->est_sigma.alloc(nsig);
      if (bd->est_J.n < (size_t)I.nif) bd->est_J.alloc((size_t)I.nif);
      if (bd->est_scratch.n < nd) bd->est_scratch.alloc(nd);
      if (neu && bd->est_N.n < (size_t)F.nf) bd->est_N.alloc((size_t)F.nf);
      if (neu && bd->est_h.n < nh) bd->est_h.alloc(nh);
      if (neu && mask_host && bd->mask.n < (size_t)F.nf) bd->mask.alloc((size_t)F.nf);
    }
    if (neu) {
      hip_check(hipMemcpyAsync(bd->est_h.p, h_host, nh * sizeof(double), hipMemcpyHostToDevice, st), "H2D h");
      if (mask_host) hip_check(hipMemcpyAsync(bd->mask.p, mask_host, (size_t)F.nf, hipMemcpyHostToDevice, st), "H2D mask");
    }
    energy::Args E;
    E.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    E.w = loc->w.p;
    E.p_nodal = p_nodal ? p_nodal->buf.p : nullptr;
    E.p = p;
    E.n = L.n, E.S = S, E.u = u, E.B = 1;
    energy::launch_field_flux(st, L.dim, L.k, E, z->buf.p, bd->est_sigma.p);
    hip_check(hipGetLastError(), "estimate flux launch");
    estimate::Args A;
    A.own = E.own;
    A.w = E.w, A.p_nodal = E.p_nodal, A.p = p;
    A.sigma = bd->est_sigma.p;
    A.f = f ? f->buf.p : nullptr;
    A.r = r, A.scale = scale, A.own_scale = own_scale != 0;
    A.n = L.n, A.nel = I.nel, A.nlf = I.nlf, A.q = F.q;
    A.inodes = bd->inodes.p, A.iweights = bd->iweights.p, A.inormal = bd->inormal.p, A.nif = I.nif;
    A.bnodes = bd->nodes.p, A.bweights = bd->weights.p, A.bnormal = bd->normal.p;
    A.mask = neu && mask_host ? bd->mask.p : nullptr;
    A.h = neu ? bd->est_h.p : nullptr;
    A.nf = F.nf;
    A.elem_facet = bd->elem_facet.p;
    estimate::launch_estimate(st, L.dim, L.k, A, bd->est_J.p, bd->est_N.p, eta->buf.p, bd->est_scratch.p);
    hip_check(hipGetLastError(), "estimate launch");
    hip_check(hipStreamSynchronize(st), "sync estimate");
    hip_check(hipMemcpy(out_host, bd->est_scratch.p + estimate::results_offset(I.nel, L.block, facets, F.q),
                        reduce::kCols * sizeof(double), hipMemcpyDeviceToHost), "D2H");
  });
}
int mgb_geo_estimate_host(mgb_geo g, const double* z, int S, int u, double p, const double* p_nodal, const double* f, double r,
                          int own_scale, double scale, const double* h, const unsigned char* mask, double* eta, double* J, double* N,
                          double* sigma_out, double* out) {
  return guard([&] {
    need(g && z && eta && out, "geo_estimate_host: null argument");
    need_estimate_shape("geo_estimate_host", S, u, p, r, own_scale, scale);
    need(g->g.w.size() == (size_t)g->g.n, "geo_estimate_host: the geometry must carry one weight per node");
    if (p_nodal)
      for (int i = 0; i < g->g.n; ++i) need(good_q(p_nodal[i]), "geo_estimate_host: every p_nodal must be finite and >= 1");
    boundary::Facets F;
    boundary::Interior I;
    boundary::build_facet_lists(g->g, &F, &I);
    const int n = g->g.n, dim = F.dim;
    energy::Args E;
    E.own.block = g->g.block;
    E.own.nel = n / g->g.block;
    E.own.x = g->g.x.data();
    E.w = g->g.w.data();
    E.p_nodal = p_nodal;
    E.p = p;
    E.n = n, E.S = S, E.u = u, E.B = 1;
    std::vector<double> sigma((size_t)n * dim), Jv((size_t)I.nif), Nv((size_t)F.nf);
    estimate::field_flux_host(dim, F.k, E, z, sigma.data());
    const bool neu = h != nullptr && F.nf > 0;
    estimate::Args A;
    A.own = E.own;
    A.w = E.w, A.p_nodal = p_nodal, A.p = p;
    A.sigma = sigma.data();
    A.f = f;
    A.r = r, A.scale = scale, A.own_scale = own_scale != 0;
    A.n = n, A.nel = I.nel, A.nlf = I.nlf, A.q = F.q;
    A.inodes = I.nodes.data(), A.iweights = I.weights.data(), A.inormal = I.normal.data(), A.nif = I.nif;
    A.bnodes = F.nodes.data(), A.bweights = F.weights.data(), A.bnormal = F.normal.data();
    A.mask = neu ? mask : nullptr;
    A.h = neu ? h : nullptr;
    A.nf = F.nf;
    A.elem_facet = I.elem_facet.data();
    std::vector<double> etav((size_t)I.nel * estimate::kParts);
    double res[reduce::kCols];
    estimate::estimate_host(dim, F.k, A, etav.data(), Jv.data(), Nv.data(), res);
    std::copy(etav.begin(), etav.end(), eta);
    if (J) std::copy(Jv.begin(), Jv.end(), J);
    if (N) {
      if (neu) std::copy(Nv.begin(), Nv.end(), N);
      else std::fill(N, N + F.nf, 0.0);
    }
    if (sigma_out) std::copy(sigma.begin(), sigma.end(), sigma_out);
    std::copy(res, res + reduce::kCols, out);
  });
}

// ---- error indicators of the steps of a parabolic run (estimate.hpp / estimate.hip)
namespace {
void need_steps_shape(const char* who, int B, const double* ts, int S, int u, double p, double r, double scale, bool has_f, int f_rows,
                      bool has_h, int h_rows) {
  const std::string w(who);
  need_field_shape(w, B, S, u, p);
  if (B + 1 > 65535) throw std::invalid_argument(w + ": at most 65535 snapshots per call");
  for (int k = 0; k <= B; ++k)
    if (!std::isfinite(ts[k]) || (k > 0 && !(ts[k] > ts[k - 1]))) throw std::invalid_argument(w + ": ts must be finite and strictly increasing");
  if (!good_q(r)) throw std::invalid_argument(w + ": r must be finite and >= 1");
  if (!std::isfinite(scale)) throw std::invalid_argument(w + ": the scale must be finite");
  if (has_f && f_rows != 1 && f_rows != B) throw std::invalid_argument(w + ": f must have 1 or B rows");
  if (has_h && h_rows != 1 && h_rows != B) throw std::invalid_argument(w + ": h must have 1 or B rows");
}
}  // namespace
int mgb_estimate_steps(mgb_boundary bd, int B, const mgb_vec* z, const double* ts_host, int S, int u, double p, mgb_vec p_nodal,
                       mgb_vec f, int f_rows, double r, double scale, const double* h_host, int h_rows, const unsigned char* mask_host,
                       mgb_vec sigma, mgb_vec parts, double* out_host) {
  return guard([&] {
    need(bd && z && ts_host && sigma && parts && out_host, "estimate_steps: null argument");
    need_steps_shape("estimate_steps", B, ts_host, S, u, p, r, scale, f != nullptr, f_rows, h_host != nullptr, h_rows);
    mgb_locator_s* loc = bd->loc;
    need(loc->ctx->ctx.world == 1, "estimate_steps: sharded contexts are not supported");
    const interp::Locator& L = loc->loc;
    const boundary::Facets& F = bd->F;
    const boundary::Interior& I = bd->I;
    std::vector<const double*> table;
    field_table("estimate_steps", loc, B + 1, z, S, table);
    need(sigma->n == (long long)(B + 1) * L.n * L.dim, "estimate_steps: sigma must hold (B + 1) x n x dim values");
    need(parts->n == (long long)B * I.nel * estimate::kStepParts, "estimate_steps: parts must hold B x nel x 4 values");
    need(!p_nodal || p_nodal->n == L.n, "estimate_steps: p_nodal must hold n values");
    need(!f || f->n == (long long)f_rows * L.n, "estimate_steps: f must hold f_rows x n values");
    need(sigma->ctx == loc->ctx && parts->ctx == loc->ctx && (!p_nodal || p_nodal->ctx == loc->ctx) && (!f || f->ctx == loc->ctx),
         "estimate_steps: vectors of another context");
    need(sigma != parts && sigma != p_nodal && sigma != f && parts != p_nodal && parts != f, "estimate_steps: an output is also an input");
    for (int b = 0; b <= B; ++b) need(z[b] != sigma && z[b] != parts, "estimate_steps: an output is also an input");
    const bool neu = h_host != nullptr && F.nf > 0;
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const int facets = I.nif + (neu ? F.nf : 0);
    const size_t nJ = (size_t)B * I.nif, nN = (size_t)B * F.nf, nd = estimate::scratch_doubles(I.nel, L.block, facets, F.q, B, 2),
                 nh = (size_t)(neu ? h_rows : 0) * F.nf * F.q;
    // an earlier call's launches may still read the buffers: wait before any of them is replaced
    if (bd->est_J.n < nJ || bd->est_scratch.n < nd || (neu && (bd->est_N.n < nN || bd->est_h.n < nh ||
        (mask_host && bd->mask.n < (size_t)F.nf)))) {
      hip_check(hipStreamSynchronize(st), "sync estimate_steps");
      if (bd->est_J.n < nJ) bd->est_J.alloc(nJ);
      if (bd->est_scratch.n < nd) bd->est_scratch.alloc(nd);
      if (neu && bd->est_N.n < nN) bd->est_N.alloc(nN);
      if (neu && bd->est_h.n < nh) bd->est_h.alloc(nh);
      if (neu && mask_host && bd->mask.n < (size_t)F.nf) bd->mask.alloc((size_t)F.nf);
    }
    std::vector<double> dt((size_t)B);
    for (int k = 0; k < B; ++k) dt[k] = ts_host[k + 1] - ts_host[k];
    bd->est_dt.upload(dt.data(), dt.size());
    bd->est_table.upload(table.data(), table.size());
    if (neu) {
      hip_check(hipMemcpyAsync(bd->est_h.p, h_host, nh * sizeof(double), hipMemcpyHostToDevice, st), "H2D h");
      if (mask_host) hip_check(hipMemcpyAsync(bd->mask.p, mask_host, (size_t)F.nf, hipMemcpyHostToDevice, st), "H2D mask");
    }
    energy::Args E;
    E.own = L.view(loc->cellptr.p, loc->cellelem.p, loc->x.p);
    E.w = loc->w.p;
    E.p_nodal = p_nodal ? p_nodal->buf.p : nullptr;
    E.p = p;
    E.z = bd->est_table.p;
    E.n = L.n, E.S = S, E.u = u, E.B = B + 1;
    energy::launch_field_flux(st, L.dim, L.k, E, nullptr, sigma->buf.p);
    hip_check(hipGetLastError(), "estimate_steps flux launch");
    estimate::Args A;
    A.own = E.own;
    A.w = E.w, A.p_nodal = E.p_nodal, A.p = p;
    A.sigma = sigma->buf.p;
    A.f = f ? f->buf.p : nullptr;
    A.f_stride = f && f_rows == B && B > 1 ? L.n : 0;
    A.r = r, A.scale = scale, A.own_scale = true;
    A.n = L.n, A.nel = I.nel, A.nlf = I.nlf, A.q = F.q;
    A.inodes = bd->inodes.p, A.iweights = bd->iweights.p, A.inormal = bd->inormal.p, A.nif = I.nif;
    A.bnodes = bd->nodes.p, A.bweights = bd->weights.p, A.bnormal = bd->normal.p;
    A.mask = neu && mask_host ? bd->mask.p : nullptr;
    A.h = neu ? bd->est_h.p : nullptr;
    A.h_stride = neu && h_rows == B && B > 1 ? (long long)F.nf * F.q : 0;
    A.nf = F.nf;
    A.elem_facet = bd->elem_facet.p;
    A.B = B, A.steps = true;
    A.z = bd->est_table.p, A.S = S, A.u = u, A.dt = bd->est_dt.p;
    estimate::launch_estimate(st, L.dim, L.k, A, bd->est_J.p, bd->est_N.p, parts->buf.p, bd->est_scratch.p);
    hip_check(hipGetLastError(), "estimate_steps launch");
    hip_check(hipStreamSynchronize(st), "sync estimate_steps");
    hip_check(hipMemcpy(out_host, bd->est_scratch.p + estimate::results_offset(I.nel, L.block, facets, F.q, B, 2),
                        (size_t)B * 2 * reduce::kCols * sizeof(double), hipMemcpyDeviceToHost), "D2H");
  });
}
int mgb_geo_estimate_steps_host(mgb_geo g, int B, const double* const* z, const double* ts, int S, int u, double p,
                                const double* p_nodal, const double* f, int f_rows, double r, double scale, const double* h, int h_rows,
                                const unsigned char* mask, double* sigma_out, double* parts, double* J, double* N, double* out) {
  return guard([&] {
    need(g && z && ts && parts && out, "geo_estimate_steps_host: null argument");
    need_steps_shape("geo_estimate_steps_host", B, ts, S, u, p, r, scale, f != nullptr, f_rows, h != nullptr, h_rows);
    for (int b = 0; b <= B; ++b) need(z[b] != nullptr, "geo_estimate_steps_host: null field");
    need(g->g.w.size() == (size_t)g->g.n, "geo_estimate_steps_host: the geometry must carry one weight per node");
    if (p_nodal)
      for (int i = 0; i < g->g.n; ++i) need(good_q(p_nodal[i]), "geo_estimate_steps_host: every p_nodal must be finite and >= 1");
    boundary::Facets F;
    boundary::Interior I;
    boundary::build_facet_lists(g->g, &F, &I);
    const int n = g->g.n, dim = F.dim;
    energy::Args E;
    E.own.block = g->g.block;
    E.own.nel = n / g->g.block;
    E.own.x = g->g.x.data();
    E.w = g->g.w.data();
    E.p_nodal = p_nodal;
    E.p = p;
    E.n = n, E.S = S, E.u = u, E.B = 1;
    const size_t nsig = (size_t)n * dim;
    std::vector<double> sigma((size_t)(B + 1) * nsig), Jv((size_t)B * I.nif), Nv((size_t)B * F.nf), dt((size_t)B);
    for (int b = 0; b <= B; ++b) estimate::field_flux_host(dim, F.k, E, z[b], sigma.data() + (size_t)b * nsig);
    for (int k = 0; k < B; ++k) dt[k] = ts[k + 1] - ts[k];
    const bool neu = h != nullptr && F.nf > 0;
    estimate::Args A;
    A.own = E.own;
    A.w = E.w, A.p_nodal = p_nodal, A.p = p;
    A.sigma = sigma.data();
    A.f = f;
    A.f_stride = f && f_rows == B && B > 1 ? n : 0;
    A.r = r, A.scale = scale, A.own_scale = true;
    A.n = n, A.nel = I.nel, A.nlf = I.nlf, A.q = F.q;
    A.inodes = I.nodes.data(), A.iweights = I.weights.data(), A.inormal = I.normal.data(), A.nif = I.nif;
    A.bnodes = F.nodes.data(), A.bweights = F.weights.data(), A.bnormal = F.normal.data();
    A.mask = neu ? mask : nullptr;
    A.h = neu ? h : nullptr;
    A.h_stride = neu && h_rows == B && B > 1 ? (long long)F.nf * F.q : 0;
    A.nf = F.nf;
    A.elem_facet = I.elem_facet.data();
    A.B = B, A.steps = true;
    A.z = z, A.S = S, A.u = u, A.dt = dt.data();
    std::vector<double> pv((size_t)B * I.nel * estimate::kStepParts), res((size_t)B * 2 * reduce::kCols);
    estimate::estimate_host(dim, F.k, A, pv.data(), Jv.data(), Nv.data(), res.data());
    std::copy(pv.begin(), pv.end(), parts);
    if (J) std::copy(Jv.begin(), Jv.end(), J);
    if (N) {
      if (neu) std::copy(Nv.begin(), Nv.end(), N);
      else std::fill(N, N + (size_t)B * F.nf, 0.0);
    }
    if (sigma_out) std::copy(sigma.begin(), sigma.end(), sigma_out);
    std::copy(res.begin(), res.end(), out);
  });
}

// ---- mixed boundary conditions: Dirichlet subspace on part of the boundary (mixed.hpp), Neumann load (boundary.hpp / boundary.hip)
int mgb_geo_dirichlet_on(mgb_geo g, const char* name, const uint8_t* facet_mask) {
  return guard([&] {
    need(g && name, "geo_dirichlet_on: null argument");
    mixed::dirichlet_on(g->g, name, facet_mask);
  });
}
int mgb_geo_boundary_incidence(mgb_geo g, int* nb, int* ninc, int32_t* rows, int32_t* start, int32_t* idx) {
  return guard([&] {
    need(g, "geo_boundary_incidence: null geometry");
    const boundary::Incidence I = boundary::build_incidence(boundary::build_facets(g->g));
    if (nb) *nb = I.nb();
    if (ninc) *ninc = (int)I.idx.size();
    if (rows) std::copy(I.rows.begin(), I.rows.end(), rows);
    if (start) std::copy(I.start.begin(), I.start.end(), start);
    if (idx) std::copy(I.idx.begin(), I.idx.end(), idx);
  });
}
int mgb_geo_boundary_load_host(mgb_geo g, int B, const double* h, const uint8_t* facet_mask, double* out) {
  return guard([&] {
    need(g && h && out, "geo_boundary_load_host: null argument");
    need(B >= 1, "geo_boundary_load_host: B must be >= 1");
    need(g->g.w.size() == (size_t)g->g.n, "geo_boundary_load_host: the geometry must carry one weight per node");
    const boundary::Facets F = boundary::build_facets(g->g);
    const boundary::Incidence I = boundary::build_incidence(F);
    boundary::LoadArgs A;
    A.rows = I.rows.data(), A.start = I.start.data(), A.idx = I.idx.data();
    A.weights = F.weights.data();
    A.mask = facet_mask;
    A.w = g->g.w.data();
    A.nb = I.nb(), A.nf = F.nf, A.q = F.q;
    boundary::boundary_load_host(A, B, h, out);
  });
}
int mgb_boundary_incidence(mgb_boundary b, int* nb, int* ninc, int32_t* rows, int32_t* start, int32_t* idx) {
  return guard([&] {
    need(b, "boundary_incidence: null boundary");
    const boundary::Incidence& I = b->inc;
    if (nb) *nb = I.nb();
    if (ninc) *ninc = (int)I.idx.size();
    if (rows) std::copy(I.rows.begin(), I.rows.end(), rows);
    if (start) std::copy(I.start.begin(), I.start.end(), start);
    if (idx) std::copy(I.idx.begin(), I.idx.end(), idx);
  });
}
int mgb_boundary_load(mgb_boundary bd, int B, const double* h_host, const uint8_t* mask_host, mgb_vec out) {
  return guard([&] {
    need(bd && h_host && out, "boundary_load: null argument");
    mgb_locator_s* loc = bd->loc;
    need(loc->ctx->ctx.world == 1, "boundary_load: sharded contexts are not supported");
    need(out->ctx == loc->ctx, "boundary_load: vector of another context");
    need(B >= 1 && B <= 65535, "boundary_load: B must be in [1, 65535]");
    const boundary::Facets& F = bd->F;
    const int nb = bd->inc.nb();
    need(out->n == (long long)B * nb, "boundary_load: out must hold B x nb values");
    if (nb == 0) return;
    hipStream_t st = loc->ctx->ctx.stream;
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    const size_t nh = (size_t)B * F.nf * F.q;
    if (bd->load_h.n < nh) {      // an earlier launch may still read the old buffer
      hip_check(hipStreamSynchronize(st), "sync boundary_load");
      bd->load_h.alloc(nh);
    }
    hip_check(hipMemcpyAsync(bd->load_h.p, h_host, nh * sizeof(double), hipMemcpyHostToDevice, st), "H2D h");
    if (mask_host) {
      if (bd->mask.n < (size_t)F.nf) {
        hip_check(hipStreamSynchronize(st), "sync boundary_load");
        bd->mask.alloc((size_t)F.nf);
      }
      hip_check(hipMemcpyAsync(bd->mask.p, mask_host, (size_t)F.nf, hipMemcpyHostToDevice, st), "H2D mask");
    }
    boundary::LoadArgs A;
    A.rows = bd->inc_rows.p, A.start = bd->inc_start.p, A.idx = bd->inc_idx.p;
    A.weights = bd->weights.p;
    A.mask = mask_host ? bd->mask.p : nullptr;
    A.w = loc->w.p;
    A.nb = nb, A.nf = F.nf, A.q = F.q;
    boundary::launch_boundary_load(st, A, B, bd->load_h.p, out->buf.p);
    hip_check(hipGetLastError(), "boundary_load launch");
  });
}
int mgb_boundary_load_add(mgb_boundary bd, mgb_vec load, int k, double alpha, mgb_vec y, long long stride, long long offset) {
  return guard([&] {
    need(bd && load && y, "boundary_load_add: null argument");
    mgb_locator_s* loc = bd->loc;
    need(loc->ctx->ctx.world == 1, "boundary_load_add: sharded contexts are not supported");
    need(load->ctx == loc->ctx && y->ctx == loc->ctx, "boundary_load_add: vectors of another context");
    const int nb = bd->inc.nb();
    need(nb == 0 ? load->n == 0 : (load->n > 0 && load->n % nb == 0), "boundary_load_add: load must hold B x nb values");
    if (nb == 0) return;
    need(k >= 0 && k < load->n / nb, "boundary_load_add: field k outside [0, B)");
    need(stride >= 1 && offset >= 0 && offset < stride, "boundary_load_add: needs stride >= 1 and 0 <= offset < stride");
    need((long long)bd->inc.rows.back() * stride + offset < (long long)y->n, "boundary_load_add: a boundary row lies outside y");
    need(std::isfinite(alpha), "boundary_load_add: alpha must be finite");
    hip_check(hipSetDevice(loc->ctx->ctx.device), "hipSetDevice");
    boundary::launch_boundary_load_add(loc->ctx->ctx.stream, nb, bd->inc_rows.p, load->buf.p + (size_t)k * nb, alpha, stride, offset,
                                       y->buf.p);
    hip_check(hipGetLastError(), "boundary_load_add launch");
  });
}
int mgb_amg_add_cost_rows(mgb_amg a, mgb_boundary bd, mgb_vec load, int k, double alpha, int col) {
  return guard([&] {
    need(a && bd && load, "amg_add_cost_rows: null argument");
    need(a->ctx->ctx.world == 1, "amg_add_cost_rows: sharded contexts are not supported");
    need(bd->loc->ctx == a->ctx && load->ctx == a->ctx, "amg_add_cost_rows: objects of another context");
    need(bd->loc->loc.n == a->amg->n(), "amg_add_cost_rows: the boundary belongs to another geometry");
    const int nb = bd->inc.nb();
    need(nb == 0 ? load->n == 0 : (load->n > 0 && load->n % nb == 0), "amg_add_cost_rows: load must hold B x nb values");
    if (nb == 0) return;
    need(k >= 0 && k < load->n / nb, "amg_add_cost_rows: field k outside [0, B)");
    need(col >= 0 && col < a->amg->params().K, "amg_add_cost_rows: column outside [0, K)");
    need(std::isfinite(alpha), "amg_add_cost_rows: alpha must be finite");
    a->amg->add_cost_rows(nb, bd->inc_rows.p, load->buf.p + (size_t)k * nb, alpha, col);
  });
}

// ---- host-only helpers
int mgb_plan_prolongation(mgb_plan fine, mgb_plan coarse, int* rows, int* cols, int* nnz, int32_t* rowptr, int32_t* colidx,
                          double* vals) {
  return guard([&] {
    need(fine && coarse, "null plan");
    Csr P = build_prolongation(fine->plan.R, coarse->plan.R);
    if (rows) *rows = P.rows;
    if (cols) *cols = P.cols;
    if (nnz) *nnz = P.nnz();
    if (rowptr) std::copy(P.rowptr.begin(), P.rowptr.end(), rowptr);
    if (colidx) std::copy(P.colidx.begin(), P.colidx.end(), colidx);
    if (vals) std::copy(P.vals.begin(), P.vals.end(), vals);
  });
}
int mgb_plan_create(mgb_geo g, int S, const char* const* state_vars, int K, const char* const* D, int nq,
                    const int* idx_q, int idx_s, int level, mgb_plan* out) {
  return guard([&] {
    need(g && out, "null argument");
    AmgSpec spec = make_spec(S, state_vars, K, D);
    BarrierParams P = make_params(K, nq, idx_q, idx_s, 1.0);
    Csr Dstack = build_dstack(g->g, spec);
    auto* p = new mgb_plan_s;
    try {
      p->plan = build_level_plan(g->g, spec, Dstack, level, P);
      p->n = g->g.n;
      p->nY = P.nY();
    } catch (...) {
      delete p;
      throw;
    }
    *out = p;
  });
}
int mgb_reduction_scratch_doubles(int n_local, int max_level_unknowns, long long* out) {
  return guard([&] {
    need(out && n_local >= 0 && max_level_unknowns >= 0, "reduction_scratch: bad arguments");
    *out = (long long)reduction_scratch_doubles(n_local, max_level_unknowns);
  });
}
int mgb_plan_destroy(mgb_plan p) {
  return guard([&] { delete p; });
}
int mgb_plan_sizes(mgb_plan p, int* N, int* nnz_lower, int* nnz_T, int* nnz_B) {
  return guard([&] {
    need(p, "null plan");
    if (N) *N = p->plan.N;
    if (nnz_lower) *nnz_lower = p->plan.Apat.nnz();
    if (nnz_T) *nnz_T = p->plan.T.nnz();
    if (nnz_B) *nnz_B = p->plan.B.nnz();
  });
}
int mgb_plan_pattern(mgb_plan p, int32_t* rowptr, int32_t* colidx) {
  return guard([&] {
    need(p, "null plan");
    if (rowptr) std::copy(p->plan.Apat.rowptr.begin(), p->plan.Apat.rowptr.end(), rowptr);
    if (colidx) std::copy(p->plan.Apat.colidx.begin(), p->plan.Apat.colidx.end(), colidx);
  });
}
int mgb_plan_eval_host(mgb_plan p, const double* Y, double* lower_vals) {
  return guard([&] {
    need(p && Y && lower_vals, "null argument");
    // rows of T in chunks on the host threads (each value is one row's dot product: same result as the sequential loop)
    const Csr& T = p->plan.T;
    const int nthr = std::max(1, std::min(MfChol::threads(), T.rows / 4096));
    auto rows = [&](int r0, int r1) {
      for (int r = r0; r < r1; ++r) {
        double acc = 0;
        for (int k = T.rowptr[r]; k < T.rowptr[r + 1]; ++k) acc += T.vals[k] * Y[T.colidx[k]];
        lower_vals[r] = acc;
      }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthr; ++t) th.emplace_back(rows, (int)((long long)T.rows * t / nthr), (int)((long long)T.rows * (t + 1) / nthr));
    rows(0, (int)((long long)T.rows / nthr));
    for (auto& x : th) x.join();
  });
}

int mgb_plan_shard(mgb_plan p, int S, int K, int rank, int world, int block, mgb_plan* out, int* r0, int* r1) {
  return guard([&] {
    need(p && out && r0 && r1, "plan_shard: null argument");
    shard_rows(rank, world, p->n, block, r0, r1);
    auto* q = new mgb_plan_s;
    try {
      q->plan = shard_level_plan(p->plan, p->n, S, K, p->nY, *r0, *r1);
      q->n = *r1 - *r0;
      q->nY = p->nY;
    } catch (...) {
      delete q;
      throw;
    }
    *out = q;
  });
}
int mgb_plan_apply_B_host(mgb_plan p, const double* s, double* Bs) {
  return guard([&] {
    need(p && s && Bs, "null argument");
    spmv_host(p->plan.B, s, Bs);
  });
}
int mgb_plan_apply_BT_host(mgb_plan p, const double* v, double* g) {
  return guard([&] {
    need(p && v && g, "null argument");
    spmv_host(p->plan.BT, v, g);
  });
}

int mgb_plan_chol_bench(mgb_plan p, const double* Y, int dim, int reps, double* seconds_per_factor,
                        double* seconds_per_solve, double* flops, double* front_doubles, double* residual) {
  return guard([&] {
    need(p && Y && reps > 0, "chol_bench: bad arguments");
    const LevelPlan& pl = p->plan;
    std::vector<double> vals(pl.Apat.nnz());
    spmv_host(pl.T, Y, vals.data());
    MfChol ch;
    ch.analyze(pl.Apat, pl.coords.data(), dim);
    auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r)
      if (!ch.factor(vals.data())) throw NumericError("MfChol: bench matrix not SPD");
    const double tf = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / reps;
    const int N = pl.N;
    std::vector<double> xs(N), b(N, 0.0);
    for (int i = 0; i < N; ++i) xs[i] = std::sin(0.37 * i) + 0.1;
    for (int r = 0; r < N; ++r)
      for (int k = pl.Apat.rowptr[r]; k < pl.Apat.rowptr[r + 1]; ++k) {
        const int c = pl.Apat.colidx[k];
        b[r] += vals[k] * xs[c];
        if (c != r) b[c] += vals[k] * xs[r];
      }
    std::vector<double> b0 = b;
    t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r) {
      b = b0;
      ch.solve(b.data());
    }
    const double ts = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / reps;
    double mx = 0, sc = 0;
    for (int i = 0; i < N; ++i) {
      mx = std::max(mx, std::fabs(b[i] - xs[i]));
      sc = std::max(sc, std::fabs(xs[i]));
    }
    if (seconds_per_factor) *seconds_per_factor = tf;
    if (seconds_per_solve) *seconds_per_solve = ts;
    if (flops) *flops = ch.factor_flops();
    if (front_doubles) *front_doubles = (double)ch.front_doubles();
    if (residual) *residual = mx / sc;
  });
}

int mgb_plan_hostchol_create(mgb_plan p, int dim, mgb_hostchol* out) {
  return guard([&] {
    need(p && out && dim >= 1 && dim <= 3, "hostchol_create: bad arguments");
    auto* c = new mgb_hostchol_s;
    try {
      c->ch.analyze(p->plan.Apat, p->plan.coords.data(), dim);
    } catch (...) {
      delete c;
      throw;
    }
    *out = c;
  });
}
int mgb_plan_hostchol_create_ranked(mgb_plan p, int dim, int K, int world, int block, mgb_hostchol* out) {
  return guard([&] {
    need(p && out && dim >= 1 && dim <= 3 && K >= 1 && world >= 1, "hostchol_create_ranked: bad arguments");
    auto* c = new mgb_hostchol_s;
    try {
      const std::vector<unsigned long long> mask = dof_rank_masks(p->plan.B, p->n, K, world, block);
      c->ch.analyze(p->plan.Apat, p->plan.coords.data(), dim, 64, mask.empty() ? nullptr : mask.data(), world);
    } catch (...) {
      delete c;
      throw;
    }
    *out = c;
  });
}
int mgb_hostchol_rank_aligned(mgb_hostchol c, int world, int* aligned, int* top_values) {
  return guard([&] {
    need(c && aligned, "hostchol_rank_aligned: null argument");
    *aligned = c->ch.rank_aligned(world) ? 1 : 0;
    if (top_values) *top_values = *aligned ? (int)c->ch.top_value_indices(c->ch.partition(world)).size() : 0;
  });
}
int mgb_hostchol_destroy(mgb_hostchol c) {
  return guard([&] { delete c; });
}
int mgb_hostchol_info(mgb_hostchol c, int* n, int* threads, double* flops) {
  return guard([&] {
    need(c, "null argument");
    if (n) *n = c->ch.size();
    if (threads) *threads = MfChol::threads();
    if (flops) *flops = c->ch.factor_flops();
  });
}
int mgb_hostchol_factor_solve(mgb_hostchol c, const double* lower_vals, const double* g, double* x) {
  return guard([&] {
    need(c && lower_vals && g && x, "hostchol_factor_solve: null argument");
    if (!c->ch.factor(lower_vals)) throw NumericError("MfChol: matrix is not positive definite");
    if (x != g) std::copy(g, g + c->ch.size(), x);
    c->ch.solve(x);
  });
}

int mgb_hostchol_partition(mgb_hostchol c, int world, int* split_world, int cap, int* nnodes, int* owner) {
  return guard([&] {
    need(c && world >= 1, "hostchol_partition: bad arguments");
    CholPartition part = c->ch.partition(world);
    if (split_world) *split_world = part.world;
    if (nnodes) *nnodes = (int)part.owner.size();
    if (owner) std::copy(part.owner.begin(), part.owner.begin() + std::min<size_t>(cap, part.owner.size()), owner);
  });
}
int mgb_hostchol_factor_solve_dist(mgb_hostchol c, int rank, int world, mgb_allreduce_fn fn, void* user, const double* lower_vals,
                                   const double* g, double* x) {
  return guard([&] {
    need(c && lower_vals && g && x && world >= 1 && rank >= 0 && rank < world && (world == 1 || fn), "hostchol_factor_solve_dist: bad arguments");
    CholPartition part = c->ch.partition(world);
    if (x != g) std::copy(g, g + c->ch.size(), x);
    auto ar = [&](double* ptr, long long count) {
      const int rc = fn(user, ptr, count);
      if (rc != 0) throw InternalError("mgb: allreduce callback failed with code " + std::to_string(rc));
    };
    if (!c->ch.factor_solve_dist(lower_vals, x, part, rank, ar)) throw NumericError("MfChol: matrix is not positive definite");
  });
}

int mgb_hostchol_factor_solve_dist_local(mgb_hostchol c, int rank, int world, mgb_allreduce_fn fn, void* user,
                                         const double* local_lower_vals, const double* g, double* x) {
  return guard([&] {
    need(c && local_lower_vals && g && x && world >= 2 && rank >= 0 && rank < world && fn, "hostchol_factor_solve_dist_local: bad arguments");
    CholPartition part = c->ch.partition(world);
    if (x != g) std::copy(g, g + c->ch.size(), x);
    auto ar = [&](double* ptr, long long count) {
      const int rc = fn(user, ptr, count);
      if (rc != 0) throw InternalError("mgb: allreduce callback failed with code " + std::to_string(rc));
    };
    if (!c->ch.factor_solve_dist(local_lower_vals, x, part, rank, ar, /*vals_local=*/true))
      throw NumericError("MfChol: matrix is not positive definite");
  });
}

int mgb_plan_chol_tree(mgb_plan p, int dim, int cap, int* nnodes, int* ns, int* nf, int* parent) {
  return guard([&] {
    need(p && nnodes, "chol_tree: bad arguments");
    MfChol ch;
    ch.analyze(p->plan.Apat, p->plan.coords.data(), dim);
    std::vector<int> a, b, c;
    ch.tree(a, b, c);
    *nnodes = (int)a.size();
    const int m = std::min<int>(cap, (int)a.size());
    if (ns) std::copy(a.begin(), a.begin() + m, ns);
    if (nf) std::copy(b.begin(), b.begin() + m, nf);
    if (parent) std::copy(c.begin(), c.begin() + m, parent);
  });
}

int mgb_plan_chol_bwd_fused(mgb_plan p, int dim, int cut, int top_nf, int threads, int* info, int cap_wg, int* wg, int cap_bdry,
                            int* bdry, int* slots, int cap_nodes, int* bofs, int* first) {
  return guard([&] {
    need(p && info, "chol_bwd_fused: bad arguments");
    MfChol ch;
    ch.analyze(p->plan.Apat, p->plan.coords.data(), dim);
    const CholTree T = ch.view();
    FusedKnobs kn = fused_knobs(GpuChol::knobs());
    kn.cut = cut;
    kn.top_nf = top_nf;
    kn.threads = threads;
    const FusedPlan P = plan_bwd_fused(T, kn);
    std::vector<int> bd;
    for (const std::vector<int>* l : T.bdry) bd.insert(bd.end(), l->begin(), l->end());
    const int v[12] = {P.h_top, P.h_cut, P.nwg, P.wstride, P.max_levels, P.xs_cap, P.red_cap, P.sl_cap, (int)P.lds_bytes,
                       (int)bd.size(), T.size(), T.nheights};
    std::copy(v, v + 12, info);
    if (wg) std::copy(P.wg.begin(), P.wg.begin() + std::min<size_t>(cap_wg, P.wg.size()), wg);
    const size_t mb = std::min<size_t>(cap_bdry, bd.size()), mn = std::min<size_t>(cap_nodes, T.size());
    if (bdry) std::copy(bd.begin(), bd.begin() + mb, bdry);
    if (slots) std::copy(P.slots.begin(), P.slots.begin() + mb, slots);
    if (bofs) std::copy(T.bofs.begin(), T.bofs.begin() + mn, bofs);
    if (first) std::copy(T.first.begin(), T.first.begin() + mn, first);
  });
}

int mgb_plan_chol_premap(mgb_plan p, int dim, int leaf, int single, int mode, int tiles, long long* info, int cap_nodes, int* height,
                         int* producer, long long* soff, long long* eoff, int* fofs, int* iofs, int cap_heights, int* hkind, int* hwg,
                         int* hconsumer, int cap_fwd, int* fwd, int cap_pinv, int* pinv) {
  return guard([&] {
    need(p && info, "chol_premap: bad arguments");
    MfChol ch;
    ch.analyze(p->plan.Apat, p->plan.coords.data(), dim);
    const CholTree T = ch.view();
    CholKnobs kn = GpuChol::knobs();
    kn.leaf = leaf != 0;
    kn.single = single != 0;
    kn.premap = mode;
    kn.premap_tiles = tiles;
    const PremapPlan P = plan_premap(T, kn);
    const long long v[5] = {(long long)T.size(), T.nheights, (long long)P.fwd.size(), (long long)P.pinv.size(), P.slab_doubles};
    std::copy(v, v + 5, info);
    const size_t mn = std::min<size_t>(std::max(cap_nodes, 0), T.size()), mh = std::min<size_t>(std::max(cap_heights, 0), T.nheights);
    if (height) std::copy(T.height.begin(), T.height.begin() + mn, height);
    if (producer) std::copy(P.producer.begin(), P.producer.begin() + mn, producer);
    if (soff) std::copy(P.soff.begin(), P.soff.begin() + 2 * mn, soff);
    if (eoff) std::copy(P.eoff.begin(), P.eoff.begin() + mn, eoff);
    if (fofs) std::copy(P.fofs.begin(), P.fofs.begin() + mn, fofs);
    if (iofs) std::copy(P.iofs.begin(), P.iofs.begin() + mn, iofs);
    if (hkind) std::copy(P.hkind.begin(), P.hkind.begin() + mh, hkind);
    if (hwg) std::copy(P.hwg.begin(), P.hwg.begin() + mh, hwg);
    if (hconsumer) std::copy(P.hconsumer.begin(), P.hconsumer.begin() + mh, hconsumer);
    if (fwd) std::copy(P.fwd.begin(), P.fwd.begin() + std::min<size_t>(std::max(cap_fwd, 0), P.fwd.size()), fwd);
    if (pinv) std::copy(P.pinv.begin(), P.pinv.begin() + std::min<size_t>(std::max(cap_pinv, 0), P.pinv.size()), pinv);
  });
}

int mgb_plan_chol_schedule(mgb_plan p, int dim, const int* knobs, int world, int rank, int* info, int cap_launch, int* launch,
                           int cap_lists, int* lists, int cap_starts, int* starts, int cap_tiles, int* tiles, int cap_singles,
                           int* singles, int cap_rects, int* rects, int cap_asm, int* apos, int* asrc) {
  return guard([&] {
    need(p && info && world >= 1 && rank >= 0 && rank < world, "chol_schedule: bad arguments");
    MfChol ch;
    ch.analyze(p->plan.Apat, p->plan.coords.data(), dim);
    CholKnobs kn = GpuChol::knobs();
    if (knobs) {
      const int* k = knobs;
      kn = CholKnobs{k[0] != 0, k[1] != 0, k[2] != 0, k[3] != 0, k[4] != 0, k[5] != 0, k[6] != 0, k[7], k[8], k[9], k[10] != 0, k[11],
                     k[12], k[13], k[14], k[15]};
    }
    const CholPartition part = world > 1 ? ch.partition(world) : CholPartition();
    const ChainPlan P = plan_chain(ch.view(), part, rank, kn);
    const int v[10] = {(int)P.chain.size(), P.own_bwd, P.top_fwd, (int)P.lists.size(), (int)P.starts.size(), (int)P.tiles.size(),
                       (int)P.singles.size(), (int)P.rects.size(), (int)P.asrc.size(), part.world};
    std::copy(v, v + 10, info);
    const auto upto = [](int cap, size_t n) { return std::min<size_t>(std::max(cap, 0), n); };
    if (launch)
      for (size_t i = 0; i < upto(cap_launch, P.chain.size()); ++i) {
        const Launch& L = P.chain[i];
        const int r[10] = {(int)L.kind, L.ofs, L.cnt, L.block, (int)L.lds, L.p, L.npiv, L.rect ? 1 : 0, L.premap ? 1 : 0, L.nproducers};
        std::copy(r, r + 10, launch + 10 * i);
      }
    if (lists) std::copy(P.lists.begin(), P.lists.begin() + upto(cap_lists, P.lists.size()), lists);
    if (starts)
      for (size_t i = 0; i < upto(cap_starts, P.starts.size()); ++i) {
        const StartJob& j = P.starts[i];
        const int r[5] = {j.node, j.chunk, j.rb, j.a0, j.a1};
        std::copy(r, r + 5, starts + 5 * i);
      }
    if (tiles)
      for (size_t i = 0; i < upto(cap_tiles, P.tiles.size()); ++i) {
        const int r[3] = {P.tiles[i].pad, P.tiles[i].ti, P.tiles[i].tj};
        std::copy(r, r + 3, tiles + 3 * i);
      }
    if (singles)
      for (size_t i = 0; i < upto(cap_singles, P.singles.size()); ++i) {
        const SingleTile& u = P.singles[i];
        // a single tile names its front by offset: fronts are laid out in node order
        const auto g = std::lower_bound(P.nodes.begin(), P.nodes.end(), u.off, [](const GNode& a, long long o) { return a.off < o; });
        const int r[3] = {(int)(g - P.nodes.begin()), u.ti, u.tj};
        std::copy(r, r + 3, singles + 3 * i);
      }
    if (rects)
      for (size_t i = 0; i < upto(cap_rects, P.rects.size()); ++i) {
        rects[2 * i] = P.rects[i].node;
        rects[2 * i + 1] = P.rects[i].chunk;
      }
    if (apos) std::copy(P.apos.begin(), P.apos.begin() + upto(cap_asm, P.apos.size()), apos);
    if (asrc) std::copy(P.asrc.begin(), P.asrc.begin() + upto(cap_asm, P.asrc.size()), asrc);
  });
}

int mgb_chol_selftest(int nx, int ny, double* max_residual, double* flops, double* seconds) {
  return guard([&] {
    need(nx > 0 && ny > 0, "selftest: bad size");
    const int N = nx * ny;
    std::vector<Triplet> t;
    std::vector<double> coords((size_t)N * 2);
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const int r = j * nx + i;
        coords[2 * r] = i;
        coords[2 * r + 1] = j;
        t.push_back({r, r, 6.0 + 1e-3 * ((r * 7919) % 13)});
        if (i > 0) t.push_back({r, r - 1, -1.0});
        if (j > 0) t.push_back({r, r - nx, -1.0});
        if (i > 0 && j > 0) t.push_back({r, r - nx - 1, -0.5});
      }
    Csr Lo = from_triplets(N, N, t);
    MfChol ch;
    ch.analyze(Lo, coords.data(), 2);
    const auto t0 = std::chrono::steady_clock::now();
    if (!ch.factor(Lo.vals.data())) throw NumericError("MfChol: selftest matrix not SPD");
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::vector<double> xs(N), b(N, 0.0);
    for (int i = 0; i < N; ++i) xs[i] = std::sin(0.37 * i) + 0.1;
    for (int r = 0; r < N; ++r)
      for (int k = Lo.rowptr[r]; k < Lo.rowptr[r + 1]; ++k) {
        const int c = Lo.colidx[k];
        b[r] += Lo.vals[k] * xs[c];
        if (c != r) b[c] += Lo.vals[k] * xs[r];
      }
    ch.solve(b.data());
    double mx = 0;
    for (int i = 0; i < N; ++i) mx = std::max(mx, std::fabs(b[i] - xs[i]));
    if (max_residual) *max_residual = mx;
    if (flops) *flops = ch.factor_flops();
    if (seconds) *seconds = sec;
  });
}

int mgb_reduce_selftest(mgb_ctx ctx, int rows, int nwg, const double* partials_host, double* out_host) {
  return guard([&] {
    need(ctx && partials_host && out_host, "reduce_selftest: null argument");
    need(rows >= 1 && nwg >= 1, "reduce_selftest: rows and nwg must be >= 1");
    hipStream_t st = ctx->ctx.stream;
    hip_check(hipSetDevice(ctx->ctx.device), "hipSetDevice");
    const size_t np = (size_t)rows * nwg * reduce::kCols, no = (size_t)rows * reduce::kCols;
    DevBuf<double> buf;
    buf.alloc(np + no);
    buf.upload(partials_host, np);
    reduce::launch_finish(st, rows, buf.p, nwg, (size_t)nwg * reduce::kCols, reduce::kCols, buf.p + np);
    hip_check(hipGetLastError(), "reduce_selftest launch");
    hip_check(hipStreamSynchronize(st), "sync reduce_selftest");
    hip_check(hipMemcpy(out_host, buf.p + np, no * sizeof(double), hipMemcpyDeviceToHost), "D2H");
  });
}

}  // extern "C"
