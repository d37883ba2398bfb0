// Device-resident multifrontal Cholesky for the Newton systems (R'HR) n = g.
//
// Replaces, on the GPU, what the reference does with `A \ b` -> MUMPS on every Newton step
// (test/test_instrumented_solve.jl:25-28,99; tools/profile_ops.jl:117-126).  The sparsity pattern of
// R_l'HR_l is fixed per level, so the host analysis of MfChol (nested-dissection tree, front index lists,
// assembly / extend-add maps) is done once and uploaded; each Newton step then runs, entirely on the
// context stream with no host round trip, ONE dependent chain of launches:
//
//   for each tree height (leaves first):
//     front_start : zero + assemble the front columns, pull both children's Schur complements (fixed
//                   order), factor the first 32x32 pivot block
//     front_step p: (one launch per 32-wide panel) every 64x64 tile of the trailing matrix re-derives the
//                   panel rows it needs (L = A * L11^-T), applies the rank-32 update, and the tile that
//                   owns the next pivot block factors it, so a panel costs one launch
//   backward sweep  L' x = u: ONE launch (backward_fused_kernel: one workgroup per subtree of a cut of the tree solves its
//     own path from the top and then its subtree, no synchronisation between workgroups; bwd_fused.hpp); heights whose fronts
//     are too large to repeat, and split factorisations, run one or two launches per height (root first) instead
//
// The right-hand side rides along as an extra row of every front (Cholesky of [A b; b' *]), so the
// forward sweep L u = b happens inside the factorisation at no extra launch.  Fronts are stored as
// (nf+1) x (nf+1) column-major squares: the lower triangle holds the working matrix, the upper triangle
// receives the finished rows of L (L[i][k] at row k, column i) -- which is the layout the backward sweep
// wants (unit-stride over k) and makes the panel write race-free.  Everything is gather/pull form:
// no atomics, bitwise reproducible.  Every 32x32 diagonal block of L is kept (row-major, reciprocal
// diagonal) in a side buffer for the substitutions of the panel TRSM and of the backward sweep.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "chol_plan.hpp"

namespace mgb {

class KernelTimer;   // amg.hpp: optional HIP-event bracketing of individual launches
struct Ctx;          // amg.hpp: device, stream and (sharded jobs) the allreduce callback

class GpuChol {
 public:
  GpuChol() = default;
  GpuChol(const GpuChol&) = delete;
  GpuChol& operator=(const GpuChol&) = delete;
  ~GpuChol();
  static const CholKnobs& knobs();
  using Kind = mgb::Kind;      // the launch kinds (chol_plan.hpp): the codes schedule_info reports
  // ctx (nullable): on a sharded context (ctx->world a power of two the tree can be split into) the factorisation is
  // split by subtrees -- this rank factors its subtree, the subtree roots' Schur complements (with their right-hand-side
  // rows) are summed over the ranks (one rank contributes each), every rank factors the replicated top and sweeps back
  // through the top and its own subtree, and a second allreduce assembles x and the pivot flag.  Bitwise the same
  // arithmetic as the unsplit factorisation.
  void build(const MfChol& sym, Ctx* ctx = nullptr);
  bool split() const { return part_.split(); }
  // split AND the tree's top follows the row partition (MfChol::rank_aligned): factor_solve takes THIS rank's row-block
  // contributions to the matrix entries -- the caller does not sum the values over the ranks; the entries of the top
  // nodes ride in the Schur-complement collective and their sums are written back into d_vals.
  bool values_local() const { return vals_local_; }
  // doubles one Newton system exchanges inside factor_solve: the subtree roots' packed Schur complements, then either the matrix
  // entries among top unknowns that ride behind them (values_local: the Newton loop solves with x_local, no collective for x) or
  // x and the pivot flag (n + 1)
  double exchange_doubles() const { return (double)xchg_doubles_ + (vals_local_ ? ntop_vals_ : n_ + 1); }
  // d_x = A^{-1} d_b: d_vals = device lower-triangle values in the pattern order given to MfChol::analyze,
  // d_b / d_x device vectors in the ORIGINAL ordering (may alias).
  // flag_armed: the caller guarantees the pivot flag is zero (it re-arms it itself behind the chain): no memset launch
  // d_vals is written only when values_local() (top entries <- their sums over the ranks)
  // values_summed: d_vals already holds the sums over the ranks on every rank (a matrix handed in from outside)
  // x_local (split + values_local only): d_b holds this rank's own-interior entries and the SUMMED entries of the top unknowns
  // (zeros / anything elsewhere); d_x comes back valid on the same set and zero elsewhere, and the pivot flag stays on the device
  // unreduced -- no collective for x: the caller folds the flag into its scalar reduction (Amg: owner-local Newton vectors)
  void factor_solve(hipStream_t st, double* d_vals, const double* d_b, double* d_x, KernelTimer* timer = nullptr,
                    bool flag_armed = false, bool values_summed = false, bool x_local = false);
  // per unknown (original ordering) of a split factorisation: 0 = interior of another rank's subtree, 1 = of this rank's, 2 = top
  const int* unknown_kind() const { return d_kind_orig_; }
  const int* top_unknowns() const { return d_top_unk_; }      // original indices of the top (separator) unknowns
  int ntop_unknowns() const { return ntop_unk_; }
  // the bare launch chain (no flag re-arm, no graph of its own): for callers that capture it into a larger graph together
  // with what follows the solve.  Not for split factorisations (their collectives cannot be captured).
  void enqueue_chain(hipStream_t st, const double* d_vals, const double* d_b, double* d_x);
  int* fail_flag() const { return d_fail_; }   // device int: nonzero after factor_solve() if a pivot was not positive
  int size() const { return n_; }
  double front_bytes() const { return (double)total_front_ * 8; }
  double factor_flops() const { return flops_; }
  int launches_per_solve() const { return (int)chain_.size(); }
  // the chain in launch order (nullable outputs): *nlaunch launches, the Kind code (enum order) and the workgroup count of
  // the first min(cap, *nlaunch) of them.  Read-only.
  void schedule_info(int cap, int* nlaunch, int* kind, int* workgroups) const;
  // pre-mapped child contributions, per launch of the first min(cap, launches) (nullable outputs): 1 if the launch reads
  // its fronts' contribution slabs instead of gathering, and how many of its fronts store their Schur complement into one
  void premap_info(int cap, int* consumer, int* producers) const;
  double slab_bytes() const { return (double)premap_.slab_doubles * 8; }
  // per unknown (original ordering, nullable outputs): its tree node (postorder) and its column among that node's own columns
  static void unknown_columns(const MfChol& sym, int* node, int* col);

 private:
  template <class T>
  T* upload(const std::vector<T>& v);
  void run(hipStream_t st, int begin, int end, const double* d_vals, const double* d_b, double* d_x, KernelTimer* tm);
  void enqueue(hipStream_t st, const double* d_vals, const double* d_b, double* d_x, KernelTimer* tm);
  void print_stamps(hipStream_t st);
  void reset_stamps();
  void factor_solve_split(hipStream_t st, double* d_vals, const double* d_b, double* d_x, KernelTimer* tm, bool values_summed,
                          bool x_local);
  int* d_kind_orig_ = nullptr;
  int* d_top_unk_ = nullptr;
  int ntop_unk_ = 0;
  Ctx* ctx_ = nullptr;
  CholPartition part_;
  long long xchg_doubles_ = 0;
  RootXchg* d_roots_ = nullptr;
  int nroots_ = 0, max_root_nb_ = 0;
  double* d_xchg_ = nullptr;      // Schur exchange buffer (+ ntop_vals_ matrix entries of the top nodes behind it)
  bool vals_local_ = false;
  int ntop_vals_ = 0;
  int* d_top_idx_ = nullptr;      // indices into d_vals of the entries assembled into the top nodes
  double* d_xsol_ = nullptr;      // n + 1: masked solution + pivot flag
  int* d_own_orig_ = nullptr;     // per unknown (original ordering): 1 if this rank contributes it to the assembled x
  struct GraphEntry {      // captured launch chain for one (values, rhs, solution) pointer triple
    const double* vals;
    const double* b;
    double* x;
    hipGraphExec_t exec;
  };
  std::vector<GraphEntry> graphs_;
  int n_ = 0;
  long long total_front_ = 0;
  double flops_ = 0;
  // device
  double* d_fronts_ = nullptr;
  double* d_rect_ = nullptr;      // L21' x_bdry of the split backward sweep (n entries, new ordering)
  double* d_linv_ = nullptr;      // 32x32 diagonal (pivot) blocks of L
  double* d_slabs_ = nullptr;     // pre-mapped child contributions: zeroed once by build(), written by the producers only
  int* d_fwd_ = nullptr;          // ... the forward maps (child boundary row -> parent front row)
  PremapPlan premap_;             // ... their host tables (all flags off for split factorisations)
  double* d_y_ = nullptr;         // solution in the new ordering
  int* d_fail_ = nullptr;
  long long* d_prof_ = nullptr;   // MGB_CHOL_PROF=1: phase stamps of workgroup 0 of every launch but backward_rect
  [[maybe_unused]] long long* d_wgprof_ = nullptr; // (-DMGB_PROF_PER_WG builds) start / end of every workgroup of every stamped launch
  GNode* d_nodes_ = nullptr;
  int* d_perm_ = nullptr;
  int* d_bdry_ = nullptr;
  int* d_pinv_ = nullptr;        // per parent, per child slot: parent front row -> child boundary row
  int* d_asm_src_ = nullptr;
  int* d_asm_pos_ = nullptr;
  int* d_lists_ = nullptr;        // node lists per height
  GNode* d_hnodes_ = nullptr;     // ... and the node descriptors themselves in that order (leaf / backward launches)
  GNode* d_rnodes_ = nullptr;     // node descriptor per backward_rect job
  StartJob* d_start_ = nullptr;
  StepTile* d_tiles_ = nullptr;
  SingleTile* d_singles_ = nullptr;
  RectJob* d_rectjobs_ = nullptr;
  FusedPlan fused_;               // fused backward sweep (unsplit factorisations): host tables, empty where it is off
  int* d_fused_wg_ = nullptr;     // ... its workgroup records
  int* d_fused_slots_ = nullptr;  // ... and the LDS slot of every boundary entry (parallel to d_bdry_)
  // host schedule: every dispatch of the chain, decided once by plan_chain (chol_plan.hpp)
  // own forward | own backward | (split) top forward | top backward, in launch order; a launch's position is its profile slot.
  // Own: this rank's subtree when split, else everything; top: the replicated separators above the subtrees.
  std::vector<Launch> chain_;
  int own_bwd_ = 0, top_fwd_ = 0;      // where own backward and the top begin
  std::vector<void*> allocs_;
};

}  // namespace mgb
