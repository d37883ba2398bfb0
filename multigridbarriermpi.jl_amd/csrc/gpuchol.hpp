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

#include "bwd_fused.hpp"
#include "chol_premap.hpp"
#include "mfchol.hpp"

namespace mgb {

class KernelTimer;   // amg.hpp: optional HIP-event bracketing of individual launches
struct Ctx;          // amg.hpp: device, stream and (sharded jobs) the allreduce callback

struct RootXchg {     // one subtree root of a split factorisation: where its Schur complement lives and travels
  long long off;      // front offset
  long long xoff;     // offset of its packed lower triangle (+ right-hand-side row) in the exchange buffer
  int ld, ns, nb;     // leading dimension nf + 1, own columns, boundary size
  int owned;          // 1 on the rank that factors this subtree
};

struct GNode {
  long long off;      // offset of the (nf+1) x (nf+1) column-major front
  long long loff;     // offset of this node's 32x32 pivot blocks of L (one per panel)
  int nf, ns, first, parent;
  int bofs;           // offset of this node's bdry / ea lists (nb entries each)
  int child[2];       // -1 if absent
  int iofs;           // offset of the two (nf+1)-long inverse extend-add maps (-1: leaf)
  int a0, a1;         // range of this node's entries in the assembly list
  int pld;            // pre-mapped store (chol_premap.hpp): the parent's leading dimension,
  int fofs;           // ... where this node's forward map begins,
  long long eoff;     // ... and the offset of its slab in the parent (-1: the Schur complement stays in the front)
};

struct StartJob {     // one workgroup of front_start: 32 columns x 256 rows (counted from the chunk's first row) of one front,
                      // with everything of the node and its children inline (no dependent descriptor loads)
  long long off, loff;      // front, first pivot block
  long long boff[2];        // first boundary entry of each child's front (own front offset if absent)
  int cld[2];               // child leading dimensions (0 = no child)
  int nf, ns, iofs, first;
  int node, chunk, rb;
  int a0, a1;         // range of the (column-sorted) assembly list
  long long soff[2];  // pre-mapped consumer launches: the front's contribution slab per child slot (unused slot: any valid offset)
};

struct StepTile {     // one workgroup of front_step: a 64x64 tile of the trailing matrix of one front
  long long off;      // front offset
  long long loff;     // offset of THIS panel's pivot block
  int nf, ns;
  short ti, tj;
  int pad;            // node index
};

struct SingleTile {   // one workgroup of front_single: a tile of a single-panel front, with everything it needs inline
  long long off, loff;      // front, pivot block
  long long boff[2];        // first boundary entry of each child's front (own front offset if absent)
  int cld[2];               // child leading dimensions (0 = no child)
  int nf, ns, iofs, a0, a1, first;
  short ti, tj;
  int pld, fofs;      // pre-mapped store: the parent's leading dimension, where the front's forward map begins
  long long eoff;     // ... and the offset of its slab in the parent (-1: the Schur complement stays in the front)
  long long soff[2];  // pre-mapped consumer launches: the front's contribution slab per child slot
};

struct RectJob {      // one workgroup of backward_rect: 64 own columns of one front
  int node, chunk;
};

// The chain's environment knobs (all optional), read once per process
struct CholKnobs {
  bool graph;          // MGB_CHOL_GRAPH=0: plain launches instead of hipGraph replay
  bool prof;           // MGB_CHOL_PROF set: phase stamps of every launch, printed after each plain-launch unsplit chain
  bool leaf;           // MGB_CHOL_LEAF=0: no front_leaf heights
  bool single;         // MGB_CHOL_SINGLE=0: no front_single heights
  bool step2;          // MGB_CHOL_STEP2=0: one panel per launch everywhere (the scheme before front_step2)
  bool wide;           // MGB_CHOL_WIDE=0: one panel per launch beyond the fused kernel's tile count (no panel + update pairs)
  bool start_pivot;    // MGB_CHOL_START_PIVOT=0: the first pivot block is factored by the assembling workgroup
  int step2_tiles;     // MGB_CHOL_STEP2_TILES (224): largest launch, in tiles, that runs two panels fused
  int dense_tiles;     // MGB_CHOL_DENSE_TILES (512): single-panel launches above this many tiles run three tiles per CU
  int bwd_split_nf;    // MGB_BWD_SPLIT_NF (192): front size above which the backward sweep of a height has a backward_rect launch
  bool bwd_fused;      // MGB_CHOL_BWD_FUSED=0: the backward sweep as one or two launches per height (no backward_fused launch)
  int bwd_cut;         // MGB_CHOL_BWD_CUT (2): height of the subtrees the fused backward launch gives one workgroup each (raised by
                       // up to two heights until they are at most 256, one per CU; trees that need more keep the per-height launches)
  int bwd_fused_nf;    // MGB_CHOL_BWD_FUSED_NF (384): heights with a larger front keep their own backward launches; 0: no limit
  int bwd_fused_threads;  // MGB_CHOL_BWD_FUSED_THREADS (512): workgroup size of the fused backward launch (a power of two, 64 .. 512)
  int premap;          // MGB_CHOL_PREMAP (1): children store their Schur complements in parent order (chol_premap.hpp) for
                       // 1: front_single consumers, 2: front_start consumers too; 0: every launch gathers through the index maps
  int premap_tiles;    // MGB_CHOL_PREMAP_TILES (400): largest launch, in workgroups, that reads pre-mapped slabs
};

class GpuChol {
 public:
  GpuChol() = default;
  GpuChol(const GpuChol&) = delete;
  GpuChol& operator=(const GpuChol&) = delete;
  ~GpuChol();
  static const CholKnobs& knobs();
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
  double exchange_doubles() const { return (double)xchg_doubles_ + ntop_vals_ + n_ + 1; }
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
  static PremapKnobs premap_knobs();      // the rule's knobs as this process reads them
  // per unknown (original ordering, nullable outputs): its tree node (postorder) and its column among that node's own columns
  static void unknown_columns(const MfChol& sym, int* node, int* col);

 private:
  template <class T>
  T* upload(const std::vector<T>& v);
  struct Jobs;
  int schedule(const std::vector<std::vector<int>>& heights, const std::vector<GNode>& nodes,
               const std::vector<std::vector<StartJob>>& sjobs, const MfChol& sym, Jobs& jobs);
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
  int n_ = 0, nnodes_ = 0, nheights_ = 0, max_nf_ = 0;
  long long total_front_ = 0;
  double flops_ = 0;
  // device
  double* d_fronts_ = nullptr;
  double* d_rect_ = nullptr;      // L21' x_bdry of the split backward sweep (n entries, new ordering)
  double* d_linv_ = nullptr;      // 32x32 diagonal (pivot) blocks of L
  double* d_slabs_ = nullptr;     // pre-mapped child contributions: zeroed once by build(), written by the producers only
  int* d_fwd_ = nullptr;          // ... the forward maps (child boundary row -> parent front row)
  PremapPlan premap_;             // ... their host tables (all flags off for split factorisations)
  const std::vector<std::vector<int>>* premap_heights_ = nullptr;     // (during build) the height lists that plan covers
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
  const std::vector<std::vector<int>>* fused_heights_ = nullptr;      // (during build) the height lists the plan covers
  FusedPlan fused_;               // fused backward sweep (unsplit factorisations): host tables, empty where it is off
  int* d_fused_wg_ = nullptr;     // ... its workgroup records
  int* d_fused_slots_ = nullptr;  // ... and the LDS slot of every boundary entry (parallel to d_bdry_)
  // host schedule: every dispatch of the chain, decided once by build()
  enum class Kind : unsigned char {
    Leaf, Single, SingleNarrow, SingleDense, SingleDenseNarrow, Start, Step, Step2, Panel2, Update2, BwdRect, Bwd256, Bwd1024, BwdFused
  };
  struct Launch {
    Kind kind;
    int ofs, cnt;       // job range, one workgroup per job, in lists (Leaf, Bwd*), singles (Single*), starts (Start),
                        // tiles (Step, Step2, Panel2, Update2), rects (BwdRect) or the fused sweep's workgroup records (BwdFused)
    int block;          // threads per workgroup
    size_t lds;         // dynamic LDS bytes
    int p, npiv;        // first panel, leading pivot workgroups (step kinds)
    bool rect;          // Bwd*: the rectangular part ran in the BwdRect launch before
    int timer;          // KernelTimer class
    double bytes;       // algorithmic bytes
    bool premap = false;     // Single*, Start: reads the contribution slabs (no gather)
    int nproducers = 0;      // Leaf, Single*: fronts of the launch that store into a slab
  };
  // own forward | own backward | (split) top forward | top backward, in launch order; a launch's position is its profile slot.
  // Own: this rank's subtree when split, else everything; top: the replicated separators above the subtrees.
  std::vector<Launch> chain_;
  int own_bwd_ = 0, top_fwd_ = 0;      // where own backward and the top begin
  std::vector<void*> allocs_;
};

}  // namespace mgb
