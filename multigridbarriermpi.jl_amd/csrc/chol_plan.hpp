// Host plan of the device Cholesky chain (gpuchol.hpp): the front layout, every job and every launch, decided once per
// symbolic analysis by plan_chain().  Host-only: no HIP header, built with the host compiler, testable without a GPU
// (mgb_plan_chol_schedule).  The chain's constants and the plain descriptors the kernels read are stated here once;
// the three planners (plan_chain and, called by it, plan_premap and plan_bwd_fused) share one view of the tree, CholTree.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "bwd_fused.hpp"
#include "chol_premap.hpp"
#include "mfchol.hpp"

namespace mgb {

constexpr int PB = 32;       // panel width
constexpr int LP = PB + 1;   // padded LDS row length
constexpr int TS = 64;       // trailing-update tile
constexpr int TB = 256;      // threads per workgroup (factorisation kernels)
constexpr int RT = 1024;     // threads per workgroup (backward_rect)
// dynamic LDS of the two-panel kernels (front_step2_body): the fused launch, the panel launch and the update launch
constexpr int kStep2Lds = (2 * PB * PB + 3 * PB * LP + 2 * 2 * PB * (TS + 8)) * (int)sizeof(double);
constexpr int kPanel2Lds = (2 * PB * PB + 3 * PB * LP + 2 * PB * (TS + 8)) * (int)sizeof(double);
constexpr int kUpdate2Lds = (2 * 2 * PB * (TS + 8)) * (int)sizeof(double);

// The symbolic tree as MfChol::view() hands it out, in postorder (children before parents); the pointers stay valid as
// long as the MfChol.  Heights and the front layout are computed by layout() and nowhere else.
struct CholTree {
  int n = 0;                                // unknowns
  double flops = 0;
  const std::vector<int>* perm = nullptr;   // perm[new] = old
  std::vector<int> ns, nf, first, parent;   // own columns, front size, first own unknown (new ordering), parent (-1: root)
  std::vector<int> child[2];                // the two child slots (-1: absent)
  std::vector<const std::vector<int>*> bdry, ea, a_idx, a_pos;      // boundary list (new indices, ascending), position of each
                                            // boundary entry in the parent's front, matrix entries (index into the values,
                                            // destination in the nf x nf front)
  std::vector<int> height;                  // leaves 0
  std::vector<long long> off, loff;         // the (nf+1) x (nf+1) column-major front, its 32x32 pivot blocks of L (one per panel)
  std::vector<int> bofs;                    // offset of the node's boundary list in the concatenated one
  int nheights = 0, max_nf = 0, bdry_total = 0;
  long long front_doubles = 0, linv_doubles = 0;
  int size() const { return (int)ns.size(); }
  void layout();                            // fills height .. linv_doubles from the members above them
};

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

// The chain's knobs with their defaults.  GpuChol::knobs() reads them from the environment once per process; host callers
// of plan_chain pass their own.
struct CholKnobs {
  bool graph = true;          // MGB_CHOL_GRAPH=0: plain launches instead of hipGraph replay
  bool prof = false;          // MGB_CHOL_PROF set: phase stamps of every launch, printed after each plain-launch unsplit chain
  bool leaf = true;           // MGB_CHOL_LEAF=0: no front_leaf heights
  bool single = true;         // MGB_CHOL_SINGLE=0: no front_single heights
  bool step2 = true;          // MGB_CHOL_STEP2=0: one panel per launch everywhere (the scheme before front_step2)
  bool wide = true;           // MGB_CHOL_WIDE=0: one panel per launch beyond the fused kernel's tile count (no panel + update pairs)
  bool start_pivot = true;    // MGB_CHOL_START_PIVOT=0: the first pivot block is factored by the assembling workgroup
  int step2_tiles = 224;      // MGB_CHOL_STEP2_TILES: largest launch, in tiles, that runs two panels fused
  int dense_tiles = 512;      // MGB_CHOL_DENSE_TILES: single-panel launches above this many tiles (what two tiles per CU hold at
                              // once) run three tiles per CU
  int bwd_split_nf = 192;     // MGB_BWD_SPLIT_NF: front size above which the backward sweep of a height has a backward_rect launch
  bool bwd_fused = true;      // MGB_CHOL_BWD_FUSED=0: the backward sweep as one or two launches per height (no backward_fused launch)
  int bwd_cut = 2;            // MGB_CHOL_BWD_CUT: height of the subtrees the fused backward launch gives one workgroup each (raised by
                              // up to two heights until they are at most 256, one per CU; trees that need more keep the per-height launches)
  int bwd_fused_nf = 384;     // MGB_CHOL_BWD_FUSED_NF: heights with a larger front keep their own backward launches; 0: no limit
  int bwd_fused_threads = 512;  // MGB_CHOL_BWD_FUSED_THREADS: workgroup size of the fused backward launch (a power of two, 64 .. 512)
  int premap = 1;             // MGB_CHOL_PREMAP: children store their Schur complements in parent order (chol_premap.hpp) for
                              // 1: front_single consumers, 2: front_start consumers too (no gain measured inside a Newton step,
                              // DESIGN.md 4b); 0: every launch gathers through the index maps
  int premap_tiles = 400;     // MGB_CHOL_PREMAP_TILES: largest launch, in workgroups, that reads pre-mapped slabs (fem2d L=7: the
                              // 512-tile launch gains 0.4 us for a fifth of the slabs)
};
FusedKnobs fused_knobs(const CholKnobs& kn);

enum class Kind : unsigned char {
  Leaf, Single, SingleNarrow, SingleDense, SingleDenseNarrow, Start, Step, Step2, Panel2, Update2, BwdRect, Bwd256, Bwd1024, BwdFused
};

struct Launch {       // one dispatch of the chain
  Kind kind;
  int ofs, cnt;       // job range, one workgroup per job, in lists (Leaf, Bwd*), singles (Single*), starts (Start),
                      // tiles (Step, Step2, Panel2, Update2), rects (BwdRect) or the fused sweep's workgroup records (BwdFused)
  int block;          // threads per workgroup
  size_t lds;         // dynamic LDS bytes
  int p, npiv;        // first panel, leading pivot workgroups (step kinds)
  bool rect;          // Bwd*: the rectangular part ran in the BwdRect launch before
  double bytes;       // algorithmic bytes
  bool premap = false;     // Single*, Start: reads the contribution slabs (no gather)
  int nproducers = 0;      // Leaf, Single*: fronts of the launch that store into a slab
};

// Workgroup counts, written once: the planners count with an empty f, the job builders emit with one.
// f(ti, tj) for every 64x64 tile of the lower triangle of a front's trailing matrix from row k on; returns how many
template <class F>
int for_trailing_tiles(int nf, int k, F&& f) {
  const int Tr = (nf + 1 - k + TS - 1) / TS, Tc = std::max(1, (nf - k + TS - 1) / TS);
  int cnt = 0;
  for (int ti = 0; ti < Tr; ++ti)
    for (int tj = 0; tj <= std::min(ti, Tc - 1); ++tj, ++cnt) f(ti, tj);
  return cnt;
}
// f(chunk, rb) for every front_start job of a front, chunk-major: 32 columns x 256 rows, rows counted from the chunk's
// first (chunk * 32 .. nf inclusive); returns how many.  With the pivot knob a front with own columns has one job more.
template <class F>
int for_start_jobs(int nf, F&& f) {
  int cnt = 0;
  for (int ch = 0; ch * PB < nf; ++ch)
    for (int rb = 0; rb < (nf + 1 - ch * PB + TB - 1) / TB; ++rb, ++cnt) f(ch, rb);
  return cnt;
}
inline bool has_pivot_job(bool start_pivot, int ns) { return start_pivot && ns > 0; }

struct ChainPlan {
  std::vector<GNode> nodes;
  std::vector<int> asrc, apos;      // assembly lists, per node sorted by the front_start job that owns the destination
  std::vector<int> bdry;            // the concatenated boundary lists
  PremapPlan premap;                // pre-mapped child contributions (all flags off for split factorisations)
  FusedPlan fused;                  // fused backward sweep (unsplit factorisations): empty where it is off
  std::vector<int> lists;           // the job arrays every Launch indexes: node lists per height,
  std::vector<StartJob> starts;
  std::vector<StepTile> tiles;
  std::vector<SingleTile> singles;
  std::vector<RectJob> rects;
  // own forward | own backward | (split) top forward | top backward, in launch order; a launch's position is its profile slot.
  // Own: this rank's subtree when split, else everything; top: the replicated separators above the subtrees.
  std::vector<Launch> chain;
  int own_bwd = 0, top_fwd = 0;     // where own backward and the top begin
};

// part: the split over the ranks (owner empty or world 1: unsplit), rank: this one
ChainPlan plan_chain(const CholTree& T, const CholPartition& part, int rank, const CholKnobs& kn);

}  // namespace mgb
