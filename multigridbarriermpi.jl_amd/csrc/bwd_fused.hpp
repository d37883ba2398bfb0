// Host tables of the fused backward sweep of the device Cholesky (backward_fused_kernel, gpuchol.hip): plan_bwd_fused, called
// by plan_chain (chol_plan.hpp) and by the host-only mgb_plan_chol_bwd_fused, on the tree view and front layout they share.
//
// A front of the backward sweep L'x = u needs only the solution entries of its ancestors.  So the elimination tree is
// cut at a height h_cut: every maximal subtree of height <= h_cut gets ONE workgroup, which first solves the fronts on
// its own path (ancestors of height <= h_top, top down; every workgroup below the same ancestor repeats that solve
// with the same code on the same data, so all copies agree bit for bit) and then its subtree, one depth at a time.
// Nothing crosses workgroups: no flags, no atomics, no grid barrier.  Fronts above h_top (too large to repeat) keep
// their per-height launches; their solution entries are read from global memory at kernel entry.
//
// The values a workgroup has computed or read live in one LDS vector: ancestors first (root down to the parent of the
// subtree root), the subtree's own unknowns behind (a subtree's unknowns are one contiguous range of the new ordering).
// The slot of boundary entry i of front t depends only on t's ancestors, so one table, parallel to the boundary
// lists, serves every workgroup.
#pragma once
#include <cstddef>
#include <vector>

namespace mgb {

struct CholTree;

struct FusedKnobs {
  int cut = 2;         // h_cut: subtree height (heights above the leaves) ...
  int max_wg = 256;    // ... raised until there are at most this many subtrees (the CUs of an MI355X); <= 0: no limit
  int max_raise = 2;   // ... by at most this many heights: beyond, no fused launch (the per-height launches run wider)
  int top_nf = 384;    // heights with a front larger than this keep their own launches (h_top is below them); <= 0: no limit
  int threads = 512;   // workgroup size of the fused kernel: a power of two, 64 .. 512
  int split_nf = 192;  // CholKnobs::bwd_split_nf of the per-height schedule whose order of additions is reproduced
};

// layout of one workgroup's record (ints): header, levels, jobs
constexpr int kFusedHdr = 8;        // nlevels, njobs, first level to solve, xs length, slot-list length, first subtree level, 2 unused
constexpr int kFusedLevelInts = 4;  // first job, jobs, most panels of a job, reduction scratch per front (doubles; 0: no boundary)
constexpr int kFusedJobInts = 16;
enum FusedJobField {                // ints of a job
  FJ_OFF = 0,       // (2) front offset
  FJ_LOFF = 2,      // (2) offset of the front's pivot blocks
  FJ_FIRST = 4,     // first own unknown (new ordering)
  FJ_NF = 5,
  FJ_NS = 6,
  FJ_SOFS = 7,      // offset of the front's slot list in the table (= its boundary-list offset)
  FJ_BASE = 8,      // LDS slot of its first own unknown
  FJ_LSOFS = 9,     // offset of its staged slot list in the workgroup's LDS copy
  FJ_NSL = 10,      // partial sums per column of the rectangular part (0: no boundary)
  FJ_NT = 11,       // thread count of the per-height kernel whose panel-update order is reproduced
  FJ_FLAGS = 12,    // 1: this workgroup stores the front's solution; 2: above h_top (entries read from y, nothing to solve)
  FJ_NODE = 13
};

struct FusedPlan {
  int h_top = -1, h_cut = -1, nwg = 0;
  int wstride = 0;      // ints per workgroup record (even)
  int max_levels = 0;
  int xs_cap = 0, sl_cap = 0, red_cap = 0;      // LDS: solution vector / reduction scratch (doubles), staged slot lists (ints)
  int threads = 0;
  size_t lds_bytes = 0;
  std::vector<int> wg;       // nwg records
  std::vector<int> slots;    // parallel to the concatenated boundary lists
  bool enabled() const { return nwg > 0; }
};

// T: the tree view with the front layout the job records quote (chol_plan.hpp)
FusedPlan plan_bwd_fused(const CholTree& T, const FusedKnobs& kn);

}  // namespace mgb
