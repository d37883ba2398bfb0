// Host tables of the pre-mapped child contributions of the device Cholesky (gpuchol.hip).
//
// The extend-add maps are symbolic: the same for every factorisation on a level.  Where the launch that assembles a front
// qualifies (a "consumer": front_single / front_start, rule below) each child stores its Schur complement -- with the
// reduced right-hand side as its last row -- not into its own front but into a *contribution slab* of the parent, already
// in the parent's index order: slab s (child slot 0 / 1) of parent front t is indexed like the front itself,
// E_s[ld * j + i], ld = nf + 1, rows i >= j and the right-hand-side row i = nf, and child entry (a, q) lands at
// (fwd[a], fwd[q]).  The slabs are zeroed once; the producers write the same positions on every factorisation, so the
// uncovered entries stay +0.0 and the parent reads child0 + child1 as E_0[p] + E_1[p] at the entry's own position: two
// plain tile loads and one add, bitwise the gather's (x or 0.0) + (y or 0.0).
//
// Rule (one function, used by GpuChol::schedule and by the host-only mgb_plan_chol_premap): a height's first launch is a
// consumer iff it is a Single* launch (mode >= 1) or a Start launch (mode >= 2), at least one of its fronts has a child,
// every present child of every front in it is produced by a Leaf or Single* launch, and it has at most `tiles` workgroups.
// A front is a producer iff its parent's launch is a consumer.
#pragma once
#include <vector>

namespace mgb {

struct PremapKnobs {
  bool leaf = true;          // CholKnobs::leaf / single / start_pivot: they decide the launch kinds and workgroup counts
  bool single = true;
  bool start_pivot = true;
  int mode = 0;              // MGB_CHOL_PREMAP: 0 off, 1 front_single consumers, 2 front_start consumers too
  int tiles = 0;             // MGB_CHOL_PREMAP_TILES: largest consumer launch, in workgroups
};

enum PremapHeightKind { PH_LEAF = 0, PH_SINGLE = 1, PH_START = 2 };

// what schedule() decides per height before anything else: front_leaf, front_single or front_start + panel launches
struct HeightShape {
  int max_ns = 0, max_nf = 0;
  bool childless = true, all_pivots = true, one_tile = true;
  int kind(const PremapKnobs& kn) const;      // PremapHeightKind
};

struct PremapPlan {
  int nheights = 0;
  std::vector<int> height;         // per node (leaves 0)
  std::vector<int> hkind;          // per height: PremapHeightKind
  std::vector<int> hwg;            // per height: workgroups of its first launch (Leaf: fronts, Single: tiles, Start: jobs)
  std::vector<int> hconsumer;      // per height: 1 if that launch reads the slabs
  std::vector<int> producer;       // per node: 1 if it stores its Schur complement into its parent's slab
  std::vector<long long> soff;     // per node, 2 entries: slab offset per child slot (-1: no slab)
  std::vector<long long> eoff;     // per node: offset of the slab it stores into (-1: its own front)
  std::vector<int> pld;            // per node: leading dimension of the parent's front (0: root)
  std::vector<int> fofs;           // per node: where its forward map begins (-1: root)
  std::vector<int> fwd;            // forward maps: nb + 1 entries per node, boundary row -> parent front row (the last: nf of the parent)
  std::vector<int> iofs;           // per node: where its two (nf + 1)-long inverse maps begin (-1: no children)
  std::vector<int> pinv;           // per parent and child slot: parent front row -> child boundary row (-1: none; nf -> nb)
  long long slab_doubles = 0;
  bool any() const { return slab_doubles > 0; }
};

// ns / nf / parent / two child slots (-1: absent) per node in postorder; ea[t]: position of boundary entry i of node t in
// its parent's front (ascending).  Throws InternalError on a malformed map.
PremapPlan plan_premap(const std::vector<int>& ns, const std::vector<int>& nf, const std::vector<int>& parent,
                       const std::vector<int>& child0, const std::vector<int>& child1, const std::vector<const std::vector<int>*>& ea,
                       const PremapKnobs& kn);

}  // namespace mgb
