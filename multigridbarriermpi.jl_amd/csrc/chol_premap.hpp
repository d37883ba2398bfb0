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
// Rule (plan_premap, called by plan_chain of chol_plan.hpp and by the host-only mgb_plan_chol_premap): a height's first
// launch is a consumer iff it is a Single* launch (MGB_CHOL_PREMAP >= 1) or a Start launch (>= 2), at least one of its fronts
// has a child, every present child of every front in it is produced by a Leaf or Single* launch, and it has at most
// MGB_CHOL_PREMAP_TILES workgroups.  A front is a producer iff its parent's launch is a consumer.
#pragma once
#include <vector>

namespace mgb {

struct CholTree;       // chol_plan.hpp: the tree view, the chain's constants and knobs
struct CholKnobs;

enum PremapHeightKind { PH_LEAF = 0, PH_SINGLE = 1, PH_START = 2 };

// what decides the first launch of a set of fronts of one height: front_leaf, front_single or front_start + panel launches
struct HeightShape {
  int max_ns = 0, max_nf = 0;
  bool childless = true, all_pivots = true, one_tile = true;
  void add(int ns, int nf, bool has_child);
  int kind(const CholKnobs& kn) const;      // PremapHeightKind
};

struct PremapPlan {
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

// Throws InternalError on a malformed extend-add map.
PremapPlan plan_premap(const CholTree& T, const CholKnobs& kn);

}  // namespace mgb
