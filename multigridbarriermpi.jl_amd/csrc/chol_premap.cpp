// Host tables of the pre-mapped child contributions (see chol_premap.hpp).  Host-compilable: no HIP.
#include "chol_premap.hpp"

#include <algorithm>

#include "chol_plan.hpp"
#include "errors.hpp"

namespace mgb {

void HeightShape::add(int ns, int nf, bool has_child) {
  max_ns = std::max(max_ns, ns);
  max_nf = std::max(max_nf, nf);
  childless = childless && !has_child;
  all_pivots = all_pivots && ns >= 1;      // a pass-through front (ns = 0) needs front_start to copy it
  one_tile = one_tile && nf + 1 - std::min(ns, PB) <= TS;      // the trailing matrix after the first panel is one 64-row tile
}

int HeightShape::kind(const CholKnobs& kn) const {
  // leaf heights with small fronts: the whole front in one workgroup (front_leaf_kernel).  nf <= 95 alone is not enough:
  // a narrow leaf with a wide boundary (3-D trees under a small MGB_LEAF: ns = 16, nf = 88) has more trailing rows than
  // the kernel's one tile, and the rows past it were never updated
  if (kn.leaf && max_nf <= 95 && max_ns <= 2 * PB && childless && all_pivots && one_tile) return PH_LEAF;
  // single-panel heights with children: one dependency-free launch (front_single_kernel)
  if (kn.single && max_ns <= PB && !childless && all_pivots) return PH_SINGLE;
  return PH_START;
}

PremapPlan plan_premap(const CholTree& T, const CholKnobs& kn) {
  const int n = T.size();
  const std::vector<int>&ns = T.ns, &nf = T.nf, &parent = T.parent, &height = T.height;
  PremapPlan P;
  // forward maps (child boundary row -> parent front row) and their inverses
  P.fofs.assign(n, -1);
  P.pld.assign(n, 0);
  P.iofs.assign(n, -1);
  for (int t = 0; t < n; ++t) {
    if (parent[t] < 0) continue;
    const int nb = nf[t] - ns[t], pnf = nf[parent[t]];
    P.fofs[t] = (int)P.fwd.size();
    P.pld[t] = pnf + 1;
    for (int a = 0; a < nb; ++a) {
      const int e = (*T.ea[t])[a];
      if (e < 0 || e >= pnf || (a > 0 && e <= (*T.ea[t])[a - 1])) throw InternalError("chol_premap: bad extend-add map");
      P.fwd.push_back(e);
    }
    P.fwd.push_back(pnf);      // the right-hand-side row
  }
  for (int t = 0; t < n; ++t) {
    if (T.child[0][t] < 0 && T.child[1][t] < 0) continue;
    P.iofs[t] = (int)P.pinv.size();
    P.pinv.resize(P.pinv.size() + 2 * (size_t)(nf[t] + 1), -1);
    for (int s = 0; s < 2; ++s) {
      const int c = T.child[s][t];
      if (c < 0) continue;
      int* iv = P.pinv.data() + P.iofs[t] + (size_t)s * (nf[t] + 1);
      const int cnb = nf[c] - ns[c];
      for (int a = 0; a <= cnb; ++a) {
        const int e = P.fwd[P.fofs[c] + a];
        if (iv[e] != -1) throw InternalError("chol_premap: bad extend-add map");
        iv[e] = a;
      }
    }
  }
  // the first launch of every height: kind and workgroups
  std::vector<HeightShape> shape(T.nheights);
  for (int t = 0; t < n; ++t) shape[height[t]].add(ns[t], nf[t], T.child[0][t] >= 0 || T.child[1][t] >= 0);
  P.hkind.assign(T.nheights, PH_START);
  P.hwg.assign(T.nheights, 0);
  for (int h = 0; h < T.nheights; ++h) P.hkind[h] = shape[h].kind(kn);
  const auto count = [](int, int) {};
  for (int t = 0; t < n; ++t) {
    const int h = height[t];
    if (P.hkind[h] == PH_LEAF) P.hwg[h] += 1;
    else if (P.hkind[h] == PH_SINGLE) P.hwg[h] += for_trailing_tiles(nf[t], ns[t], count);      // behind the one panel
    else P.hwg[h] += has_pivot_job(kn.start_pivot, ns[t]) + for_start_jobs(nf[t], count);
  }
  // the rule
  P.hconsumer.assign(T.nheights, 0);
  for (int h = 0; h < T.nheights; ++h) {
    const bool kind_ok = (P.hkind[h] == PH_SINGLE && kn.premap >= 1) || (P.hkind[h] == PH_START && kn.premap >= 2);
    P.hconsumer[h] = (kind_ok && !shape[h].childless && P.hwg[h] <= kn.premap_tiles) ? 1 : 0;
  }
  for (int t = 0; t < n; ++t)
    if (parent[t] >= 0 && P.hkind[height[t]] == PH_START) P.hconsumer[height[parent[t]]] = 0;
  // slabs: one per present child of every consumer front, indexed like the front (ld x nf, lower part + row nf)
  P.producer.assign(n, 0);
  P.soff.assign(2 * (size_t)n, -1);
  P.eoff.assign(n, -1);
  for (int t = 0; t < n; ++t) {
    if (!P.hconsumer[height[t]]) continue;
    for (int s = 0; s < 2; ++s) {
      const int c = T.child[s][t];
      if (c < 0) continue;
      P.soff[2 * (size_t)t + s] = P.slab_doubles;
      P.eoff[c] = P.slab_doubles;
      P.producer[c] = 1;
      P.slab_doubles += (long long)(nf[t] + 1) * nf[t];
    }
  }
  return P;
}

}  // namespace mgb
