// Host tables of the pre-mapped child contributions (see chol_premap.hpp).  Host-compilable: no HIP.
#include "chol_premap.hpp"

#include <algorithm>

#include "errors.hpp"

namespace mgb {

namespace {
constexpr int PB = 32, TS = 64, TB = 256;      // panel width, tile, threads per workgroup (gpuchol.hip)
}

int HeightShape::kind(const PremapKnobs& kn) const {
  // leaf heights with small fronts: the whole front in one workgroup (front_leaf_kernel).  nf <= 95 alone is not enough:
  // a narrow leaf with a wide boundary (3-D trees under a small MGB_LEAF: ns = 16, nf = 88) has more trailing rows than
  // the kernel's one tile, and the rows past it were never updated
  if (kn.leaf && max_nf <= 95 && max_ns <= 2 * PB && childless && all_pivots && one_tile) return PH_LEAF;
  // single-panel heights with children: one dependency-free launch (front_single_kernel)
  if (kn.single && max_ns <= PB && !childless && all_pivots) return PH_SINGLE;
  return PH_START;
}

PremapPlan plan_premap(const std::vector<int>& ns, const std::vector<int>& nf, const std::vector<int>& parent,
                       const std::vector<int>& child0, const std::vector<int>& child1, const std::vector<const std::vector<int>*>& ea,
                       const PremapKnobs& kn) {
  const int n = (int)ns.size();
  PremapPlan P;
  P.height.assign(n, 0);
  for (int t = 0; t < n; ++t)      // postorder: children first
    for (int c : {child0[t], child1[t]})
      if (c >= 0) P.height[t] = std::max(P.height[t], P.height[c] + 1);
  P.nheights = n ? *std::max_element(P.height.begin(), P.height.end()) + 1 : 0;
  // forward maps (child boundary row -> parent front row) and their inverses
  P.fofs.assign(n, -1);
  P.pld.assign(n, 0);
  P.iofs.assign(n, -1);
  for (int t = 0; t < n; ++t) {
    if (parent[t] < 0) continue;
    const int nb = nf[t] - ns[t], pnf = nf[parent[t]];
    if ((int)ea[t]->size() != nb) throw InternalError("chol_premap: ea/bdry size mismatch");
    P.fofs[t] = (int)P.fwd.size();
    P.pld[t] = pnf + 1;
    for (int a = 0; a < nb; ++a) {
      const int e = (*ea[t])[a];
      if (e < 0 || e >= pnf || (a > 0 && e <= (*ea[t])[a - 1])) throw InternalError("chol_premap: bad extend-add map");
      P.fwd.push_back(e);
    }
    P.fwd.push_back(pnf);      // the right-hand-side row
  }
  for (int t = 0; t < n; ++t) {
    if (child0[t] < 0 && child1[t] < 0) continue;
    P.iofs[t] = (int)P.pinv.size();
    P.pinv.resize(P.pinv.size() + 2 * (size_t)(nf[t] + 1), -1);
    for (int s = 0; s < 2; ++s) {
      const int c = s ? child1[t] : child0[t];
      if (c < 0) continue;
      if (parent[c] != t) throw InternalError("chol_premap: child / parent mismatch");
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
  std::vector<HeightShape> shape(P.nheights);
  std::vector<int> has_child(P.nheights, 0);
  for (int t = 0; t < n; ++t) {
    HeightShape& h = shape[P.height[t]];
    h.max_ns = std::max(h.max_ns, ns[t]);
    h.max_nf = std::max(h.max_nf, nf[t]);
    h.childless = h.childless && child0[t] < 0 && child1[t] < 0;
    h.all_pivots = h.all_pivots && ns[t] >= 1;
    h.one_tile = h.one_tile && nf[t] + 1 - std::min(ns[t], PB) <= TS;
    if (child0[t] >= 0 || child1[t] >= 0) has_child[P.height[t]] = 1;
  }
  P.hkind.assign(P.nheights, PH_START);
  P.hwg.assign(P.nheights, 0);
  for (int h = 0; h < P.nheights; ++h) P.hkind[h] = shape[h].kind(kn);
  for (int t = 0; t < n; ++t) {
    const int h = P.height[t];
    if (P.hkind[h] == PH_LEAF) {
      P.hwg[h] += 1;
    } else if (P.hkind[h] == PH_SINGLE) {      // the tiles of the trailing matrix behind the one panel (append_tiles)
      const int k = ns[t], Tr = (nf[t] + 1 - k + TS - 1) / TS, Tc = std::max(1, (nf[t] - k + TS - 1) / TS);
      for (int ti = 0; ti < Tr; ++ti) P.hwg[h] += std::min(ti, Tc - 1) + 1;
    } else {      // front_start: 32 columns x 256 rows per job, and the pivot job
      const int nch = (nf[t] + PB - 1) / PB;
      if (kn.start_pivot && ns[t] > 0 && nch > 0) P.hwg[h] += 1;
      for (int ch = 0; ch < nch; ++ch) P.hwg[h] += (nf[t] + 1 - ch * PB + TB - 1) / TB;
    }
  }
  // the rule
  P.hconsumer.assign(P.nheights, 0);
  for (int h = 0; h < P.nheights; ++h) {
    const bool kind_ok = (P.hkind[h] == PH_SINGLE && kn.mode >= 1) || (P.hkind[h] == PH_START && kn.mode >= 2);
    P.hconsumer[h] = (kind_ok && has_child[h] && P.hwg[h] <= kn.tiles) ? 1 : 0;
  }
  for (int t = 0; t < n; ++t)
    for (int c : {child0[t], child1[t]})
      if (c >= 0 && P.hkind[P.height[c]] == PH_START) P.hconsumer[P.height[t]] = 0;
  // slabs: one per present child of every consumer front, indexed like the front (ld x nf, lower part + row nf)
  P.producer.assign(n, 0);
  P.soff.assign(2 * (size_t)n, -1);
  P.eoff.assign(n, -1);
  for (int t = 0; t < n; ++t) {
    if (!P.hconsumer[P.height[t]]) continue;
    for (int s = 0; s < 2; ++s) {
      const int c = s ? child1[t] : child0[t];
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
