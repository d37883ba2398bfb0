// Host tables of the fused backward sweep (see bwd_fused.hpp).  Host-compilable: no HIP.
#include "bwd_fused.hpp"

#include <algorithm>

#include "chol_plan.hpp"
#include "errors.hpp"

namespace mgb {

namespace {
int round64(int v) { return (v + 63) & ~63; }
}  // namespace

FusedPlan plan_bwd_fused(const CholTree& T, const FusedKnobs& kn) {
  FusedPlan P;
  const int n = T.size(), nheights = T.nheights;
  const std::vector<int>&ns = T.ns, &nf = T.nf, &first = T.first, &parent = T.parent, &height = T.height, &bofs = T.bofs;
  const std::vector<long long>&off = T.off, &loff = T.loff;
  if (kn.threads < 64 || kn.threads > 512 || (kn.threads & (kn.threads - 1))) throw ArgError("gpuchol: fused backward sweep: bad thread count");
  P.threads = kn.threads;
  P.slots.assign(T.bdry_total, -1);
  if (n == 0) return P;
  std::vector<int> hmax(nheights, 0);
  for (int t = 0; t < n; ++t) hmax[height[t]] = std::max(hmax[height[t]], nf[t]);
  // h_top: the heights below the first one that holds a front too large to repeat
  int h_top = -1;
  while (h_top + 1 < nheights && (kn.top_nf <= 0 || hmax[h_top + 1] <= kn.top_nf)) ++h_top;
  if (h_top < 0) return P;
  // h_cut: the knob, raised until the subtrees are no more than the workgroups the chip runs at once (a workgroup of
  // this kernel fills a CU: a second round would repeat every path) -- by at most max_raise heights.  A tree that needs
  // more has a bottom that is bound by throughput, not by latency: its heights run wider as launches of their own
  // (fem2d L=9, 16 384 leaves: 0.5 % slower through 256 subtrees of 127 fronts), so there is no fused launch then.
  int h_cut = std::min(std::max(kn.cut, 0), h_top);
  auto count_roots = [&](int c) {
    int k = 0;
    for (int t = 0; t < n; ++t) k += height[t] <= c && (parent[t] < 0 || height[parent[t]] > c);
    return k;
  };
  if (kn.max_wg > 0) {
    for (int raised = 0; raised < kn.max_raise && h_cut < h_top && count_roots(h_cut) > kn.max_wg; ++raised) ++h_cut;
    if (count_roots(h_cut) > kn.max_wg) return P;
  }
  // subtree roots left to right; root_of: the subtree a node belongs to (-1: above the cut)
  std::vector<int> roots, root_of(n, -1), minfirst(first);      // minfirst: first unknown of a node's subtree
  for (int t = 0; t < n; ++t)
    if (parent[t] >= 0) minfirst[parent[t]] = std::min(minfirst[parent[t]], minfirst[t]);
  for (int t = n - 1; t >= 0; --t) {      // parents first
    if (height[t] > h_cut) continue;
    if (parent[t] >= 0 && height[parent[t]] <= h_cut) root_of[t] = root_of[parent[t]];
    else root_of[t] = t;
  }
  for (int t = 0; t < n; ++t)
    if (root_of[t] == t) roots.push_back(t);
  // LDS slot of a node's first own unknown: ancestors' unknowns first (root down), the subtree's own range behind
  std::vector<int> above(n, 0), base(n, 0);      // above: unknowns of the strict ancestors
  for (int t = n - 1; t >= 0; --t)
    if (parent[t] >= 0) above[t] = above[parent[t]] + ns[parent[t]];
  for (int t = 0; t < n; ++t) {
    const int r = root_of[t];
    if (r < 0) {
      base[t] = above[t];
      continue;
    }
    // a subtree is a contiguous run of nodes and of unknowns ending at its root
    if (first[r] + ns[r] - minfirst[r] < 0 || first[t] < minfirst[r] || first[t] + ns[t] > first[r] + ns[r])
      throw InternalError("gpuchol: subtree unknowns are not contiguous");
    base[t] = above[r] + first[t] - minfirst[r];
  }
  for (int t = 0; t < n; ++t) {
    if (height[t] > h_top) continue;
    const std::vector<int>& bd = *T.bdry[t];
    int a = parent[t];
    for (size_t i = 0; i < bd.size(); ++i) {      // ascending: walk up the ancestors once
      while (a >= 0 && !(bd[i] >= first[a] && bd[i] < first[a] + ns[a])) a = parent[a];
      if (a < 0) {      // not ascending along the path: search from the parent again
        a = parent[t];
        while (a >= 0 && !(bd[i] >= first[a] && bd[i] < first[a] + ns[a])) a = parent[a];
        if (a < 0) throw InternalError("gpuchol: boundary entry outside the ancestors");
      }
      const int ab = (root_of[a] >= 0) ? base[a] : above[a];
      P.slots[bofs[t] + i] = ab + bd[i] - first[a];
    }
  }
  // the order of additions of the per-height launches: thread count and rectangular split of each height
  auto nsl_rect = [&](int t) {
    const int h = height[t], nb = nf[t] - ns[t];
    if (nb == 0 || ns[t] == 0) return 0;
    if (hmax[h] > kn.split_nf) return 1024 / 64;      // backward_rect_kernel: 1 024 threads, 64-column chunks
    const int nt = hmax[h] > 384 ? 1024 : 256;
    return nt / std::min(nt, round64(ns[t]));
  };
  // workgroup records
  const int W = kn.threads / 64;
  struct Rec {
    std::vector<std::vector<int>> levels;      // nodes per level
    int first_solve = 0, sub_level = 0;      // levels: (above h_top) | path, one front each | subtree, by depth
  };
  std::vector<Rec> recs(roots.size());
  std::vector<char> stored(n, 0);
  std::vector<std::vector<int>> kids(n);
  for (int t = 0; t < n; ++t)
    if (parent[t] >= 0) kids[parent[t]].push_back(t);
  size_t max_jobs = 0;
  for (size_t w = 0; w < roots.size(); ++w) {
    Rec& R = recs[w];
    const int r = roots[w];
    std::vector<int> anc;
    for (int a = parent[r]; a >= 0; a = parent[a]) anc.push_back(a);
    std::reverse(anc.begin(), anc.end());
    std::vector<int> ab;
    for (int a : anc)
      if (height[a] > h_top) ab.push_back(a);
    if (!ab.empty()) {
      R.levels.push_back(ab);
      R.first_solve = 1;
    }
    for (int a : anc)
      if (height[a] <= h_top) R.levels.push_back({a});
    R.sub_level = (int)R.levels.size();
    std::vector<int> cur{r};
    while (!cur.empty()) {
      R.levels.push_back(cur);
      std::vector<int> nxt;
      for (int t : cur) nxt.insert(nxt.end(), kids[t].begin(), kids[t].end());
      cur.swap(nxt);
    }
    size_t nj = 0;
    for (const auto& l : R.levels) nj += l.size();
    max_jobs = std::max(max_jobs, nj);
    P.max_levels = std::max(P.max_levels, (int)R.levels.size());
  }
  P.h_top = h_top;
  P.h_cut = h_cut;
  P.nwg = (int)roots.size();
  const int jo = kFusedHdr + kFusedLevelInts * P.max_levels;      // even
  P.wstride = jo + kFusedJobInts * (int)max_jobs;
  P.wg.assign((size_t)P.nwg * P.wstride, 0);
  for (size_t w = 0; w < roots.size(); ++w) {
    const Rec& R = recs[w];
    int* rec = P.wg.data() + w * P.wstride;
    const int r = roots[w];
    int nj = 0, sl = 0;
    for (size_t l = 0; l < R.levels.size(); ++l) {
      const std::vector<int>& lv = R.levels[l];
      int* li = rec + kFusedHdr + kFusedLevelInts * l;
      const bool solve = (int)l >= R.first_solve;
      int maxp = 0, items = 0;
      li[0] = nj;
      li[1] = (int)lv.size();
      for (int t : lv) {
        int* j = rec + jo + kFusedJobInts * nj++;
        const int nsl = solve ? nsl_rect(t) : 0;
        int flags = 0;
        if (!solve) flags = 2;
        else if (root_of[t] >= 0 || !stored[t]) {      // a path front is stored by the leftmost subtree below it
          flags = 1;
          stored[t] = 1;
        }
        j[FJ_OFF] = (int)(off[t] & 0xffffffffLL);
        j[FJ_OFF + 1] = (int)(off[t] >> 32);
        j[FJ_LOFF] = (int)(loff[t] & 0xffffffffLL);
        j[FJ_LOFF + 1] = (int)(loff[t] >> 32);
        j[FJ_FIRST] = first[t];
        j[FJ_NF] = nf[t];
        j[FJ_NS] = ns[t];
        j[FJ_SOFS] = bofs[t];
        j[FJ_BASE] = base[t];
        j[FJ_LSOFS] = sl;
        j[FJ_NSL] = nsl;
        j[FJ_NT] = hmax[height[t]] > 384 ? 1024 : 256;
        j[FJ_FLAGS] = flags;
        j[FJ_NODE] = t;
        if (solve) {
          sl += nf[t] - ns[t];
          maxp = std::max(maxp, (ns[t] + PB - 1) / PB);
          items = std::max(items, nsl * ns[t]);
        }
      }
      li[2] = maxp;
      li[3] = items;
      if (solve) {      // fronts of a level run side by side, a power-of-two share of the waves each
        int G = W;
        while (G > 1 && W / G < (int)lv.size()) G >>= 1;
        P.red_cap = std::max(P.red_cap, (W / G) * items);
      }
    }
    rec[0] = (int)R.levels.size();
    rec[1] = nj;
    rec[2] = R.first_solve;
    rec[3] = above[r] + first[r] + ns[r] - minfirst[r];
    rec[4] = sl;
    rec[5] = R.sub_level;
    P.xs_cap = std::max(P.xs_cap, rec[3]);
    P.sl_cap = std::max(P.sl_cap, sl);
  }
  P.lds_bytes = (size_t)P.wstride * 4 + (size_t)(P.xs_cap + P.red_cap) * 8 + (size_t)P.sl_cap * 4;
  return P;
}

}  // namespace mgb
