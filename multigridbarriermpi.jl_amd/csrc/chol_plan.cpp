// Host plan of the device Cholesky chain (see chol_plan.hpp).  Host-compilable: no HIP.
#include "chol_plan.hpp"

#include <numeric>

#include "errors.hpp"

namespace mgb {

void CholTree::layout() {
  const int nn = size();
  height.assign(nn, 0);
  off.resize(nn);
  loff.resize(nn);
  bofs.resize(nn);
  front_doubles = linv_doubles = 0;
  bdry_total = max_nf = 0;
  int nchildren = 0, nparents = 0;
  for (int t = 0; t < nn; ++t) {      // postorder: children first
    for (int s = 0; s < 2; ++s) {
      const int c = child[s][t];
      if (c < 0) continue;
      if (c >= t || parent[c] != t) throw InternalError("gpuchol: elimination tree is not in postorder");
      height[t] = std::max(height[t], height[c] + 1);
      ++nchildren;
    }
    nparents += parent[t] >= 0;
    const size_t nb = (size_t)(nf[t] - ns[t]);
    if (bdry[t]->size() != nb || (parent[t] >= 0 && ea[t]->size() != nb)) throw InternalError("gpuchol: ea/bdry size mismatch");
    if ((long long)(nf[t] + 1) * (nf[t] + 1) > 2000000000LL) throw ArgError("gpuchol: front too large");
    off[t] = front_doubles;
    loff[t] = linv_doubles;
    bofs[t] = bdry_total;
    front_doubles += (long long)(nf[t] + 1) * (nf[t] + 1);
    linv_doubles += (long long)((ns[t] + PB - 1) / PB) * 2 * PB * PB;
    bdry_total += (int)nb;
    max_nf = std::max(max_nf, nf[t]);
  }
  if (nchildren != nparents) throw InternalError("gpuchol: child / parent mismatch");
  nheights = nn ? *std::max_element(height.begin(), height.end()) + 1 : 0;
}

FusedKnobs fused_knobs(const CholKnobs& kn) {
  FusedKnobs fk;
  fk.cut = kn.bwd_cut;
  fk.top_nf = kn.bwd_fused_nf;
  fk.threads = kn.bwd_fused_threads;
  fk.split_nf = kn.bwd_split_nf;
  return fk;
}

namespace {

// what StartJob and SingleTile carry inline of front t and its children
template <class J>
void fill_inline(J& j, const ChainPlan& P, int t) {
  const GNode& g = P.nodes[t];
  j.off = g.off;
  j.loff = g.loff;
  j.nf = g.nf;
  j.ns = g.ns;
  j.iofs = g.iofs;
  j.first = g.first;
  for (int s = 0; s < 2; ++s) {
    j.boff[s] = g.off;
    j.cld[s] = 0;
    if (g.child[s] >= 0) {
      const GNode& c = P.nodes[g.child[s]];
      j.cld[s] = c.nf + 1;
      j.boff[s] = c.off + (long long)j.cld[s] * c.ns + c.ns;
    }
    j.soff[s] = std::max(0LL, P.premap.soff[2 * (size_t)t + s]);
  }
}

// the workgroup of front g (node t) that factors the pivot block after panel p
StepTile pivot_tile(const GNode& g, int t, int p) {
  StepTile st{};
  st.off = g.off;
  st.loff = g.loff + (long long)p * 2 * PB * PB;
  st.nf = g.nf;
  st.ns = g.ns;
  st.pad = t;      // node index (front_single_kernel)
  return st;
}

// Appends the 64x64 tiles of front g's trailing matrix from row k on, after panel p: the lower triangle or (column) one
// tile per 64-row block below the next pivot block -- the workgroups of a panel launch.  Returns how many.
int append_tiles(std::vector<StepTile>& out, const GNode& g, int t, int p, int k, bool column) {
  StepTile st = pivot_tile(g, t, p);
  if (column) {
    const int Tr = std::max(0, (g.nf + 1 - k - PB + TS - 1) / TS);
    for (int ti = 0; ti < Tr; ++ti) {
      st.ti = st.tj = (short)ti;
      out.push_back(st);
    }
    return Tr;
  }
  if ((g.nf + 1 - k + TS - 1) / TS > 30000) throw ArgError("gpuchol: front too large for tile index");
  return for_trailing_tiles(g.nf, k, [&](int ti, int tj) {
    st.ti = (short)ti;
    st.tj = (short)tj;
    out.push_back(st);
  });
}

// Appends the launches of one node set to P.chain -- the forward ones height by height from the leaves, then the backward
// ones from the root -- and their jobs to the job arrays; returns where the backward ones begin.  heights[h]: the set's nodes
// of tree height h.  whole: the set is the whole tree, so the pre-map and fused plans apply.
int schedule(ChainPlan& P, const CholTree& T, const std::vector<std::vector<int>>& heights,
             const std::vector<std::vector<StartJob>>& sjobs, const CholKnobs& kn, bool whole) {
  const std::vector<GNode>& nodes = P.nodes;
  std::vector<Launch>& chain = P.chain;
  std::vector<Launch> bwd;
  std::vector<StepTile> scratch;
  // the fused backward launch (unsplit factorisations) takes every height up to h_top
  const bool fused = P.fused.enabled() && whole;
  const bool planned = whole && P.premap.any();      // (no slabs: nothing to cross-check or flag)
  double fused_bytes = 0;
  for (size_t hh = 0; hh < heights.size(); ++hh) {
    const std::vector<int>& mine = heights[hh];
    if (mine.empty()) continue;
    const int nofs = (int)P.lists.size(), ncnt = (int)mine.size();
    P.lists.insert(P.lists.end(), mine.begin(), mine.end());
    HeightShape shape;
    double start_bytes = 0;
    for (int t : mine) {
      const GNode& g = nodes[t];
      shape.add(g.ns, g.nf, g.child[0] >= 0 || g.child[1] >= 0);
      start_bytes += 0.5 * g.nf * g.nf * 8.0 + (double)T.a_idx[t]->size() * 20.0;
      for (int c : g.child) {
        if (c < 0) continue;
        const double cnb = nodes[c].nf - nodes[c].ns;
        start_bytes += 0.5 * cnb * cnb * 8.0;     // child entry read (the parent entry write is counted above)
      }
    }
    const int max_ns = shape.max_ns, max_nf = shape.max_nf;
    // front_leaf (the whole front in one workgroup), front_single (single-panel heights with children: one dependency-free
    // launch) or front_start + panel launches: HeightShape::kind, shared with the pre-mapping rule
    const int hkind = shape.kind(kn);
    const bool leaf = hkind == PH_LEAF, single = hkind == PH_SINGLE;
    // pre-mapped child contributions (the plan covers the whole tree, height by height)
    const bool consumer = planned && P.premap.hconsumer[hh];
    int nprod = 0;
    if (planned)
      for (int t : mine) nprod += P.premap.producer[t];
    auto check_wg = [&](int cnt) {
      if (planned && P.premap.hwg[hh] != cnt) throw InternalError("gpuchol: pre-map plan disagrees with the launch size");
    };
    if (leaf) {
      const size_t lds = ((size_t)(max_nf + 1) * max_nf - (size_t)max_nf * (max_nf - 1) / 2) * sizeof(double);
      check_wg(ncnt);
      chain.push_back({Kind::Leaf, nofs, ncnt, TB, lds, 0, 0, false, start_bytes, false, nprod});
    } else if (!single) {
      const int ofs = (int)P.starts.size();
      for (int t : mine)      // dedicated pivot jobs first: they are what the first panel launch waits for
        if (has_pivot_job(kn.start_pivot, nodes[t].ns)) {
          StartJob pj = sjobs[t].front();      // chunk 0, row block 0: its assembly range covers the pivot block
          pj.rb = -1;
          P.starts.push_back(pj);
        }
      for (int t : mine) P.starts.insert(P.starts.end(), sjobs[t].begin(), sjobs[t].end());
      check_wg((int)P.starts.size() - ofs);
      if (nprod) throw InternalError("gpuchol: a multi-panel front cannot store pre-mapped");
      chain.push_back({Kind::Start, ofs, (int)P.starts.size() - ofs, TB, 0, 0, 0, false, start_bytes, consumer, 0});
    }
    // panel launches, pivot-owning workgroups first: they are the critical path of the next launch
    const int npanel = leaf ? 0 : (max_ns + PB - 1) / PB;
    for (int p = 0; p < npanel; ++p) {
      // two panels per launch (front_step2) while the height has at least two left; the odd last one runs front_step
      // ... and only where the launch is latency-bound (its tiles fit the chip in one round): front_step2 holds 115 KB of
      // LDS, one workgroup per CU, and loses against two rank-32 launches at 2-3 workgroups per CU on the big 3-D heights
      const bool two = kn.step2 && !single && p + 1 < npanel;
      int ntile2 = 0;
      if (two) {
        scratch.clear();
        for (int t : mine)
          if (nodes[t].ns > p * PB) ntile2 += append_tiles(scratch, nodes[t], t, p, std::min(nodes[t].ns, (p + 2) * PB), false);
      }
      const bool pair = two && ntile2 <= kn.step2_tiles;
      const int ofs = (int)P.tiles.size();
      int npiv = 0;
      double bytes = 0;
      if (two && !pair && kn.wide) {
        // beyond that tile count: the same two panels as a panel launch (one workgroup per 64-row block, row block 0 also
        // factors the next pivot block) and an update launch (the tiles, rank-64, nothing else) -- see front_step2_body
        for (int t : mine) {
          const GNode& g = nodes[t];
          if (g.ns <= p * PB) continue;
          P.tiles.push_back(pivot_tile(g, t, p));      // the front's pivot workgroup: trailing rows k2 .. k2 + 31
          npiv++;
          const int k2 = std::min(g.ns, (p + 2) * PB);
          const double tr = g.nf + 1 - k2;
          bytes += tr * (k2 - p * PB) * 32.0;      // panel read, mirrored + in-place write
        }
        for (int t : mine)
          if (nodes[t].ns > p * PB) append_tiles(P.tiles, nodes[t], t, p, std::min(nodes[t].ns, (p + 2) * PB), true);
        chain.push_back({Kind::Panel2, ofs, (int)P.tiles.size() - ofs, TB, kPanel2Lds, p, npiv, false, bytes});
        const int uofs = (int)P.tiles.size();
        double ubytes = 0;
        for (int t : mine) {
          const GNode& g = nodes[t];
          if (g.ns <= p * PB) continue;
          const int k2 = std::min(g.ns, (p + 2) * PB);
          append_tiles(P.tiles, g, t, p, k2, false);
          const double tr = g.nf + 1 - k2;
          ubytes += tr * (k2 - p * PB) * 8.0 + 0.5 * tr * tr * 16.0;      // solved panel read, trailing read + write
        }
        chain.push_back({Kind::Update2, uofs, (int)P.tiles.size() - uofs, TB, kUpdate2Lds, p, 0, false, ubytes});
        ++p;
        continue;
      }
      const int np = pair ? 2 : 1;
      for (int t : mine) {
        const GNode& g = nodes[t];
        if (g.ns <= p * PB) continue;
        const int k1 = std::min(g.ns, (p + np) * PB), kw = k1 - p * PB;      // first trailing row, pivots of this launch
        if (k1 < g.ns) {
          P.tiles.push_back(pivot_tile(g, t, p));
          npiv++;
        }
        const double tr = g.nf + 1 - k1;
        bytes += tr * kw * 16.0 + 0.5 * tr * tr * 16.0;      // panel read + mirrored write, trailing read + write
      }
      for (int t : mine)
        if (nodes[t].ns > p * PB) append_tiles(P.tiles, nodes[t], t, p, std::min(nodes[t].ns, (p + np) * PB), false);
      const int cnt = (int)P.tiles.size() - ofs;
      if (single) {      // same tiles, self-contained descriptors
        const int sofs = (int)P.singles.size();
        for (int q = ofs; q < ofs + cnt; ++q) {
          const StepTile& s = P.tiles[q];
          const GNode& g = nodes[s.pad];
          SingleTile u{};
          fill_inline(u, P, s.pad);
          u.pld = g.pld;
          u.fofs = g.fofs;
          u.eoff = g.eoff;
          u.a0 = g.a0;
          u.a1 = g.a1;
          u.ti = s.ti;
          u.tj = s.tj;
          P.singles.push_back(u);
        }
        check_wg(cnt);
        const bool narrow = max_ns <= 8, dense = cnt > kn.dense_tiles;
        const Kind k = dense ? (narrow ? Kind::SingleDenseNarrow : Kind::SingleDense) : (narrow ? Kind::SingleNarrow : Kind::Single);
        chain.push_back({k, sofs, cnt, TB, 0, 0, 0, false, start_bytes + bytes, consumer, nprod});
      } else {
        chain.push_back({pair ? Kind::Step2 : Kind::Step, ofs, cnt, TB, pair ? (size_t)kStep2Lds : 0, p, npiv, false, bytes});
      }
      if (pair) ++p;
    }
    // backward: above bwd_split_nf the rectangular part runs in its own multi-workgroup launch first
    const bool split = max_nf > kn.bwd_split_nf;
    const int rofs = (int)P.rects.size();
    double rect_bytes = 0, tri_bytes = 0;
    for (int t : mine) {
      const GNode& g = nodes[t];
      const double nb = g.nf - g.ns;
      rect_bytes += nb * g.ns * 8.0 + nb * 12.0;
      tri_bytes += 0.5 * g.ns * g.ns * 8.0 + g.ns * 28.0;
      if (split && nb > 0)
        for (int ch = 0; ch * 64 < g.ns; ++ch) P.rects.push_back({t, ch});
    }
    const int nrect = (int)P.rects.size() - rofs, nt = max_nf > 384 ? 1024 : 256;
    if (fused && (int)hh <= P.fused.h_top) {
      P.rects.resize(rofs);
      fused_bytes += rect_bytes + tri_bytes;
      continue;
    }
    std::vector<Launch> h;
    if (nrect) h.push_back({Kind::BwdRect, rofs, nrect, RT, (size_t)(max_nf + RT) * sizeof(double), 0, 0, false, rect_bytes});
    h.push_back({nt == 1024 ? Kind::Bwd1024 : Kind::Bwd256, nofs, ncnt, nt, (size_t)(max_nf + nt + PB) * sizeof(double), 0, 0, nrect > 0,
                 tri_bytes + (nrect ? 0.0 : rect_bytes)});
    bwd.insert(bwd.begin(), h.begin(), h.end());      // the backward sweep runs from the root
  }
  const int first_bwd = (int)chain.size();
  chain.insert(chain.end(), bwd.begin(), bwd.end());
  if (fused) chain.push_back({Kind::BwdFused, 0, P.fused.nwg, P.fused.threads, P.fused.lds_bytes, 0, 0, false, fused_bytes});
  return first_bwd;
}

}  // namespace

ChainPlan plan_chain(const CholTree& T, const CholPartition& part, int rank, const CholKnobs& kn) {
  const int nn = T.size();
  const bool split = part.split();
  ChainPlan P;
  {      // pre-mapped child contributions: the tables first, every descriptor below carries its part of them
    CholKnobs pk = kn;
    if (split) pk.premap = 0;      // schur_pack_kernel reads the subtree roots' Schur complements from the fronts
    P.premap = plan_premap(T, pk);
  }
  P.nodes.resize(nn);
  for (int t = 0; t < nn; ++t) {
    GNode& g = P.nodes[t];
    g.pld = P.premap.pld[t];
    g.fofs = P.premap.fofs[t];
    g.eoff = P.premap.eoff[t];
    g.off = T.off[t];
    g.loff = T.loff[t];
    g.nf = T.nf[t];
    g.ns = T.ns[t];
    g.first = T.first[t];
    g.parent = T.parent[t];
    g.bofs = T.bofs[t];
    g.child[0] = T.child[0][t];
    g.child[1] = T.child[1][t];
    g.iofs = P.premap.iofs[t];      // the inverse maps (per parent and child slot: parent front row -> child boundary row, the
                                    // child's right-hand-side row for nf) come with the plan: premap.pinv
    P.bdry.insert(P.bdry.end(), T.bdry[t]->begin(), T.bdry[t]->end());
  }
  // assembly map, per node sorted by the front_start job (32-column chunk, 256-row block counted from the chunk's
  // first row) that owns the destination; positions in the (nf+1)-leading-dimension layout
  std::vector<std::vector<StartJob>> sjobs(nn);
  for (int t = 0; t < nn; ++t) {
    const int nf = T.nf[t], ld = nf + 1;
    const std::vector<int>&a_idx = *T.a_idx[t], &a_pos = *T.a_pos[t];
    const size_t m = a_idx.size();
    if ((nf + 1 + TB - 1) / TB > 65535) throw ArgError("gpuchol: front too large for the start-job key");
    auto key = [&](int e) {
      const int pos = a_pos[e], col = pos / nf, row = pos % nf, ch = col / PB;
      return (long long)ch * 65536 + (row - ch * PB) / TB;
    };
    std::vector<int> ord(m);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return key(a) < key(b); });
    size_t q = 0;
    for_start_jobs(nf, [&](int ch, int rb) {
      StartJob j{};
      fill_inline(j, P, t);
      j.node = t;
      j.chunk = ch;
      j.rb = rb;
      j.a0 = (int)P.asrc.size();
      while (q < m && key(ord[q]) == (long long)ch * 65536 + rb) {
        const int pos = a_pos[ord[q]], col = pos / nf, row = pos % nf;
        if (row < col) throw InternalError("gpuchol: assembly entry above the diagonal");
        P.asrc.push_back(a_idx[ord[q]]);
        P.apos.push_back(ld * col + row);
        ++q;
      }
      j.a1 = (int)P.asrc.size();
      sjobs[t].push_back(j);
    });
    if (q != m) throw InternalError("gpuchol: assembly entry outside the front");
    P.nodes[t].a0 = sjobs[t].empty() ? 0 : sjobs[t].front().a0;
    P.nodes[t].a1 = sjobs[t].empty() ? 0 : sjobs[t].back().a1;
  }
  // schedule: the nodes of every height, own (split: this rank's subtree; else everything) and the replicated top
  std::vector<std::vector<int>> own(T.nheights), top(T.nheights);
  for (int t = 0; t < nn; ++t) {
    if (!split || part.owner[t] == rank) own[T.height[t]].push_back(t);
    else if (part.owner[t] < 0) top[T.height[t]].push_back(t);
  }
  if (!split && kn.bwd_fused) {
    P.fused = plan_bwd_fused(T, fused_knobs(kn));
    if (P.fused.lds_bytes > 150 * 1024) P.fused = FusedPlan();      // does not fit: the per-height launches
  }
  P.own_bwd = schedule(P, T, own, sjobs, kn, !split);
  P.top_fwd = (int)P.chain.size();
  if (split) schedule(P, T, top, sjobs, kn, false);
  if ((size_t)(T.max_nf + RT + PB) * 8 > 150 * 1024) throw ArgError("gpuchol: front exceeds the LDS budget of the sweeps");
  return P;
}

}  // namespace mgb
