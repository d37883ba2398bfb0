// Stand-alone check of the host plan of the device Cholesky chain (csrc/chol_plan.hpp): a 2-D grid pattern with
// coordinates at two sizes is analysed (MfChol) and planned (plan_chain) under every knob set of
// tests/chol_reference.py VARIANTS, unsplit and split over 2 and 4 ranks, and every index the plan holds is checked
// against the array it points into.  Meant to be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I multigridbarriermpi.jl_amd/csrc \
//       tools/chol_plan_host_check.cpp multigridbarriermpi.jl_amd/csrc/{mfchol,chol_plan,chol_premap,bwd_fused}.cpp \
//       -o tools/_bin/chol_plan_host_check
// Exit status 0 and "chol_plan_host_check ok" when every property holds.
#include <cstdio>
#include <cstdlib>

#include "chol_plan.hpp"

using namespace mgb;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

struct Variant {
  const char* name;
  const char* leaf;      // MGB_LEAF (read by every analysis) or null
  CholKnobs kn;
};

static std::vector<Variant> variants() {
  std::vector<Variant> v;
  auto add = [&](const char* name, const char* leaf = nullptr) -> CholKnobs& {
    v.push_back({name, leaf, CholKnobs()});
    return v.back().kn;
  };
  add("default");
  add("STEP2=0").step2 = false;
  add("STEP2_TILES=0").step2_tiles = 0;
  {
    CholKnobs& k = add("STEP2_TILES=0 WIDE=0");
    k.step2_tiles = 0;
    k.wide = false;
  }
  add("DENSE_TILES=0").dense_tiles = 0;
  add("START_PIVOT=0").start_pivot = false;
  add("GRAPH=0").graph = false;
  {
    CholKnobs& k = add("LEAF=0 SINGLE=0");
    k.leaf = k.single = false;
  }
  {
    CholKnobs& k = add("BWD_FUSED=0 SPLIT_NF=0");
    k.bwd_fused = false;
    k.bwd_split_nf = 0;
  }
  add("BWD_FUSED=0").bwd_fused = false;
  add("MGB_LEAF=8", "8");
  add("MGB_LEAF=160", "160");
  return v;
}

static void check_plan(const CholTree& T, const ChainPlan& P, bool split) {
  const int nn = T.size();
  const size_t nasm = P.asrc.size();
  CHECK(P.nodes.size() == (size_t)nn && P.apos.size() == nasm && (int)P.bdry.size() == T.bdry_total);
  CHECK(0 <= P.own_bwd && P.own_bwd <= P.top_fwd && P.top_fwd <= (int)P.chain.size() && !P.chain.empty());
  CHECK(split || P.top_fwd == (int)P.chain.size());
  CHECK(!split || (!P.premap.any() && !P.fused.enabled()));
  for (int t = 0; t < nn; ++t) {
    const GNode& g = P.nodes[t];
    CHECK(g.off >= 0 && g.off + (long long)(g.nf + 1) * (g.nf + 1) <= T.front_doubles);
    CHECK(g.loff >= 0 && g.loff + (long long)((g.ns + PB - 1) / PB) * 2 * PB * PB <= T.linv_doubles);
    CHECK(g.a0 >= 0 && g.a0 <= g.a1 && (size_t)g.a1 <= nasm && g.bofs + g.nf - g.ns <= T.bdry_total);
    CHECK(g.iofs < 0 || (size_t)g.iofs + 2 * (size_t)(g.nf + 1) <= P.premap.pinv.size());
    CHECK(g.fofs < 0 || (size_t)g.fofs + (size_t)(g.nf - g.ns + 1) <= P.premap.fwd.size());
    CHECK(g.eoff < 0 || g.eoff + (long long)g.pld * (g.pld - 1) <= P.premap.slab_doubles);
  }
  for (size_t e = 0; e < nasm; ++e) CHECK(P.asrc[e] >= 0 && P.apos[e] >= 0);
  for (const Launch& L : P.chain) {
    size_t have = 0;
    switch (L.kind) {
      case Kind::Leaf: case Kind::Bwd256: case Kind::Bwd1024: have = P.lists.size(); break;
      case Kind::Single: case Kind::SingleNarrow: case Kind::SingleDense: case Kind::SingleDenseNarrow: have = P.singles.size(); break;
      case Kind::Start: have = P.starts.size(); break;
      case Kind::Step: case Kind::Step2: case Kind::Panel2: case Kind::Update2: have = P.tiles.size(); break;
      case Kind::BwdRect: have = P.rects.size(); break;
      case Kind::BwdFused: have = (size_t)P.fused.nwg; break;
    }
    CHECK(L.ofs >= 0 && L.cnt >= 1 && (size_t)L.ofs + (size_t)L.cnt <= have);
    CHECK(L.block >= 64 && L.block <= 1024 && L.lds <= 160 * 1024 && L.npiv >= 0 && L.npiv <= L.cnt);
  }
  for (int t : P.lists) CHECK(t >= 0 && t < nn);
  for (const StartJob& j : P.starts)
    CHECK(j.node >= 0 && j.node < nn && j.off == P.nodes[j.node].off && j.a0 >= 0 && j.a0 <= j.a1 && (size_t)j.a1 <= nasm && j.rb >= -1 &&
          j.soff[0] >= 0 && j.soff[1] >= 0 && j.soff[0] <= P.premap.slab_doubles && j.soff[1] <= P.premap.slab_doubles);
  for (const StepTile& s : P.tiles)
    CHECK(s.pad >= 0 && s.pad < nn && s.off == P.nodes[s.pad].off && s.tj >= 0 && s.tj <= s.ti && (s.ti + 1) * TS <= s.nf + 1 + TS);
  for (const SingleTile& u : P.singles)
    CHECK(u.off >= 0 && u.off < T.front_doubles && u.tj >= 0 && u.tj <= u.ti && u.a0 <= u.a1 && (size_t)u.a1 <= nasm && u.soff[0] >= 0 &&
          u.soff[1] >= 0);
  for (const RectJob& r : P.rects) CHECK(r.node >= 0 && r.node < nn && r.chunk >= 0 && r.chunk * 64 < P.nodes[r.node].ns);
}

static void check_grid(int nx, int ny) {
  const int N = nx * ny;
  std::vector<Triplet> t;
  std::vector<double> coords((size_t)N * 2);
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {      // the pattern of mgb_chol_selftest: 5-point stencil plus one diagonal neighbour
      const int r = j * nx + i;
      coords[2 * r] = i;
      coords[2 * r + 1] = j;
      t.push_back({r, r, 1.0});
      if (i > 0) t.push_back({r, r - 1, 1.0});
      if (j > 0) t.push_back({r, r - nx, 1.0});
      if (i > 0 && j > 0) t.push_back({r, r - nx - 1, 1.0});
    }
  const Csr Lo = from_triplets(N, N, t);
  for (const Variant& v : variants()) {
    if (v.leaf) setenv("MGB_LEAF", v.leaf, 1);
    else unsetenv("MGB_LEAF");
    MfChol ch;
    ch.analyze(Lo, coords.data(), 2);
    const CholTree T = ch.view();
    size_t launches = 0;
    for (int world : {1, 2, 4}) {
      const CholPartition part = world > 1 ? ch.partition(world) : CholPartition();
      CHECK(part.world == world);
      for (int rank = 0; rank < world; ++rank) {
        const ChainPlan P = plan_chain(T, part, rank, v.kn);
        check_plan(T, P, world > 1);
        if (world == 1) launches = P.chain.size();
      }
    }
    std::printf("%4d x %-4d %-24s nodes %5d  heights %2d  max front %4d  launches %3zu\n", nx, ny, v.name, T.size(), T.nheights, T.max_nf,
                launches);
  }
}

int main() {
  check_grid(47, 31);
  check_grid(160, 130);
  if (failures) {
    std::fprintf(stderr, "chol_plan_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("chol_plan_host_check ok\n");
  return 0;
}
