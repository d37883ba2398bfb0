// Stand-alone check of the host code behind mixed boundary conditions: mixed::dirichlet_on, the
// incidence table and the host restatement of the Neumann load, over fem1d, fem2d with and without K, fem3d k = 1..3 at
// L <= 3, and the refused inputs.  Meant to be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I multigridbarriermpi.jl_amd/csrc \
//       tools/mixed_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp -o tools/_bin/mixed_host_check
// Exit status 0 and "mixed_host_check ok" when every property holds.
#include <cstdio>
#include <cstdlib>

#include "mixed.hpp"

using namespace mgb;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static bool same(const Csr& a, const Csr& b) {
  return a.rows == b.rows && a.cols == b.cols && a.rowptr == b.rowptr && a.colidx == b.colidx && a.vals == b.vals;
}

template <class F>
static bool refused(F&& fn) {
  try {
    fn();
  } catch (const ArgError&) {
    return true;
  }
  return false;
}

static void check_geometry(const char* name, GeometryHost g) {
  const boundary::Facets F = boundary::build_facets(g);
  const boundary::Incidence I = boundary::build_incidence(F);
  const int nb = I.nb(), m = F.nf * F.q;
  CHECK((int)I.start.size() == nb + 1 && (int)I.idx.size() == m && I.start.front() == 0 && I.start.back() == m);
  std::vector<int> seen((size_t)m, 0);
  for (int r = 0; r < nb; ++r) {
    CHECK(r == 0 || I.rows[r] > I.rows[r - 1]);
    CHECK(I.start[r + 1] > I.start[r]);
    for (int t = I.start[r]; t < I.start[r + 1]; ++t) {
      CHECK(F.nodes[I.idx[t]] == I.rows[r]);
      CHECK(t == I.start[r] || I.idx[t] > I.idx[t - 1]);
      seen[I.idx[t]]++;
    }
  }
  for (int t = 0; t < m; ++t) CHECK(seen[t] == 1);
  // subspaces: every facet = dirichlet, none = full, one side in between; kept columns vanish on the pinned rows
  std::vector<unsigned char> all((size_t)F.nf, 1), none((size_t)F.nf, 0), side((size_t)F.nf, 0);
  double lo = 1e300;
  for (int f = 0; f < F.nf; ++f) lo = std::min(lo, F.centre[(size_t)f * F.dim]);
  for (int f = 0; f < F.nf; ++f) side[f] = F.centre[(size_t)f * F.dim] < lo + 1e-9;
  mixed::dirichlet_on(g, "every", nullptr);
  mixed::dirichlet_on(g, "every2", all.data());
  mixed::dirichlet_on(g, "nothing", none.data());
  mixed::dirichlet_on(g, "side", side.data());
  const std::vector<unsigned char> pinned = mixed::pinned_rows(g.n, F, side.data());
  for (int l = 0; l < g.L; ++l) {
    CHECK(same(g.subspaces["every"][l], g.subspaces["dirichlet"][l]));
    CHECK(same(g.subspaces["every2"][l], g.subspaces["dirichlet"][l]));
    CHECK(same(g.subspaces["nothing"][l], g.subspaces["full"][l]));
    const Csr& S = g.subspaces["side"][l];
    CHECK(S.rows == g.n && S.cols <= g.subspaces["full"][l].cols && S.cols >= g.subspaces["dirichlet"][l].cols);
    for (int r = 0; r < S.rows; ++r)
      for (int e = S.rowptr[r]; e < S.rowptr[r + 1]; ++e) {
        CHECK(S.colidx[e] >= 0 && S.colidx[e] < S.cols);
        CHECK(!pinned[r] || S.vals[e] == 0.0);
      }
  }
  // refused: taken names, a name already present
  for (const char* bad : {"full", "dirichlet", "fixed", "", "a:b", "side"})
    CHECK(refused([&] { mixed::dirichlet_on(g, bad, nullptr); }));
  // load: h = 1 integrates to the measure; masked-out NaN is not read; an empty selection gives zeros
  boundary::LoadArgs A;
  A.rows = I.rows.data(), A.start = I.start.data(), A.idx = I.idx.data();
  A.weights = F.weights.data(), A.w = g.w.data();
  A.nb = nb, A.nf = F.nf, A.q = F.q;
  const int B = 3;
  std::vector<double> h((size_t)B * m, 1.0), out((size_t)B * nb, 7.0);
  boundary::boundary_load_host(A, B, h.data(), out.data());
  const double want = g.dim == 1 ? 2.0 : g.dim == 2 ? 8.0 : 24.0;
  for (int b = 0; b < B; ++b) {
    double total = 0.0;
    for (int r = 0; r < nb; ++r) total += g.w[I.rows[r]] * out[(size_t)b * nb + r];
    CHECK(std::fabs(total - want) <= 1e-12 * want);
  }
  A.mask = side.data();
  std::vector<double> clean((size_t)B * nb), dirty((size_t)B * nb);
  boundary::boundary_load_host(A, B, h.data(), clean.data());
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < F.nf; ++f)
      if (!side[f])
        for (int j = 0; j < F.q; ++j) h[((size_t)b * F.nf + f) * F.q + j] = std::numeric_limits<double>::quiet_NaN();
  boundary::boundary_load_host(A, B, h.data(), dirty.data());
  CHECK(clean == dirty);
  A.mask = none.data();
  boundary::boundary_load_host(A, B, h.data(), out.data());
  for (double v : out) CHECK(v == 0.0);
  std::printf("%-16s n %6d  L %d  facets %5d x %2d  boundary rows %5d  side columns", name, g.n, g.L, F.nf, F.q, nb);
  for (int l = 0; l < g.L; ++l) std::printf(" %d", g.subspaces["side"][l].cols);
  std::printf("\n");
}

int main() {
  const double Lshape[] = {-1, -1, 0, -1, 0, 0, -1, -1, 0, 0, -1, 0, 0, -1, 1, -1, 1, 0, 0, -1, 1, 0, 0, 0, -1, 0, 0, 0, 0, 1, -1, 0, 0, 1, -1, 1};
  for (int L = 1; L <= 3; ++L) {
    char name[64];
    std::snprintf(name, sizeof name, "fem1d L=%d", L);
    check_geometry(name, fem1d_native(L));
    std::snprintf(name, sizeof name, "fem2d L=%d", L);
    check_geometry(name, fem2d_native(L, nullptr, 0));
    std::snprintf(name, sizeof name, "fem2d K L=%d", L);
    check_geometry(name, fem2d_native(L, Lshape, 18));
    for (int k = 1; k <= 3; ++k) {
      std::snprintf(name, sizeof name, "fem3d k=%d L=%d", k, L);
      check_geometry(name, fem3d_native(L, k));
    }
  }
  // refused geometries: no full subspace; a level of it missing
  GeometryHost g = fem1d_native(2);
  GeometryHost no_full = g;
  no_full.subspaces.erase("full");
  CHECK(refused([&] { mixed::dirichlet_on(no_full, "m", nullptr); }));
  GeometryHost short_full = g;
  short_full.subspaces["full"].pop_back();
  CHECK(refused([&] { mixed::dirichlet_on(short_full, "m", nullptr); }));
  GeometryHost empty_level = g;
  empty_level.subspaces["full"][0] = Csr();
  CHECK(refused([&] { mixed::dirichlet_on(empty_level, "m", nullptr); }));
  CHECK(!no_full.subspaces.count("m") && !short_full.subspaces.count("m") && !empty_level.subspaces.count("m"));
  if (failures) {
    std::fprintf(stderr, "mixed_host_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("mixed_host_check ok\n");
  return 0;
}
