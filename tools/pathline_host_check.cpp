// Stand-alone check of the per-seed routine behind path_lines: pathline::advance<DIM, K>, the code the
// gfx950 kernel and the host restatement both run, over fem2d L = 1..4, the L shape and fem3d k = 1..3 at L = 1, 2, through
// B = 4 snapshots (two constants, a quadratic and an oscillating field, so that particles rest, move and leave), both
// directions, p = 1, 2, 1.5, 1.75, substeps = 1, 3, 8, every release index, from a grid of seeds that reaches past the mesh and
// holds a NaN and an Inf, and once more with a NaN node in the last snapshot.  Every output of a row lives in a heap block of
// exactly its size (the path row: (stop - release) substeps + 2 slots), so a write beyond it is a sanitizer report.  Meant to
// be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I multigridbarriermpi.jl_amd/csrc tools/pathline_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp \
//       -o tools/_bin/pathline_host_check
// Exit status 0 and "pathline_host_check ok" when every property holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "pathline.hpp"

using namespace mgb;

static int failures = 0;
static long long particles = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

template <int DIM, int K>
static void check_mesh(const GeometryHost& g) {
  const interp::Locator L = interp::build_locator(g);
  const int S = 2, per = DIM == 2 ? 7 : 4, B = 4;
  std::vector<double> z[B + 1];
  for (int f = 0; f <= B; ++f) {
    z[f].assign((size_t)g.n * S, 0.25);
    for (int i = 0; i < g.n; ++i) {
      const double* x = &g.x[(size_t)i * DIM];
      double r2 = 0.0, s = 1.0;
      for (int d = 0; d < DIM; ++d) {
        r2 += x[d] * x[d];
        s *= std::sin(2.3 * x[d] + 0.4 * d);
      }
      z[f][(size_t)i * S + 1] = f <= 1 ? 0.5 : f == 2 ? r2 + x[0] - 0.5 * x[DIM - 1] : s;
    }
  }
  z[B][(size_t)(g.n / 2) * S + 1] = std::numeric_limits<double>::quiet_NaN();      // the oscillating field with a NaN node
  const double ts[B] = {0.0, 0.25, 0.375, 1.0};
  std::vector<double> seeds;
  int m = 1;
  for (int d = 0; d < DIM; ++d) m *= per;
  for (int i = 0; i < m; ++i) {
    int r = i;
    for (int d = 0; d < DIM; ++d) {
      seeds.push_back(-1.23 + 2.46 * ((r % per) + 0.37) / per);      // some outside [-1, 1]^DIM
      r /= per;
    }
  }
  for (int d = 0; d < DIM; ++d) seeds.push_back(d == 0 ? std::numeric_limits<double>::quiet_NaN() : 0.1);
  for (int d = 0; d < DIM; ++d) seeds.push_back(d == DIM - 1 ? std::numeric_limits<double>::infinity() : 0.1);
  m += 2;
  const double ps[4] = {1.0, 2.0, 1.5, 1.75};
  const int subs[3] = {1, 3, 8};
  for (int poisoned = 0; poisoned < 2; ++poisoned) {
    const double* table[B] = {z[0].data(), z[1].data(), z[2].data(), z[poisoned ? B : 3].data()};
    for (int c = 0; c < 4; ++c)
      for (int stop = 1; stop < B; ++stop)
        for (int rel = 0; rel < stop; ++rel)
          for (double sgn : {1.0, -1.0}) {
            const int n = subs[(c + stop + rel) % 3];
            pathline::Args A{};
            A.own = L.view(L.cellptr.data(), L.cellelem.data(), g.x.data());
            A.z = table, A.ts = ts;
            A.p = ps[c], A.sgn = sgn, A.speed = c == 1 ? 0.5 : 2.0, A.gmin = 1e-12;
            A.m = m, A.S = S, A.u = 1, A.B = B, A.stop = stop, A.substeps = n;
            A.stride = (long long)(stop - rel) * n + 2;
            const int most = (stop - rel) * n;
            for (int i = 0; i < m; ++i) {
              std::unique_ptr<double[]> row(new double[pathline::kRowCols]), end(new double[DIM]);
              std::unique_ptr<double[]> pts(new double[(size_t)A.stride * DIM]);
              std::unique_ptr<int32_t[]> pel(new int32_t[(size_t)A.stride]), st(new int32_t[1]), cnt(new int32_t[1]), ee(new int32_t[1]),
                  rs(new int32_t[1]);
              pathline::advance<DIM, K>(A, &seeds[(size_t)i * DIM], rel, row.get(), end.get(), st.get(), cnt.get(), ee.get(), rs.get(),
                                        pts.get(), pel.get());
              ++particles;
              CHECK(st[0] >= pathline::kDone && st[0] <= pathline::kNonFinite);
              CHECK(cnt[0] >= 0 && cnt[0] <= most + 1);
              if (st[0] == pathline::kOutside) {
                CHECK(cnt[0] == 0 && ee[0] == -1 && rs[0] == 0 && row[0] != row[0] && row[4] != row[4] && end[0] != end[0]);
                continue;
              }
              CHECK(i < m - 2);      // the NaN and the Inf seed are outside
              CHECK(ee[0] >= 0 && ee[0] < L.nel && cnt[0] >= 1 && row[0] >= 0.0 && row[4] >= 0.0 && row[4] <= row[0]);
              CHECK(rs[0] >= 0 && rs[0] <= most);
              CHECK(row[1] >= ts[rel] && row[1] <= ts[stop]);
              for (int j = 0; j < cnt[0]; ++j) CHECK(pel[j] >= 0 && pel[j] < L.nel);
              for (int d = 0; d < DIM; ++d) {
                CHECK(pts[d] == seeds[(size_t)i * DIM + d]);
                CHECK(end[d] == pts[(size_t)(cnt[0] - 1) * DIM + d]);
              }
              if (st[0] == pathline::kDone) CHECK(cnt[0] == most + 1 && row[1] == ts[stop]);
              if (rel == 0 && st[0] == pathline::kDone) CHECK(rs[0] >= n);      // the first slab lies between two constants
              if (!poisoned) CHECK(st[0] != pathline::kNonFinite);
              // the same particle without paths: the same row
              std::unique_ptr<double[]> row2(new double[pathline::kRowCols]), end2(new double[DIM]);
              pathline::advance<DIM, K>(A, &seeds[(size_t)i * DIM], rel, row2.get(), end2.get(), st.get(), cnt.get(), ee.get(), rs.get(),
                                        nullptr, nullptr);
              for (int k = 0; k < pathline::kRowCols; ++k) CHECK(row2[k] == row[k] || (row2[k] != row2[k] && row[k] != row[k]));
            }
          }
  }
}

int main() {
  for (int L = 1; L <= 4; ++L) check_mesh<2, 0>(fem2d_native(L, nullptr, 0));
  const double lshape[] = {-1, -1, 0, -1, -1, 0, 0, -1, 0, 0, -1, 0, 0, -1, 1, -1, 0, 0, 1, -1, 1, 0, 0, 0, -1, 0, 0, 0, -1, 1, 0, 0, 0, 1, -1, 1};
  check_mesh<2, 0>(fem2d_native(3, lshape, 18));
  for (int L = 1; L <= 2; ++L) {
    check_mesh<3, 1>(fem3d_native(L, 1));
    check_mesh<3, 2>(fem3d_native(L, 2));
    check_mesh<3, 3>(fem3d_native(L, 3));
  }
  if (failures) {
    std::fprintf(stderr, "pathline_host_check: %d failures\n", failures);
    return 1;
  }
  std::printf("pathline_host_check ok (%lld particles)\n", particles);
  return 0;
}
