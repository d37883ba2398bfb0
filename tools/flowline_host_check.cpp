// Stand-alone check of the per-seed routine behind flow_lines: flowline::trace<DIM, K>, the code the
// gfx950 kernel and the host restatement both run, over fem2d L = 1..4 and fem3d k = 1..3 at L = 1, 2, on a linear, a quadratic
// and an oscillating field, both directions, p = 1, 2, 1.5, max_steps = 1, 7, 200, from a grid of seeds that reaches past the
// mesh and holds a NaN and an Inf.  Every output of a row lives in a heap block of exactly its size (the path row: max_steps + 2
// slots), so a write beyond it is a sanitizer report.  Meant to be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I multigridbarriermpi.jl_amd/csrc tools/flowline_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp \
//       -o tools/_bin/flowline_host_check
// Exit status 0 and "flowline_host_check ok" when every property holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "flowline.hpp"

using namespace mgb;

static int failures = 0;
static long long lines_traced = 0;
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
  CHECK(L.min_extent > 0.0 && interp::finite(L.min_extent));
  const int S = 2, per = DIM == 2 ? 9 : 5;
  std::vector<double> z[3];
  for (int f = 0; f < 3; ++f) {
    z[f].assign((size_t)g.n * S, 0.25);
    for (int i = 0; i < g.n; ++i) {
      const double* x = &g.x[(size_t)i * DIM];
      double r2 = 0.0, s = 1.0;
      for (int d = 0; d < DIM; ++d) {
        r2 += x[d] * x[d];
        s *= std::sin(2.3 * x[d] + 0.4 * d);
      }
      z[f][(size_t)i * S + 1] = f == 0 ? x[0] - 0.5 * x[DIM - 1] : f == 1 ? r2 : s;
    }
  }
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
  const double ps[3] = {1.0, 2.0, 1.5};
  const int steps[3] = {1, 7, 200};
  for (int f = 0; f < 3; ++f)
    for (int c = 0; c < 3; ++c)
      for (double sgn : {1.0, -1.0}) {
        flowline::Args A{};
        A.own = L.view(L.cellptr.data(), L.cellelem.data(), g.x.data());
        A.p = ps[c], A.ds = 0.25 * L.min_extent, A.gmin = 1e-12, A.sgn = sgn;
        A.m = m, A.S = S, A.u = 1, A.B = 1, A.max_steps = steps[c];
        A.stride = (long long)steps[c] + 2;
        for (int i = 0; i < m; ++i) {
          std::unique_ptr<double[]> row(new double[flowline::kRowCols]), end(new double[DIM]);
          std::unique_ptr<double[]> pts(new double[(size_t)A.stride * DIM]);
          std::unique_ptr<int32_t[]> pel(new int32_t[(size_t)A.stride]), st(new int32_t[1]), cnt(new int32_t[1]), ee(new int32_t[1]);
          flowline::trace<DIM, K>(A, z[f].data(), &seeds[(size_t)i * DIM], row.get(), end.get(), st.get(), cnt.get(), ee.get(), pts.get(),
                                  pel.get());
          ++lines_traced;
          CHECK(st[0] >= flowline::kExit && st[0] <= flowline::kNonFinite);
          CHECK(cnt[0] >= 0 && cnt[0] <= steps[c] + 1);
          if (st[0] == flowline::kOutside) {
            CHECK(cnt[0] == 0 && ee[0] == -1 && row[0] != row[0] && end[0] != end[0]);
            continue;
          }
          CHECK(i < m - 2);      // the NaN and the Inf seed are outside
          CHECK(ee[0] >= 0 && ee[0] < L.nel && cnt[0] >= 1 && row[0] >= 0.0 && row[0] <= steps[c] * A.ds * (1.0 + 1e-12));
          for (int j = 0; j < cnt[0]; ++j) CHECK(pel[j] >= 0 && pel[j] < L.nel);
          for (int d = 0; d < DIM; ++d) {
            CHECK(pts[d] == seeds[(size_t)i * DIM + d]);
            CHECK(end[d] == pts[(size_t)(cnt[0] - 1) * DIM + d]);
          }
          if (st[0] == flowline::kMaxSteps) CHECK(cnt[0] == steps[c] + 1);
          // the same line without paths: the same row
          std::unique_ptr<double[]> row2(new double[flowline::kRowCols]), end2(new double[DIM]);
          flowline::trace<DIM, K>(A, z[f].data(), &seeds[(size_t)i * DIM], row2.get(), end2.get(), st.get(), cnt.get(), ee.get(), nullptr,
                                  nullptr);
          for (int k = 0; k < flowline::kRowCols; ++k) CHECK(row2[k] == row[k] || (row2[k] != row2[k] && row[k] != row[k]));
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
    std::fprintf(stderr, "flowline_host_check: %d failures\n", failures);
    return 1;
  }
  std::printf("flowline_host_check ok (%lld lines)\n", lines_traced);
  return 0;
}
