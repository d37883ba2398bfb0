// Stand-alone check of the per-item routine behind sections: section::item<DIM, K>, the code the gfx950
// kernels and the host restatement both run, over fem2d L = 1..4 and fem3d k = 1..3 at L = 1, 2, 3, on a smooth field, a field
// with a NaN node and one with an Inf node, p = 1, 1.5, 2, against planes that are axis-aligned, tilted, on element faces, on the
// faces of the Kuhn tetrahedra, on the boundary and outside.  Every Term lives in a heap block of exactly its size and the
// fields in blocks of exactly n x S doubles, so a read or write beyond them is a sanitizer report.  Meant to be built with a
// sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I multigridbarriermpi.jl_amd/csrc tools/section_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp \
//       -o tools/_bin/section_host_check
// Exit status 0 and "section_host_check ok" when every property holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "section.hpp"

using namespace mgb;

static int failures = 0;
static long long items_run = 0, pieces_seen = 0;
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
  const int S = 2, W = section::piece_width(DIM);
  const double planes[7][4] = {{0.0, 0.0, 1.0, 0.3}, {1.0, 0.5, 0.25, 0.05}, {1.0, 0.0, 0.0, 0.0}, {1.0, -1.0, 0.0, 0.0},
                               {1.0, 0.0, 0.0, -1.0}, {1.0, 0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 2.0}};
  const double full[2] = {DIM == 2 ? 2.0 : 4.0, DIM == 2 ? 2.0 * std::sqrt(1.25) : 4.0 * std::sqrt(1.3125)};      // planes 0, 1
  section::Args A;
  A.own = L.view(nullptr, nullptr, g.x.data());
  A.nel = L.nel, A.S = S, A.u = 1, A.B = 1, A.nc = 1;
  A.items = section::items_per_row(DIM, L.nel);
  for (int f = 0; f < 3; ++f) {
    std::unique_ptr<double[]> z(new double[(size_t)g.n * S]);
    for (int i = 0; i < g.n; ++i) {
      const double* x = &g.x[(size_t)i * DIM];
      z[(size_t)i * S] = 0.25;
      z[(size_t)i * S + 1] = std::sin(3.0 * x[0] + 0.5) * std::cos(2.0 * x[1]) + 0.3 * x[0] * x[DIM - 1];
    }
    if (f == 1) z[(size_t)(g.n / 2) * S + 1] = std::numeric_limits<double>::quiet_NaN();
    if (f == 2) z[(size_t)(g.n - 1) * S + 1] = std::numeric_limits<double>::infinity();
    const double ps[3] = {1.0, 1.5, 2.0};
    for (double p : ps)
      for (int l = 0; l < 7; ++l) {
        // in 2-D the first two components of the normal (plane 0: the line y = 0.3) and the offset
        double plane[DIM + 1];
        for (int d = 0; d < DIM; ++d) plane[d] = planes[l][d];
        if (DIM == 2 && l == 0) plane[1] = 1.0;
        plane[DIM] = planes[l][3];
        A.p = p;
        double measure = 0.0;
        bool poisoned = false;
        long long count = 0;
        for (long long it = 0; it < A.items; ++it) {
          std::unique_ptr<section::Term<DIM>> T(new section::Term<DIM>);
          section::item<DIM, K>(A, z.get(), plane, it, *T);
          ++items_run;
          CHECK(T->emit >= 0 && T->emit <= (DIM == 2 ? 1 : 2));
          if (T->c[0] != T->c[0]) {
            poisoned = true;
            CHECK(T->emit == 0 && T->c[1] != T->c[1] && T->c[2] != T->c[2] && T->c[3] != T->c[3] && T->c[4] != T->c[4]);
            continue;
          }
          CHECK(T->c[0] >= 0.0 && (T->emit > 0) == (T->c[0] > 0.0 || T->c[3] > -std::numeric_limits<double>::infinity()));
          if (T->emit == 0) CHECK(T->c[0] == 0.0 && T->c[1] == 0.0 && T->c[2] == 0.0 && T->c[3] < 0.0 && T->c[4] < 0.0 && std::isinf(T->c[3]));
          for (int q = 0; q < T->emit; ++q)
            for (int k = 0; k < W; ++k) CHECK(interp::finite(T->piece[q][k]));
          measure += T->c[0];
          count += T->emit;
        }
        pieces_seen += count;
        CHECK(f > 0 || !poisoned);
        if (l >= 5) CHECK(count == 0 && measure == 0.0);
        if (l < 2 && !poisoned) CHECK(std::fabs(measure - full[l]) <= 1e-12 * full[l]);
        if (l == 4 && !poisoned) CHECK(std::fabs(measure - full[0]) <= 1e-12 * full[0]);      // the boundary face x = -1, from inside
      }
  }
}

int main() {
  for (int L = 1; L <= 4; ++L) check_mesh<2, 0>(fem2d_native(L, nullptr, 0));
  for (int L = 1; L <= 3; ++L) {
    check_mesh<3, 1>(fem3d_native(L, 1));
    check_mesh<3, 2>(fem3d_native(L, 2));
    check_mesh<3, 3>(fem3d_native(L, 3));
  }
  if (failures) {
    std::fprintf(stderr, "section_host_check: %d failures\n", failures);
    return 1;
  }
  std::printf("section_host_check ok (%lld items, %lld pieces)\n", items_run, pieces_seen);
  return 0;
}
