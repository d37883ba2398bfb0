// Stand-alone check of the per-segment routine behind line_integrals: ray::integrate<DIM, K>, the code the
// gfx950 kernels and the host restatement both run, over fem2d L = 1..4 and fem3d k = 1..3 at L = 1, 2, 3, on a smooth field, a
// field with a NaN node and one with an Inf node, p = 1, 1.5, 2, along segments that lie in faces, along edges, through
// vertices, within tau of a face, inside one element, outside, with a == b and with non-finite ends, and along seeded random
// chords.  Every output -- the row of 8 doubles, the count, the pieces and their elements -- lives in a heap block of exactly
// its size, the end points in blocks of exactly DIM doubles and the fields in blocks of exactly n x S doubles, so a read or
// write beyond them is a sanitizer report; the pieces are written in a second pass into blocks of exactly `count` rows.
// Meant to be built with a sanitizer and run on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I multigridbarriermpi.jl_amd/csrc tools/ray_host_check.cpp multigridbarriermpi.jl_amd/csrc/geometry.cpp \
//       -o tools/_bin/ray_host_check
// Exit status 0 and "ray_host_check ok" when every property holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

#include "ray.hpp"

using namespace mgb;

static int failures = 0;
static long long rays_run = 0, pieces_seen = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static double uniform(unsigned long long& s) {      // a 64-bit LCG: the same chords on every run
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) / 9007199254740992.0;
}

template <int DIM, int K>
static void check_mesh(const GeometryHost& g) {
  const interp::Locator L = interp::build_locator(g);
  const int S = 2;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // a, b per segment, three coordinates each (the third unused in 2-D)
  std::vector<std::vector<double>> segs = {
      {-1.2, 0.0, 0.0, 1.2, 0.0, 0.0},      {-0.9, 1.0, 1.0, 0.8, 1.0, 1.0},     {0.0, -1.0, 0.0, 0.0, 1.0, 0.0},
      {-1.0, -0.7, -1.0, -1.0, 0.9, -1.0},  {-0.8, 1e-13, 0.1, 0.9, 1e-13, 0.2}, {-0.8, -1e-13, 0.1, 0.9, -1e-13, 0.2},
      {-0.9, 0.0, 0.0, 0.9, 1.8e-11, 0.0},  {-1.0, -1.0, -1.0, 1.0, 1.0, 1.0},   {-1.0, 1.0, -1.0, 1.0, -1.0, 1.0},
      {0.10, 0.02, 0.07, 0.20, 0.04, 0.21}, {1.5, 1.5, 0.0, 2.0, 3.0, 0.5},      {-2.0, 1.5, 0.2, 2.0, 1.5, 0.3},
      {0.3, 0.3, 0.3, 0.3, 0.3, 0.3},       {nan, 0.0, 0.0, 0.5, 0.1, 0.0},      {0.0, inf, 0.0, 0.5, 0.1, 0.0},
      {-0.5, 0.1, 0.2, 0.5, -inf, 0.2},     {-1e300, 0.1, 0.2, 1e300, 0.1, 0.2}, {-3.0, 0.1, 0.1, 3.0, 0.1, 0.1}};
  unsigned long long seed = 12345u + 7u * DIM + K;
  for (int r = 0; r < 40; ++r) {
    std::vector<double> s(6);
    for (double& v : s) v = -1.3 + 2.6 * uniform(seed);
    segs.push_back(s);
  }
  ray::Args A;
  A.own = L.view(L.cellptr.data(), L.cellelem.data(), g.x.data());
  A.S = S, A.u = 1, A.B = 1, A.m = 1;
  for (int f = 0; f < 3; ++f) {
    std::unique_ptr<double[]> z(new double[(size_t)g.n * S]);
    for (int i = 0; i < g.n; ++i) {
      const double* x = &g.x[(size_t)i * DIM];
      z[(size_t)i * S] = 0.25;
      z[(size_t)i * S + 1] = std::sin(3.0 * x[0] + 0.5) * std::cos(2.0 * x[1]) + 0.3 * x[0] * x[DIM - 1];
    }
    if (f == 1) z[(size_t)(g.n / 2) * S + 1] = nan;
    if (f == 2) z[(size_t)(g.n - 1) * S + 1] = inf;
    const double ps[3] = {1.0, 1.5, 2.0};
    for (double p : ps)
      for (size_t si = 0; si < segs.size(); ++si) {
        std::unique_ptr<double[]> a(new double[DIM]), b(new double[DIM]), row(new double[ray::kCols]);
        std::unique_ptr<int32_t> count(new int32_t(-7));
        for (int d = 0; d < DIM; ++d) {
          a[d] = segs[si][d];
          b[d] = segs[si][3 + d];
        }
        for (int c = 0; c < ray::kCols; ++c) row[c] = 7.0;
        A.p = p;
        ray::integrate<DIM, K>(A, z.get(), a.get(), b.get(), row.get(), count.get(), nullptr, nullptr, 0);
        ++rays_run;
        const int n = *count;
        CHECK(n >= 0 && n <= L.nel);
        if (n < 0) continue;
        // the second pass: pieces into blocks of exactly n rows (a null block for n = 0), nothing else written
        std::unique_ptr<double[]> piece(n ? new double[(size_t)n * ray::kPieceWidth] : nullptr);
        std::unique_ptr<int32_t[]> elem(n ? new int32_t[n] : nullptr);
        if (n) ray::integrate<DIM, K>(A, z.get(), a.get(), b.get(), nullptr, nullptr, piece.get(), elem.get(), n);
        pieces_seen += n;
        double ell = 0.0;
        for (int d = 0; d < DIM; ++d) ell += (b[d] - a[d]) * (b[d] - a[d]);
        ell = std::sqrt(ell);
        if (n == 0) {
          CHECK(row[0] == 0.0 && row[1] == 0.0 && row[2] == 0.0 && row[3] == 0.0 && row[4] == -inf && row[5] == inf);
          CHECK(row[6] != row[6] && row[7] != row[7]);
          continue;
        }
        CHECK(si < 10 || si >= 17);                          // outside, a == b, non-finite or overflowing ends: no pieces
        CHECK(row[0] > 0.0 && row[6] >= 0.0 && row[7] <= 1.0 && row[7] > row[6]);
        // the pieces overlap by tau / |beta| at most: next to nothing, except where the segment grazes a face (segment 6)
        if (si != 6) CHECK(row[0] <= (row[7] - row[6]) * ell * (1.0 + 1e-9) + 1e-9);
        if (DIM == 3) CHECK(row[3] == 0.0 || row[3] != row[3]);
        const bool poisoned = row[1] != row[1];
        CHECK(f > 0 || !poisoned);
        if (poisoned) CHECK(row[2] != row[2] && row[3] != row[3] && row[4] != row[4] && row[5] != row[5]);
        else CHECK(interp::finite(row[1]) && interp::finite(row[2]) && interp::finite(row[3]) && row[5] <= row[4]);
        double len = 0.0, sum = 0.0, lo = 2.0, hi = -1.0;
        for (int q = 0; q < n; ++q) {
          const double t0 = piece[(size_t)q * 3], t1 = piece[(size_t)q * 3 + 1];
          CHECK(elem[q] >= 0 && elem[q] < L.nel && t1 > t0 && t0 >= 0.0 && t1 <= 1.0);
          for (int q2 = 0; q2 < q; ++q2) CHECK(elem[q2] != elem[q]);
          len += (t1 - t0) * ell;
          sum += piece[(size_t)q * 3 + 2];
          lo = t0 < lo ? t0 : lo;
          hi = t1 > hi ? t1 : hi;
        }
        CHECK(len == row[0] && lo == row[6] && hi == row[7]);
        if (!poisoned) CHECK(sum == row[1]);
        // spanning chords of [-1, 1]^DIM
        if (si == 17) CHECK(std::fabs(row[0] - 2.0) <= 1e-10);
        if (si == 7 || si == 8) CHECK(std::fabs(row[0] - 2.0 * std::sqrt((double)DIM)) <= 1e-10);
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
    std::fprintf(stderr, "ray_host_check: %d failures\n", failures);
    return 1;
  }
  std::printf("ray_host_check ok (%lld rays, %lld pieces)\n", rays_run, pieces_seen);
  return 0;
}
