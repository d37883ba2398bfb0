// Level sets of nodal fields: what ONE item contributes, written ONCE.  The gfx950 kernels
// (levelset.hip) and the host restatement (mgb_geo_level_sets_host) both run item() below; tri_basis is interp.hpp's, combine
// and block_reduce are reduce.hpp's.
//   2-D (block 7: v1 v2 v3 m12 m23 m31 centroid).  ring = [v1, m12, v2, m23, v3, m31]; macro triangle k = 0..5 of element e has
//     corners A = ring[k], B = ring[(k+1) % 6], C = the centroid; with N = 2^refine it is cut into N^2 small triangles of the
//     lattice P(a,b) = A + (a/N)(B - A) + (b/N)(C - A).  Small triangle j: i = isqrt(j), q = j - i^2, b = N-1-i;
//     q even, a = q/2: (P(a,b), P(a+1,b), P(a,b+1));   q odd, a = (q-1)/2: (P(a+1,b), P(a+1,b+1), P(a,b+1)).
//     item = (e 6 + k) N^2 + j.  Lattice values: at refine = 0 the nodal values of A, B, C, loaded, and their coordinates,
//     loaded; at refine > 0 the P2 + bubble function at the lattice point's reference coordinates (the same formula on the
//     reference coordinates of A, B, C), positions by the formula on the coordinates of A, B, C.
//   1-D (block 2): one item per element, refine = 0.
//   A corner is above when v > c.  A crossing is interpolated from the BELOW corner to the ABOVE corner,
//     t = (c - v_lo) / (v_hi - v_lo), Q = P_lo + t (P_hi - P_lo): both elements at a shared edge compute the same bits.
//   Five contributions: measure of {u > c} | measure of {u = c} | int_{u > c} (u - c) | max (v - c) | max (c - v).
//   An item with a non-finite lattice value gives NaN in all five and emits nothing.
// The arithmetic is kept as written by ONE mechanism: levelset.hip, which holds the kernels AND the host restatement and is
// the only file that may instantiate item(), is compiled with -ffp-contract=off (build.sh).  That covers interp.hpp's
// tri_basis as well, which a pragma in the functions below would not; both sides run the same IEEE + - * / on the same operands.
#pragma once
#include <cstdint>

#include "interp.hpp"
#include "reduce.hpp"

namespace mgb {
namespace levelset {

using reduce::kCols;      // MGB_LEVELSET_COLS
using reduce::kThreads;
using reduce::kWaves;
using reduce::nanmax;
using reduce::combine;
using reduce::workgroups;

constexpr int kMaxRefine = 3;

// The identity of combine for THESE rows: both maxima may be negative (a level above every value gives max (v - c) < 0), so
// reduce::identity, whose column [3] starts at 0, and the finish launch that starts from it would clip them.
MGB_HD void no_items(double* c) {
  c[0] = c[1] = c[2] = 0.0;
  c[3] = c[4] = -std::numeric_limits<double>::infinity();
}
struct NoItems {      // what reduce.hpp's finish_row starts from here
  MGB_HD void operator()(double* c) const { no_items(c); }
};

// what all rows of one call share; every pointer is a host pointer or every pointer is a device pointer
struct Args {
  const double* x = nullptr;            // n x dim node coordinates
  const double* const* z = nullptr;     // B pointers to n x S fields
  const double* levels = nullptr;       // nl levels
  long long items = 0;                  // items per (field, level)
  int nel = 0, S = 0, u = 0, B = 0, nl = 0, refine = 0;
};

// items of one (field, level) row: 6 4^refine nel in 2-D, nel in 1-D
inline long long items_per_row(int dim, int nel, int refine) { return dim == 2 ? 6LL * (1LL << (2 * refine)) * nel : nel; }

// what one item gives: the five contributions, and the segment (2-D: x0 y0 x1 y1, the above side on its left; 1-D: x and
// the direction, +1 where u rises through c in +x) where emit is 1
struct Term {
  double c[kCols];
  double seg[4];
  int emit;
};

MGB_HD void poison(Term& T) {
  T.c[0] = T.c[1] = T.c[2] = T.c[3] = T.c[4] = std::numeric_limits<double>::quiet_NaN();
  T.emit = 0;
}

// the crossing of the level c on the edge from the below corner (lo) to the above corner (hi)
template <int DIM>
MGB_HD double crossing(const double* plo, double vlo, const double* phi, double vhi, double c, double* q) {
  const double t = (c - vlo) / (vhi - vlo);
#pragma unroll
  for (int d = 0; d < DIM; ++d) q[d] = plo[d] + t * (phi[d] - plo[d]);
  return t;
}

MGB_HD double cross2(double ax, double ay, double bx, double by) {
  return ax * by - ay * bx;
}

// the three lattice points of a 2-D item and their values
MGB_HD void lattice2d(const Args& A, const double* z, long long item, double (*P)[2], double* v) {
  const int N = 1 << A.refine, N2 = N * N;
  const int j = (int)(item % N2);
  const long long ek = item / N2;
  const int k = (int)(ek % 6);
  const size_t e = (size_t)(ek / 6);
  const int ring[6] = {0, 3, 1, 4, 2, 5};
  const int corner[3] = {ring[k], ring[k == 5 ? 0 : k + 1], 6};
  const double* xe = A.x + e * 14;
  const double* ze = z + e * 7 * A.S + A.u;
  if (A.refine == 0) {
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      P[m][0] = xe[2 * corner[m]];
      P[m][1] = xe[2 * corner[m] + 1];
      v[m] = ze[(size_t)corner[m] * A.S];
    }
    return;
  }
  int i = 0;
  while ((i + 1) * (i + 1) <= j) ++i;
  const int q = j - i * i, b = N - 1 - i, a = q >> 1;
  int la[3], lb[3];
  if ((q & 1) == 0) {
    la[0] = a, lb[0] = b, la[1] = a + 1, lb[1] = b, la[2] = a, lb[2] = b + 1;
  } else {
    la[0] = a + 1, lb[0] = b, la[1] = a + 1, lb[1] = b + 1, la[2] = a, lb[2] = b + 1;
  }
  // reference coordinates of the seven nodes of the block
  const double rx[7] = {0.0, 1.0, 0.0, 0.5, 0.5, 0.0, 1.0 / 3.0}, ry[7] = {0.0, 0.0, 1.0, 0.0, 0.5, 0.5, 1.0 / 3.0};
  const double* xa = xe + 2 * corner[0];
  const double* xb = xe + 2 * corner[1];
  const double* xc = xe + 2 * corner[2];
  const double rax = rx[corner[0]], ray = ry[corner[0]], rbx = rx[corner[1]], rby = ry[corner[1]], rcx = rx[6], rcy = ry[6];
  double zz[7];
#pragma unroll
  for (int n = 0; n < 7; ++n) zz[n] = ze[(size_t)n * A.S];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const double fa = (double)la[m] / (double)N, fb = (double)lb[m] / (double)N;
    P[m][0] = xa[0] + fa * (xb[0] - xa[0]) + fb * (xc[0] - xa[0]);
    P[m][1] = xa[1] + fa * (xb[1] - xa[1]) + fb * (xc[1] - xa[1]);
    const double xi = rax + fa * (rbx - rax) + fb * (rcx - rax), et = ray + fa * (rby - ray) + fb * (rcy - ray);
    double bas[7], dxi[7], det[7];
    interp::tri_basis(xi, et, bas, dxi, det);
    double acc = 0.0;
#pragma unroll
    for (int n = 0; n < 7; ++n) acc += bas[n] * zz[n];
    v[m] = acc;
  }
}

template <int DIM>
MGB_HD void item(const Args& A, const double* z, double c, long long it, Term& T);

template <>
MGB_HD void item<2>(const Args& A, const double* z, double c, long long it, Term& T) {
  double P[3][2], v[3];
  lattice2d(A, z, it, P, v);
  bool good = interp::finite(v[0]);
  good = good & interp::finite(v[1]);
  good = good & interp::finite(v[2]);
  if (!good) {
    poison(T);
    return;
  }
  T.emit = 0;
  T.c[0] = T.c[1] = T.c[2] = 0.0;
  T.c[3] = nanmax(nanmax(v[0] - c, v[1] - c), v[2] - c);
  T.c[4] = nanmax(nanmax(c - v[0], c - v[1]), c - v[2]);
  const bool up[3] = {v[0] > c, v[1] > c, v[2] > c};
  const int k_above = (int)up[0] + (int)up[1] + (int)up[2];
  if (k_above == 0) return;
  const double area = 0.5 * fabs(cross2(P[1][0] - P[0][0], P[1][1] - P[0][1], P[2][0] - P[0][0], P[2][1] - P[0][1]));
  const double mean_excess = (v[0] + v[1] + v[2]) / 3.0 - c;
  if (k_above == 3) {
    T.c[0] = area;
    T.c[2] = area * mean_excess;
    return;
  }
  // the lone corner: the one above (k_above = 1) or the one not above (k_above = 2)
  const bool want = k_above == 1;
  const int L = up[0] == want ? 0 : (up[1] == want ? 1 : 2), o1 = L == 2 ? 0 : L + 1, o2 = o1 == 2 ? 0 : o1 + 1;
  double Q0[2], Q1[2];
  if (k_above == 1) {
    crossing<2>(P[o1], v[o1], P[L], v[L], c, Q0);
    crossing<2>(P[o2], v[o2], P[L], v[L], c, Q1);
  } else {
    crossing<2>(P[L], v[L], P[o1], v[o1], c, Q0);
    crossing<2>(P[L], v[L], P[o2], v[o2], c, Q1);
  }
  const double* above = k_above == 1 ? P[L] : P[o1];
  const double a_s = 0.5 * fabs(cross2(Q0[0] - P[L][0], Q0[1] - P[L][1], Q1[0] - P[L][0], Q1[1] - P[L][1]));
  const double dx = Q1[0] - Q0[0], dy = Q1[1] - Q0[1];
  T.c[1] = sqrt(dx * dx + dy * dy);
  if (k_above == 1) {
    T.c[0] = a_s;
    T.c[2] = a_s * (v[L] - c) / 3.0;
  } else {
    T.c[0] = area - a_s;
    T.c[2] = area * mean_excess - a_s * (v[L] - c) / 3.0;
  }
  T.emit = !(k_above == 2 && v[L] == c);      // the zero-length segment at a lone corner on the level
  const bool swap = cross2(dx, dy, above[0] - Q0[0], above[1] - Q0[1]) < 0.0;
  T.seg[0] = swap ? Q1[0] : Q0[0];
  T.seg[1] = swap ? Q1[1] : Q0[1];
  T.seg[2] = swap ? Q0[0] : Q1[0];
  T.seg[3] = swap ? Q0[1] : Q1[1];
}

template <>
MGB_HD void item<1>(const Args& A, const double* z, double c, long long it, Term& T) {
  const size_t e = (size_t)it;
  const double xl = A.x[2 * e], xr = A.x[2 * e + 1];
  const double vl = z[(2 * e) * A.S + A.u], vr = z[(2 * e + 1) * A.S + A.u];
  bool good = interp::finite(vl);
  good = good & interp::finite(vr);
  if (!good) {
    poison(T);
    return;
  }
  T.emit = 0;
  T.c[0] = T.c[1] = T.c[2] = 0.0;
  T.c[3] = nanmax(vl - c, vr - c);
  T.c[4] = nanmax(c - vl, c - vr);
  const bool ul = vl > c, ur = vr > c;
  if (!ul && !ur) return;
  const double h = fabs(xr - xl);
  if (ul && ur) {
    T.c[0] = h;
    T.c[2] = h * ((vl + vr) / 2.0 - c);
    return;
  }
  const double plo = ur ? xl : xr, phi = ur ? xr : xl, vlo = ur ? vl : vr, vhi = ur ? vr : vl;
  double q;
  const double t = crossing<1>(&plo, vlo, &phi, vhi, c, &q);
  T.c[0] = (1.0 - t) * h;
  T.c[1] = 1.0;
  T.c[2] = 0.5 * (1.0 - t) * h * (vhi - c);
  T.emit = 1;
  T.seg[0] = q;
  T.seg[1] = phi > plo ? 1.0 : -1.0;
  T.seg[2] = T.seg[3] = 0.0;
}

// doubles of a segment row: x0 y0 x1 y1, or x and the direction
inline int seg_width(int dim) { return dim == 2 ? 4 : 2; }

// A serial sum whose error does not grow with the number of terms (Neumaier), for the host restatements: the items of a refined
// mesh have equal areas, so the roundings of a plain running sum all point the same way and reach 1e-12 of the sum near 2e5 items.
struct SerialSum {
  double s = 0.0, c = 0.0;
  void add(double v) {
    const double t = s + v;
    c += std::fabs(s) >= std::fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
  }
  double value() const { return s + c; }
};

// levelset.hip, host: the same per-item routine, serially, row after row (row = field * nl + level) in ascending item order.
// out: B nl x kCols; counts: B nl; row_offsets (nullable): B nl + 1; seg, item (both or neither; `capacity` rows): the
// emitted segments and their items.  Throws ArgError where the rows do not fit into capacity.
void level_sets_host(int dim, const Args& A, double* out, long long* counts, long long* row_offsets, double* seg, int32_t* item_out,
                     long long capacity);

// what the launches need, in 8-byte words of one device buffer, for rows = B nl and nwg workgroups per row:
//   partials rows x nwg x kCols | results rows x kCols | totals rows (long long)     <- results and totals: ONE copy to the host
// and of a second one, long long: counts rows x nwg | offsets rows x (nwg + 1)
inline size_t results_offset(size_t rows, size_t nwg) { return rows * nwg * kCols; }
inline size_t scratch_words(size_t rows, size_t nwg) { return rows * nwg * kCols + rows * kCols + rows; }
inline size_t offsets_offset(size_t rows, size_t nwg) { return rows * nwg; }
inline size_t count_words(size_t rows, size_t nwg) { return rows * nwg + rows * (nwg + 1); }

#if defined(__HIPCC__)
// levelset.hip: two launches on `stream` -- the measure on grid (workgroups(items), nl, B), then one workgroup per row that
// finishes the row's partials and scans its per-workgroup counts; all pointers of A are device pointers
void launch_measure(hipStream_t stream, int dim, const Args& A, double* scratch, long long* counts);
// the second of the two, on grid (rows), shared with isosurface.hip: row r folds its nwg partial rows (kCols doubles each, from
// NoItems) into results[r kCols ..] and turns its nwg counts into the nwg + 1 exclusive offsets at offsets[r (nwg + 1) ..], the
// total last and into totals[r]
void launch_finish(hipStream_t stream, int rows, const double* partials, const long long* counts, int nwg, double* results,
                   long long* offsets, long long* totals);
// one launch on the measure's grid: segment q of workgroup g of row r goes to slot row_base[r] + offsets[r (nwg + 1) + g] + q,
// slots beyond `total` are not written; seg: total x seg_width doubles, item_out: total int32
void launch_emit(hipStream_t stream, int dim, const Args& A, const long long* offsets, const long long* row_base, long long total,
                 double* seg, int32_t* item_out);
#endif

}  // namespace levelset
}  // namespace mgb
