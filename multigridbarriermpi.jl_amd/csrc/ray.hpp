// Line integrals of nodal fields: what ONE segment a -> b collects from the broken polynomial field of
// one column, written ONCE.  The gfx950 kernels (ray.hip) and the host restatement (mgb_geo_line_integrals_host) both run
// integrate() below.  Nothing here is new arithmetic: reference coordinates, the containment rule and the bin grid are
// interp.hpp's (ref_coords, find_element, cell_coord, kTau), value and gradient in a known element are flowline::value_grad,
// the Gauss tables, the number of points and sigma = a^(p-2) g with its case distinctions are section.hpp's.  The full rule is
// the comment of mgb_geo_line_integrals in include/mgb_hip.h; in short:
//   clip: the reference coordinates of a and b in element e make every constraint affine in t, g_j(t) = alpha_j + t beta_j;
//     e's interval is {t in [0, 1] : g_j(t) >= -tau for all j}, by comparisons alone; a piece needs t1 > t0;
//   ownership: the piece counts iff find_element(x((t0 + t1) / 2)) == e, the lowest element holding the midpoint;
//   walk: the segment clipped to the grown bounding box, cell layer after cell layer along the major axis, in each layer the
//     rectangle of cells the segment can touch; in cell c the elements whose piece has its midpoint in c;
//   quadrature: section::Gauss<N> on [t0, t1], N = section::gauss_points(DIM, K), rolled; extrema also at both piece ends.
// The arithmetic is kept as written by ONE mechanism: ray.hip, which holds the kernels AND the host restatement and is the
// only file that may instantiate integrate(), is compiled with -ffp-contract=off (build.sh).
#pragma once
#include <cstdint>
#include <limits>
#include <string>

#include "section.hpp"

namespace mgb {
namespace ray {

constexpr int kCols = 8;                  // MGB_RAY_COLS: length, integral, along, across, max, min, enter, leave
constexpr int kPieceWidth = 3;            // t0, t1, int u of a piece
constexpr double kSlack = 1e-9;           // the walk's slack, times the diagonal of the locator's bounding box

// what all rows of one call share; every pointer is a host pointer or every pointer is a device pointer
struct Args {
  interp::BinsView own;                   // the locator of the geometry
  const double* const* z = nullptr;       // B pointers to n x S fields
  const double* a = nullptr;              // m x dim start points
  const double* b = nullptr;              // m x dim end points
  double p = 2.0;                         // the exponent of sigma = |g|^(p-2) g
  int m = 0, S = 0, u = 0, B = 0;
  double* rows = nullptr;                 // B m x kCols
  int32_t* count = nullptr;               // B m
};

// the interval of element e on the segment whose end points have the reference coordinates ra, rb: true for a piece
template <int DIM>
MGB_HD bool clip(const double* ra, const double* rb, double& t0, double& t1) {
  constexpr int NG = DIM == 2 ? 3 : 6;
  double al[NG], be[NG];
  if constexpr (DIM == 2) {
    al[0] = 1.0 - ra[0] - ra[1];
    al[1] = ra[0];
    al[2] = ra[1];
    be[0] = (1.0 - rb[0] - rb[1]) - al[0];
    be[1] = rb[0] - ra[0];
    be[2] = rb[1] - ra[1];
  } else {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      al[2 * d] = ra[d];
      be[2 * d] = rb[d] - ra[d];
      al[2 * d + 1] = 1.0 - ra[d];
      be[2 * d + 1] = (1.0 - rb[d]) - al[2 * d + 1];
    }
  }
  t0 = 0.0;
  t1 = 1.0;
  bool some = true;
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const double s = al[j] + interp::kTau, q = -s / be[j];
    const bool up = be[j] > 0.0, down = be[j] < 0.0;
    t0 = (up & (q > t0)) ? q : t0;
    t1 = (down & (q < t1)) ? q : t1;
    // a constraint that does not move along the segment decides by its value; one that is not a number decides against
    some = some & (up | down | ((be[j] == 0.0) & !(s < 0.0))) & interp::finite(s);
  }
  return some & (t1 > t0);
}

// One segment a -> b through column A.u of field z: the row of kCols doubles and the number of owned pieces (both nullable
// together), and, with piece non-null, up to `cap` pieces (t0, t1, int u) with their elements in walk order.
template <int DIM, int K>
MGB_HD void integrate(const Args& A, const double* z, const double* a, const double* b, double* row, int32_t* count,
                      double* piece, int32_t* elem, long long cap) {
  constexpr int N = section::gauss_points(DIM, K);
  const interp::BinsView& V = A.own;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double length = 0.0, integral = 0.0, along = 0.0, across = 0.0, vmax = -inf, vmin = inf, enter = nan, leave = nan;
  int pieces = 0;
  bool good = true;
  double d[DIM], ell = 0.0;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    d[k] = b[k] - a[k];
    ell += d[k] * d[k];
    fin = fin & interp::finite(a[k]) & interp::finite(b[k]);
  }
  ell = sqrt(ell);
  fin = fin & interp::finite(ell) & (ell > 0.0);
  if (fin) {
    // the segment inside the bounding box of the bin grid, grown by the slack: [ta, tb]
    double hi[DIM], diag = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      hi[k] = V.lo[k] + (double)V.nc[k] / V.inv[k];
      diag += (hi[k] - V.lo[k]) * (hi[k] - V.lo[k]);
    }
    const double slack = kSlack * sqrt(diag);
    double ta = 0.0, tb = 1.0;
    bool in = true;
    int M = 0;
    double big = -1.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const double l = V.lo[k] - slack, h = hi[k] + slack;
      if (d[k] != 0.0) {
        const double q0 = (l - a[k]) / d[k], q1 = (h - a[k]) / d[k];
        const double qa = d[k] > 0.0 ? q0 : q1, qb = d[k] > 0.0 ? q1 : q0;
        ta = qa > ta ? qa : ta;
        tb = qb < tb ? qb : tb;
      } else {
        in = in & (a[k] >= l) & (a[k] <= h);
      }
      const double speed = fabs(d[k]) * V.inv[k];
      const bool more = speed > big;
      M = more ? k : M;
      big = more ? speed : big;
    }
    in = in & (tb >= ta);
    if (in) {
      // a, d, lo, inv, nc of the major axis and of the one or two other axes, by selects
      constexpr int NO = DIM - 1;
      const int O0 = M == 0 ? 1 : 0, O1 = M == 2 ? 1 : 2;
      double aM = a[0], dM = d[0], loM = V.lo[0], invM = V.inv[0];
      int ncM = V.nc[0], strideM = 1;
      double ao[2] = {0.0, 0.0}, dd[2] = {0.0, 0.0}, loo[2] = {0.0, 0.0}, invo[2] = {1.0, 1.0};
      int nco[2] = {1, 1}, strideo[2] = {0, 0};
      int stride = 1;
#pragma unroll
      for (int k = 0; k < DIM; ++k) {
        if (k == M) aM = a[k], dM = d[k], loM = V.lo[k], invM = V.inv[k], ncM = V.nc[k], strideM = stride;
        if (k == O0) ao[0] = a[k], dd[0] = d[k], loo[0] = V.lo[k], invo[0] = V.inv[k], nco[0] = V.nc[k], strideo[0] = stride;
        if (DIM == 3 && k == O1) ao[1] = a[k], dd[1] = d[k], loo[1] = V.lo[k], invo[1] = V.inv[k], nco[1] = V.nc[k], strideo[1] = stride;
        stride *= V.nc[k];
      }
      const double pa = aM + ta * dM, pb = aM + tb * dM;
      const bool fwd = dM > 0.0;
      const int first = interp::cell_coord((fwd ? pa : pb) - slack, loM, invM, ncM);
      const int last = interp::cell_coord((fwd ? pb : pa) + slack, loM, invM, ncM);
      const double tdir[3] = {d[0] / ell, d[1] / ell, DIM == 3 ? d[DIM - 1] / ell : 0.0};
      for (int step = 0; step <= last - first; ++step) {
        const int layer = fwd ? first + step : last - step;
        // the t-range of the layer, grown by the slack, inside [ta, tb]
        const double cl = loM + (double)layer / invM - slack, ch = loM + (double)(layer + 1) / invM + slack;
        const double ql = ((fwd ? cl : ch) - aM) / dM, qh = ((fwd ? ch : cl) - aM) / dM;
        const double tl = ql > ta ? ql : ta, th = qh < tb ? qh : tb;
        if (!(th >= tl)) continue;
        int c0[2] = {0, 0}, c1[2] = {0, 0};
#pragma unroll
        for (int o = 0; o < NO; ++o) {
          const double x0 = ao[o] + tl * dd[o], x1 = ao[o] + th * dd[o];
          const double xl = (x0 < x1 ? x0 : x1) - slack, xh = (x0 < x1 ? x1 : x0) + slack;
          c0[o] = interp::cell_coord(xl, loo[o], invo[o], nco[o]);
          c1[o] = interp::cell_coord(xh, loo[o], invo[o], nco[o]);
        }
        for (int j1 = c0[1]; j1 <= c1[1]; ++j1)
          for (int j0 = c0[0]; j0 <= c1[0]; ++j0) {
            const int cell = layer * strideM + j0 * strideo[0] + j1 * strideo[1];
            const int k1 = V.cellptr[cell + 1];
            for (int kk = V.cellptr[cell]; kk < k1; ++kk) {
              const int e = V.cellelem[kk];
              double ra[DIM], rb[DIM], t0, t1;
              interp::ref_coords<DIM>(V.x, V.block, e, a, ra);
              interp::ref_coords<DIM>(V.x, V.block, e, b, rb);
              if (!clip<DIM>(ra, rb, t0, t1)) continue;
              const double tm = 0.5 * (t0 + t1);
              double xm[DIM];
              int cm = 0, sm = 1;
#pragma unroll
              for (int k = 0; k < DIM; ++k) {
                xm[k] = a[k] + tm * d[k];
                cm += sm * interp::cell_coord(xm[k], V.lo[k], V.inv[k], V.nc[k]);
                sm *= V.nc[k];
              }
              if (cm != cell) continue;
              if (interp::find_element<DIM>(V, xm) != e) continue;
              // an owned piece: the Gauss points, then both ends (extrema only)
              const double dt = t1 - t0, len = dt * ell;
              double pu = 0.0, pal = 0.0, pac = 0.0;
#pragma unroll 1
              for (int q = 0; q < N + 2; ++q) {
                const bool inner = q < N;
                const double s = inner ? section::Gauss<N>::x[q < N ? q : 0] : (q == N ? 0.0 : 1.0);
                const double tq = inner ? t0 + s * dt : (q == N ? t0 : t1);
                double xq[DIM], v, g[DIM], sg[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) xq[k] = a[k] + tq * d[k];
                flowline::value_grad<DIM, K>(V, z, A.S, A.u, e, xq, v, g);
                good = good & interp::finite(v) & flowline::all_finite<DIM>(g);
                vmax = v > vmax ? v : vmax;
                vmin = v < vmin ? v : vmin;
                if (inner) {
                  section::sigma<DIM>(g, A.p, sg);
                  const double om = section::Gauss<N>::w[q < N ? q : 0] * len;
                  double st = sg[0] * tdir[0];
#pragma unroll
                  for (int k = 1; k < DIM; ++k) st += sg[k] * tdir[k];
                  pu += om * v;
                  pal += om * st;
                  if constexpr (DIM == 2) pac += om * (sg[1] * tdir[0] - sg[0] * tdir[1]);
                }
              }
              length += len;
              integral += pu;
              along += pal;
              across += pac;
              enter = (pieces == 0) | (t0 < enter) ? t0 : enter;
              leave = (pieces == 0) | (t1 > leave) ? t1 : leave;
              if (piece != nullptr && pieces < cap) {
                piece[(size_t)pieces * kPieceWidth] = t0;
                piece[(size_t)pieces * kPieceWidth + 1] = t1;
                piece[(size_t)pieces * kPieceWidth + 2] = pu;
                elem[pieces] = e;
              }
              ++pieces;
            }
          }
      }
    }
  }
  if (row != nullptr) {
    row[0] = length;
    row[1] = good ? integral : nan;
    row[2] = good ? along : nan;
    row[3] = good ? across : nan;
    row[4] = good ? vmax : nan;
    row[5] = good ? vmin : nan;
    row[6] = enter;
    row[7] = leave;
    *count = pieces;
  }
}

// What a call brings, as far as it can be judged before anything is allocated: the ONE place where the arguments of both entry
// points are checked (ray.hip).  Throws ArgError.
struct Call {
  int dim, B, S, u, m, workgroup;      // workgroup: 0 = the default (the host restatement passes 0)
  double p;
  bool null_argument;                  // some pointer argument is null
  int world;                           // ranks of the context (1 for the host restatement)
  long long want_len;                  // n x S
  const long long* field_len;          // null, or B lengths: -1 a null field, -2 a vector of another context
};
void check(const std::string& who, const Call& c);

// host restatement: row after row, field slowest; with offsets non-null (B m + 1) the pieces of every row are appended in CSR
// form to piece (capacity x 3) and elem (capacity).  Throws ArgError where they do not fit.
void line_integrals_host(int dim, int k, const Args& A, long long* offsets, double* piece, int32_t* elem, long long capacity);

#if defined(__HIPCC__)
constexpr int kDefaultWorkgroup = 64;
// one lane per (ray, field) on a grid (ceil(m / wg), B), wg = 64, 128 or 256; all pointers of A are device pointers
void launch_measure(hipStream_t stream, int dim, int k, const Args& A, int wg);
// the same grid: every lane walks again and writes its pieces at offsets[row] .. offsets[row + 1]
void launch_emit(hipStream_t stream, int dim, int k, const Args& A, int wg, const long long* offsets, double* piece, int32_t* elem);
#endif

}  // namespace ray
}  // namespace mgb
