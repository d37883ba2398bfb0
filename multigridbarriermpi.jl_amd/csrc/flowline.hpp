// Flow lines of nodal fields: the curves that follow grad u, traced by the explicit midpoint rule in
// arc length through the broken polynomial field, with their lengths and travel times int ds / |sigma|,
// sigma = |grad u|^(p-2) grad u.  The per-seed routine trace() is written ONCE on top of interp.hpp (locator, ref_coords,
// ElemBasis, find_element): the gfx950 kernel (flowline.hip) and the host restatement (mgb_geo_flow_lines_host) both run it,
// the way levelset.hpp is shared.  The rule -- stages, stops, the exit bisection -- is the public contract of
// include/mgb_hip.h.  The file that includes this is compiled with fp contraction off: both sides run the same IEEE
// + - * / and sqrt, so points, lengths and end values agree bit for bit; only pow (p other than 1 and 2) differs.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "interp.hpp"

namespace mgb {
namespace flowline {

constexpr int kExit = 0, kStalled = 1, kMaxSteps = 2, kOutside = 3, kNonFinite = 4;      // MGB_FLOW_* of the header
constexpr int kRowCols = 4;                                                               // length, time, u_start, u_end
constexpr int kBisect = 40;                                                               // halvings of the exit search

struct Args {
  interp::BinsView own;            // the locator of the geometry
  const double* const* z;          // B fields of n x S nodal values
  const double* seeds;             // m x dim
  double p, ds, gmin, sgn;         // sgn = +1 (up the gradient) or -1
  int m, S, u, B, max_steps;
  long long stride;                // slots per row of pts / pelem: max_steps + 2
  double* rows;                    // B m x 4
  double* end;                     // B m x dim
  int32_t *status, *count, *end_element;      // B m each
  double* pts;                     // null without paths: B m x stride x dim
  int32_t* pelem;                  // ... B m x stride
};

// value and physical gradient of column u of element e's polynomial at q (the operations of interp::eval_in_element for that
// column); q need not lie in e
template <int DIM, int K>
MGB_HD void value_grad(const interp::BinsView& V, const double* z, int S, int u, int e, const double* q, double& v, double* g) {
  double r[DIM];
  interp::ref_coords<DIM>(V.x, V.block, e, q, r);
  interp::ElemBasis<DIM, K> E;
  E.init(V.x, V.block, e, r);
  E.template eval<false>(z + (size_t)e * V.block * S, nullptr, S, u, v, g);
}

// e when q is inside e by the containment rule, else the lowest element that holds q, -1 when none does
template <int DIM>
MGB_HD int locate(const interp::BinsView& V, int e, const double* q) {
  double r[DIM];
  if (interp::ref_coords<DIM>(V.x, V.block, e, q, r)) return e;
  return interp::find_element<DIM>(V, q);
}

template <int DIM>
MGB_HD double norm(const double* g) {
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) s += g[d] * g[d];
  return sqrt(s);
}

template <int DIM>
MGB_HD bool all_finite(const double* g) {
  bool fin = true;
#pragma unroll
  for (int d = 0; d < DIM; ++d) fin = fin & interp::finite(g[d]);
  return fin;
}

// a^(1-p), the time per unit of arc length: exactly 1 for p = 1 and 1 / a for p = 2, pow otherwise
MGB_HD double slowness(double a, double p) {
  if (p == 1.0) return 1.0;
  if (p == 2.0) return 1.0 / a;
  return pow(a, 1.0 - p);
}

// the recorded points of one line: slot `count` of a row of `stride` slots; a slot beyond the stride is never written
struct Path {
  double* pts;
  int32_t* el;
  long long stride;
  int count;
  template <int DIM>
  MGB_HD void put(const double* x, int e) {
    if (pts != nullptr && count < stride) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) pts[(size_t)count * DIM + d] = x[d];
      el[count] = e;
    }
    ++count;
  }
};

// One line of field z from `seed`: row (4), end (DIM), status, count, end_element and, with pts non-null, the recorded points
// and their elements in a row of A.stride slots.
template <int DIM, int K>
MGB_HD void trace(const Args& A, const double* z, const double* seed, double* row, double* end, int32_t* status, int32_t* count,
                  int32_t* end_element, double* pts, int32_t* pelem) {
  const interp::BinsView& V = A.own;
  double x[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) x[d] = seed[d];
  int e = interp::find_element<DIM>(V, x);
  if (e < 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
#pragma unroll
    for (int c = 0; c < kRowCols; ++c) row[c] = nan;
#pragma unroll
    for (int d = 0; d < DIM; ++d) end[d] = nan;
    *status = kOutside;
    *count = 0;
    *end_element = -1;
    return;
  }
  Path P{pts, pelem, A.stride, 0};
  P.template put<DIM>(x, e);
  double length = 0.0, time = 0.0, u0 = 0.0, v = 0.0;
  int st = kMaxSteps;
  for (int k = 0;; ++k) {
    double g[DIM];
    value_grad<DIM, K>(V, z, A.S, A.u, e, x, v, g);
    if (k == 0) u0 = v;
    if (!(interp::finite(v) && all_finite<DIM>(g))) {
      st = kNonFinite;
      break;
    }
    const double a = norm<DIM>(g);
    if (!(a > A.gmin)) {
      st = kStalled;
      break;
    }
    if (k == A.max_steps) {
      st = kMaxSteps;
      break;
    }
    double q[DIM];
    const double half = 0.5 * A.ds;
#pragma unroll
    for (int d = 0; d < DIM; ++d) q[d] = x[d] + half * (A.sgn * g[d] / a);
    int en = locate<DIM>(V, e, q);      // the midpoint's element
    if (en >= 0) {
      double vm, gm[DIM];
      value_grad<DIM, K>(V, z, A.S, A.u, en, q, vm, gm);
      if (!all_finite<DIM>(gm)) {
        st = kNonFinite;
        break;
      }
      const double am = norm<DIM>(gm);
      if (!(am > A.gmin)) {
        st = kStalled;
        break;
      }
#pragma unroll
      for (int d = 0; d < DIM; ++d) q[d] = x[d] + A.ds * (A.sgn * gm[d] / am);
      en = locate<DIM>(V, en, q);      // the new point's element
      if (en >= 0) {
        length += A.ds;
        time += A.ds * slowness(am, A.p);
#pragma unroll
        for (int d = 0; d < DIM; ++d) x[d] = q[d];
        e = en;
        P.template put<DIM>(x, e);
        continue;
      }
    }
    // exit along x -> q: the last point of the segment that still has an element, by bisection from e
    double lo = 0.0, hi = 1.0, dq[DIM], r[DIM];
    int er = e;
#pragma unroll
    for (int d = 0; d < DIM; ++d) dq[d] = q[d] - x[d];
    for (int it = 0; it < kBisect; ++it) {
      const double th = 0.5 * (lo + hi);
#pragma unroll
      for (int d = 0; d < DIM; ++d) r[d] = x[d] + th * dq[d];
      const int ee = locate<DIM>(V, e, r);
      if (ee >= 0) {
        lo = th;
        er = ee;
      } else {
        hi = th;
      }
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) x[d] = x[d] + lo * dq[d];
    e = er;
    const double len = lo * norm<DIM>(dq);
    length += len;
    time += len * slowness(a, A.p);
    if (lo > 0.0) P.template put<DIM>(x, e);
    double ge[DIM];
    value_grad<DIM, K>(V, z, A.S, A.u, e, x, v, ge);
    st = kExit;
    break;
  }
  row[0] = length;
  row[1] = time;
  row[2] = u0;
  row[3] = v;
#pragma unroll
  for (int d = 0; d < DIM; ++d) end[d] = x[d];
  *status = st;
  *count = P.count;
  *end_element = e;
}

// what both entry points check alike, before anything is launched or written
void check(const Args& A, int dim, bool paths);

// host restatement: row after row, b slowest; with offsets non-null the points of every row are appended in CSR form
// (offsets B m + 1, pts capacity x dim, pelem capacity)
void flow_lines_host(int dim, int k, const Args& A, long long* offsets, double* pts, int32_t* pelem, long long capacity);

#if defined(__HIPCC__)
constexpr int kDefaultWorkgroup = 64;
// one thread per (seed, field) on a grid (ceil(m / wg), B), wg = 64, 128 or 256; all pointers of A are device pointers
void launch_trace(hipStream_t stream, int dim, int k, const Args& A, int wg);
// gathers the recorded points of every row from its fixed-stride row into the CSR arrays: grid (B m), one workgroup per row
void launch_compact(hipStream_t stream, int dim, const Args& A, const long long* offsets, double* pts, int32_t* pelem);
#endif

}  // namespace flowline
}  // namespace mgb
