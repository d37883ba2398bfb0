// Path lines through a field that changes in time: where a particle released at a seed at snapshot
// time ts[release] is at ts[stop], carried by w = speed sgn |grad u|^(p-2) grad u of the field blended linearly in time between
// the snapshots of a parabolic run, by the explicit midpoint rule in TIME.  The per-seed routine advance() is written ONCE on
// top of interp.hpp and flowline.hpp (value_grad's operations, locate, norm, all_finite, Path): the gfx950 kernel
// (pathline.hip) and the host restatement (mgb_geo_path_lines_host) both run it.  The rule -- the blend, the fractions, the
// stages, the rest, the exit bisection -- is the public contract of include/mgb_hip.h.  The file that includes this is compiled
// with fp contraction off: both sides run the same IEEE + - * / and sqrt; only pow (p other than 1, 1.5 and 2) differs.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "flowline.hpp"

namespace mgb {
namespace pathline {

constexpr int kDone = 0, kExit = 1, kOutside = 2, kNonFinite = 3;      // MGB_PATH_* of the header
constexpr int kRowCols = 5;                                            // length, time, u_start, u_end, max_step

struct Args {
  interp::BinsView own;            // the locator of the geometry
  const double* const* z;          // B snapshots of n x S nodal values
  const double* ts;                // B times, strictly increasing
  const double* seeds;             // m x dim
  const int32_t* release;          // m: the snapshot at whose time seed i is released, in [0, stop)
  double p, sgn, speed, gmin;      // sgn = +1 (up the gradient) or -1
  int m, S, u, B, stop, substeps;
  long long stride;                // slots per row of pts / pelem: (stop - min release) substeps + 2
  double* rows;                    // m x 5
  double* end;                     // m x dim
  int32_t *status, *count, *end_element, *rested;      // m each
  double* pts;                     // null without paths: m x stride x dim
  int32_t* pelem;                  // ... m x stride
};

// The field in time at q in element e, at fraction th of the slab between snapshots za and zb: v = v_a + th (v_b - v_a) and
// the same for every component of the gradient, (v_a, g_a) and (v_b, g_b) by the operations of flowline::value_grad.  The
// reference coordinates and the basis are formed once; the two snapshots go through one rolled loop, so that the sums of the
// basis stand once in the code (registers: 64 terms per sum for k = 3).
template <int DIM, int K>
MGB_HD void blend(const interp::BinsView& V, const double* za, const double* zb, int S, int u, int e, const double* q, double th,
                  double& v, double* g) {
  double r[DIM];
  interp::ref_coords<DIM>(V.x, V.block, e, q, r);
  interp::ElemBasis<DIM, K> E;
  E.init(V.x, V.block, e, r);
  const size_t at = (size_t)e * V.block * S;
  double va = 0.0, ga[DIM], vb = 0.0, gb[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) ga[d] = gb[d] = 0.0;
#pragma unroll 1
  for (int b = 0; b < 2; ++b) {
    if (b == 1) {
      va = vb;
#pragma unroll
      for (int d = 0; d < DIM; ++d) ga[d] = gb[d];
    }
    E.template eval<false>((b == 0 ? za : zb) + at, nullptr, S, u, vb, gb);
  }
  v = va + th * (vb - va);
#pragma unroll
  for (int d = 0; d < DIM; ++d) g[d] = ga[d] + th * (gb[d] - ga[d]);
}

// w(g) = speed sgn |g|^(p-2) g; false and w = 0 when not |g| > gmin (the particle rests)
template <int DIM>
MGB_HD bool velocity(const Args& A, const double* g, double* w) {
  const double a = flowline::norm<DIM>(g);
  if (!(a > A.gmin)) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) w[d] = 0.0;
    return false;
  }
  if (A.p == 1.0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) w[d] = A.speed * (A.sgn * g[d] / a);
  } else if (A.p == 2.0) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) w[d] = A.speed * (A.sgn * g[d]);
  } else if (A.p == 1.5) {
    const double ra = sqrt(a);
#pragma unroll
    for (int d = 0; d < DIM; ++d) w[d] = A.speed * (A.sgn * g[d] / ra);
  } else {
    const double f = pow(a, A.p - 2.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) w[d] = A.speed * (A.sgn * g[d] * f);
  }
  return true;
}

// One particle from `seed`, released at ts[rel]: row (5), end (DIM), status, count, end_element, rested and, with pts non-null,
// the recorded points and their elements in a row of A.stride slots.
template <int DIM, int K>
MGB_HD void advance(const Args& A, const double* seed, int rel, double* row, double* end, int32_t* status, int32_t* count,
                    int32_t* end_element, int32_t* rested, double* pts, int32_t* pelem) {
  const interp::BinsView& V = A.own;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double x[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) x[d] = seed[d];
  int e = interp::find_element<DIM>(V, x);
  if (e < 0) {
#pragma unroll
    for (int c = 0; c < kRowCols; ++c) row[c] = nan;
#pragma unroll
    for (int d = 0; d < DIM; ++d) end[d] = nan;
    *status = kOutside;
    *count = 0;
    *end_element = -1;
    *rested = 0;
    return;
  }
  flowline::Path P{pts, pelem, A.stride, 0};
  P.template put<DIM>(x, e);
  const int n = A.substeps;
  double length = 0.0, time = A.ts[A.stop], u0 = 0.0, v = 0.0, max_step = 0.0;
  int st = kDone, nrest = 0;
  bool first = true;
  for (int j = rel; j < A.stop && st == kDone; ++j) {
    const double *za = A.z[j], *zb = A.z[j + 1];
    const double t0 = A.ts[j], slab = A.ts[j + 1] - t0, dt = slab / n;
    for (int i = 0; i < n; ++i) {
      const double th = (double)i / n, thm = (double)(2 * i + 1) / (2 * n), tk = t0 + i * dt;
      double g[DIM], w[DIM], q[DIM];
      blend<DIM, K>(V, za, zb, A.S, A.u, e, x, th, v, g);
      if (first) u0 = v;
      first = false;
      if (!(interp::finite(v) && flowline::all_finite<DIM>(g))) {
        st = kNonFinite;
        time = tk;
        if (interp::finite(v)) v = nan;
        break;
      }
      velocity<DIM>(A, g, w);
      const double half = 0.5 * dt;
      double span = half;
#pragma unroll
      for (int d = 0; d < DIM; ++d) q[d] = x[d] + half * w[d];
      int en = flowline::locate<DIM>(V, e, q);      // the midpoint's element
      if (en >= 0) {
        double vm, gm[DIM];
        blend<DIM, K>(V, za, zb, A.S, A.u, en, q, thm, vm, gm);
        if (!flowline::all_finite<DIM>(gm)) {
          st = kNonFinite;
          time = tk;
          v = nan;
          break;
        }
        const bool moves = velocity<DIM>(A, gm, w);
        span = dt;
#pragma unroll
        for (int d = 0; d < DIM; ++d) q[d] = x[d] + dt * w[d];
        en = flowline::locate<DIM>(V, en, q);      // the new point's element
        if (en >= 0) {
          const double s = dt * flowline::norm<DIM>(w);
          length += s;
          max_step = max_step > s ? max_step : s;
          nrest += moves ? 0 : 1;
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
      for (int it = 0; it < flowline::kBisect; ++it) {
        const double mid = 0.5 * (lo + hi);
#pragma unroll
        for (int d = 0; d < DIM; ++d) r[d] = x[d] + mid * dq[d];
        const int ee = flowline::locate<DIM>(V, e, r);
        if (ee >= 0) {
          lo = mid;
          er = ee;
        } else {
          hi = mid;
        }
      }
#pragma unroll
      for (int d = 0; d < DIM; ++d) x[d] = x[d] + lo * dq[d];
      e = er;
      length += lo * flowline::norm<DIM>(dq);
      time = tk + lo * span;
      if (lo > 0.0) P.template put<DIM>(x, e);
      double ge[DIM];
      blend<DIM, K>(V, za, zb, A.S, A.u, e, x, th + lo * span / slab, v, ge);
      st = kExit;
      break;
    }
  }
  if (st == kDone) {
    double ge[DIM];
    flowline::value_grad<DIM, K>(V, A.z[A.stop], A.S, A.u, e, x, v, ge);      // from that snapshot alone
  }
  row[0] = length;
  row[1] = time;
  row[2] = u0;
  row[3] = v;
  row[4] = max_step;
#pragma unroll
  for (int d = 0; d < DIM; ++d) end[d] = x[d];
  *status = st;
  *count = P.count;
  *end_element = e;
  *rested = nrest;
}

// Everything both entry points are called with that can be judged without a context, and what the device entry point adds
// (null for the host restatement): judged in ONE place, before anything is allocated, launched or written.
struct Call {
  int dim, B, S, u, m, stop, substeps, direction, workgroup;      // workgroup: 0 = the default (the host restatement passes 0)
  double p, speed, gmin;
  const double* ts;                // host, B
  const int32_t* release;          // host, m
  bool null_argument;              // some pointer argument is null
  bool paths;
  int world;                       // ranks of the context (1 for the host restatement)
  long long want_len;              // n x S
  const long long* field_len;      // null, or B lengths: -1 a null field, -2 a vector of another context
};
// fills p, sgn, speed, gmin, m, S, u, B, stop, substeps and stride of A
void check(const char* who, const Call& c, Args& A);

// host restatement: row after row; with offsets non-null the points of every row are appended in CSR form
// (offsets m + 1, pts capacity x dim, pelem capacity)
void path_lines_host(int dim, int k, const Args& A, long long* offsets, double* pts, int32_t* pelem, long long capacity);

#if defined(__HIPCC__)
constexpr int kDefaultWorkgroup = 64;
// one thread per seed on a grid ceil(m / wg), wg = 64, 128 or 256; all pointers of A are device pointers
void launch_advance(hipStream_t stream, int dim, int k, const Args& A, int wg);
#endif

}  // namespace pathline
}  // namespace mgb
