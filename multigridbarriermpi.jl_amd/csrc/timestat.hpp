// Time statistics of a run of snapshots: what ONE node contributes, written ONCE.  The gfx950 kernel
// (timestat.hip) and the host restatement (mgb_geo_time_stats_host) both run node_columns(), level_columns() and the two
// term routines below; combine, block_reduce and the finish are reduce.hpp's, the -inf identity and the serial sum levelset.hpp's.
//   Snapshots m = 0..B-1, B >= 2, v_m = z[m][i S + u]; h_m = ts[m+1] - ts[m] comes from the caller (ONE subtraction, done once
//   per call on the host).  A value is ABOVE a level c when v > c (the rule of levelset.hpp).  Every sum is a plain running sum
//   in ascending m.  The rule itself is the comment of mgb_geo_time_stats in include/mgb_hip.h.
//   Loads: each routine reads every v_m once, kAhead of them at a time BEFORE it uses any, so that a thread of the kernel has
//   kAhead independent loads in flight; the arithmetic does not depend on kAhead.
//   A node with a non-finite v_m gets NaN in every column, and NaN terms.
// The arithmetic is kept as written by ONE mechanism: timestat.hip, which holds the kernel AND the host restatement and is the
// only file that may instantiate these routines, is compiled with -ffp-contract=off (build.sh).
#pragma once
#include <cmath>
#include <string>

#include "levelset.hpp"
#include "reduce.hpp"

namespace mgb {
namespace timestat {

using reduce::kCols;
using reduce::kThreads;
using reduce::kWaves;
using reduce::nanmax;
using levelset::NoItems;      // both maxima of every row may be negative: the fold starts from -inf in both

constexpr int kNodeCols = 8;       // MGB_TIMESTAT_NODE_COLS: integral max tmax min tmin variation rate change
constexpr int kLevelCols = 5;      // MGB_TIMESTAT_LEVEL_COLS: arrival left exposure excess entries
constexpr int kMaxLevels = 4096;
constexpr int kChunk = 4;          // levels whose state one thread keeps in registers (8 leaves 3 waves per SIMD, not 5, and is slower)
constexpr int kAhead = 4;          // loads in flight per thread

// what one call works on; every pointer is a host pointer or every pointer is a device pointer
struct Args {
  const double* const* z = nullptr;      // B pointers to n x S fields
  const double* h = nullptr;             // B - 1 steps
  const double* ts = nullptr;            // B times
  const double* levels = nullptr;        // nl levels
  const double* w = nullptr;             // n nodal weights
  double* node = nullptr;                // n x kNodeCols
  double* level = nullptr;               // nl x n x kLevelCols
  double never = 0.0;
  long long n = 0;
  int S = 0, u = 0, B = 0, nl = 0;
};

// the eight node columns of node i
MGB_HD void node_columns(const Args& A, size_t i, double* col) {
  const size_t off = i * (size_t)A.S + (size_t)A.u;
  double a = A.z[0][off];
  const double v0 = a;
  bool good = interp::finite(a);
  double acc = 0.0, mx = a, tmx = A.ts[0], mn = a, tmn = A.ts[0], var = 0.0, rate = 0.0;
  for (int m0 = 1; m0 < A.B; m0 += kAhead) {
    double v[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) v[k] = m0 + k < A.B ? A.z[m0 + k][off] : 0.0;
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      if (m0 + k < A.B) {
        const double b = v[k], h = A.h[m0 + k - 1], tb = A.ts[m0 + k];
        good = good & interp::finite(b);
        acc += (0.5 * h) * (a + b);
        const double d = fabs(b - a);
        var += d;
        const double q = d / h;
        rate = q > rate ? q : rate;
        if (b > mx) mx = b, tmx = tb;
        if (b < mn) mn = b, tmn = tb;
        a = b;
      }
    }
  }
  col[0] = acc, col[1] = mx, col[2] = tmx, col[3] = mn, col[4] = tmn, col[5] = var, col[6] = rate, col[7] = a - v0;
  if (!good) {
#pragma unroll
    for (int k = 0; k < kNodeCols; ++k) col[k] = std::numeric_limits<double>::quiet_NaN();
  }
}

// what node i gives to row 0
MGB_HD void node_term(double w, const double* col, double* c) {
  c[0] = w * col[0];
  c[1] = w * col[5];
  c[2] = w * col[7];
  c[3] = col[1];
  c[4] = -col[3];
}

// the five level columns of node i for the cnt <= kChunk levels from l0 on; col[k] is written for k < cnt only
MGB_HD void level_columns(const Args& A, size_t i, int l0, int cnt, double (*col)[kLevelCols]) {
  const size_t off = i * (size_t)A.S + (size_t)A.u;
  double a = A.z[0][off];
  bool good = interp::finite(a);
  double c[kChunk], arrival[kChunk], left[kChunk], exposure[kChunk], excess[kChunk];
  int entries[kChunk];
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    c[k] = A.levels[l0 + (k < cnt ? k : 0)];
    const bool up = a > c[k];
    entries[k] = up ? 1 : 0;
    arrival[k] = up ? A.ts[0] : A.never;
    left[k] = A.never;
    exposure[k] = excess[k] = 0.0;
  }
  for (int m0 = 1; m0 < A.B; m0 += kAhead) {
    double v[kAhead];
#pragma unroll
    for (int j = 0; j < kAhead; ++j) v[j] = m0 + j < A.B ? A.z[m0 + j][off] : 0.0;
#pragma unroll
    for (int j = 0; j < kAhead; ++j) {
      if (m0 + j < A.B) {
        const double b = v[j], h = A.h[m0 + j - 1], ta = A.ts[m0 + j - 1], tb = A.ts[m0 + j];
        good = good & interp::finite(b);
#pragma unroll
        for (int k = 0; k < kChunk; ++k) {
          const bool ua = a > c[k], ub = b > c[k];
          if (k >= cnt) {      // uniform: an empty slot of the last chunk
          } else if (ua & ub) {
            exposure[k] += h;
            excess[k] += h * ((a + b) * 0.5 - c[k]);
          } else if (ua | ub) {
            const double lo = ua ? b : a, hi = ua ? a : b;
            const double t = (c[k] - lo) / (hi - lo), f = 1.0 - t, e = f * h;
            exposure[k] += e;
            excess[k] += e * ((hi - c[k]) * 0.5);
            if (ub) {
              if (entries[k] == 0) arrival[k] = ta + t * h;
              entries[k] += 1;
            } else {
              left[k] = tb - t * h;
            }
          }
        }
        a = b;
      }
    }
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    if (k < cnt) {
      col[k][0] = good ? arrival[k] : nan;
      col[k][1] = good ? left[k] : nan;
      col[k][2] = good ? exposure[k] : nan;
      col[k][3] = good ? excess[k] : nan;
      col[k][4] = good ? (double)entries[k] : nan;
    }
  }
}

// what node i gives to row 1 + l
MGB_HD void level_term(double w, const double* col, double* c) {
  const bool reached = col[4] > 0.0;
  c[0] = col[4] != col[4] ? col[4] : (reached ? w : 0.0);
  c[1] = w * col[2];
  c[2] = w * col[3];
  c[3] = col[4] != col[4] ? col[4] : (reached ? col[0] : -std::numeric_limits<double>::infinity());
  c[4] = col[2];
}

// what both entry points check alike, before anything is launched or written
struct Call {
  bool null_argument = false;
  int B = 0, S = 0, u = 0, nl = 0;
  const double* ts = nullptr;
  const double* levels = nullptr;
};
void check(const std::string& who, const Call& c);

// workgroups of the statistics launch, and the y extent of its grid
inline int level_chunks(int nl) { return (nl + kChunk - 1) / kChunk; }

// doubles of the scratch buffer for nwg workgroups: partials (1 + nl) x nwg x kCols | results (1 + nl) x kCols
inline size_t results_offset(size_t nl, size_t nwg) { return (1 + nl) * nwg * kCols; }
inline size_t scratch_doubles(size_t nl, size_t nwg) { return (1 + nl) * nwg * kCols + (1 + nl) * kCols; }

// timestat.hip, host: the same routines, serially in ascending node order; out: (1 + nl) x kCols
void time_stats_host(const Args& A, double* out);

#if defined(__HIPCC__)
// timestat.hip: two launches on `stream` -- the statistics on grid (workgroups(n), 1 + level_chunks(nl)), then one workgroup
// per row that finishes the row's partials from the -inf identity; all pointers of A are device pointers
void launch_time_stats(hipStream_t stream, const Args& A, double* scratch);
#endif

}  // namespace timestat
}  // namespace mgb
