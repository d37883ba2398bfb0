// The two-stage field reduction of the post-processing modules, written ONCE: norms, parabolic
// violations, energy, boundary flux and error indicators all reduce this way.
//   Stage 1, the module's own kernel: every thread of a 256-thread workgroup holds one value (five columns, a count, a maximum);
//     block_reduce folds them -- wave shuffles at offsets 32, 16, .., 1, lane 0 of each wave to LDS, one barrier, thread 0 folds
//     waves 1, 2, 3 in that order -- and thread 0 writes ONE partial row per workgroup.
//   Stage 2, a finish launch of one workgroup per result row: thread t folds the t-th contiguous run of ceil(nwg / 256)
//     partials in ascending order (run_of), then the same block_reduce; thread 0 writes the result.
// No atomics and no hand-off between workgroups inside a launch: every word is written by one thread, every sum has a fixed
// order, so a result is bitwise reproducible and the second launch cannot wait on the first.  No thread returns in front of a
// barrier: idle threads carry the identity through it.
#pragma once
#include <cstddef>
#include <limits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef MGB_HD
#if defined(__HIPCC__)
#define MGB_HD __host__ __device__ inline
#else
#define MGB_HD inline
#endif
#endif

namespace mgb {
namespace reduce {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCols = 5;      // three sums, then two NaN-sticky maxima: MGB_NORM_COLS, MGB_ENERGY_COLS, MGB_BOUNDARY_COLS, MGB_ESTIMATE_COLS
static_assert(kWaves == 4, "four waves of 64");

// the larger of m and v where a NaN, once seen, stays
MGB_HD double nanmax(double m, double v) { return ((v > m) | (v != v)) ? v : m; }

MGB_HD void combine(double* acc, const double* c) {
  acc[0] += c[0];
  acc[1] += c[1];
  acc[2] += c[2];
  acc[3] = nanmax(acc[3], c[3]);
  acc[4] = nanmax(acc[4], c[4]);
}

// the identity of combine: the second maximum may be negative
MGB_HD void identity(double* c) {
  c[0] = c[1] = c[2] = c[3] = 0.0;
  c[4] = -std::numeric_limits<double>::infinity();
}

// workgroups of a launch with one thread per item
inline long long workgroups(long long n) { return (n + kThreads - 1) / kThreads; }

// the run [b0, b1) of `count` partials that thread t of a finish folds; empty for the trailing threads
struct Run {
  long long b0, b1;
};
MGB_HD Run run_of(int t, int count) {
  const int chunk = (count + kThreads - 1) / kThreads;
  const long long b0 = (long long)t * chunk;
  return {b0, b0 + chunk < count ? b0 + chunk : count};
}

// the operators of block_reduce: acc = op(acc, c) on N values
struct Combine {
  MGB_HD void operator()(double* acc, const double* c) const { combine(acc, c); }
};
template <int N>
struct NanMax {
  MGB_HD void operator()(double* acc, const double* c) const {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = nanmax(acc[k], c[k]);
  }
};
struct Count {
  MGB_HD void operator()(long long* acc, const long long* c) const { acc[0] += c[0]; }
};

#if defined(__HIPCC__)
// Reduce the N values of v over the workgroup; the result is valid in thread 0.  One barrier and no trailing one: where
// reductions follow each other the caller alternates between two `red` buffers.
template <int N, class T, class Op>
__device__ inline void block_reduce(T* v, Op op, T (*red)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    T t[N];
#pragma unroll
    for (int k = 0; k < N; ++k) t[k] = __shfl_down(v[k], o, 64);
    op(v, t);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) op(v, red[w]);
  }
}

// stage 2 of one row, for the calling workgroup: partial g of the row is the kCols doubles at partials + g * stride.  Id sets
// the value the fold starts from: Identity for every module whose first maximum is non-negative, the module's own otherwise.
struct Identity {
  MGB_HD void operator()(double* c) const { identity(c); }
};
template <class Id>
__device__ inline void run_combine(const double* __restrict__ partials, size_t stride, int nwg, double* c, Id id) {
  id(c);
  const Run r = run_of(threadIdx.x, nwg);
  for (long long g = r.b0; g < r.b1; ++g) combine(c, partials + (size_t)g * stride);
}
__device__ inline void run_combine(const double* __restrict__ partials, size_t stride, int nwg, double* c) {
  run_combine(partials, stride, nwg, c, Identity{});
}
template <class Id>
__device__ inline void finish_row(const double* __restrict__ partials, size_t stride, int nwg, double (*red)[kCols],
                                  double* __restrict__ out, Id id) {
  double c[kCols];
  run_combine(partials, stride, nwg, c, id);
  block_reduce<kCols>(c, Combine{}, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kCols; ++k) out[k] = c[k];
  }
}
__device__ inline void finish_row(const double* __restrict__ partials, size_t stride, int nwg, double (*red)[kCols],
                                  double* __restrict__ out) {
  finish_row(partials, stride, nwg, red, out, Identity{});
}

// reduce.hip: the finish launch on grid (rows); row r combines its nwg partials at partials + r * row_stride + g * wg_stride
// (strides in doubles) and writes out[r * kCols ..]; all pointers are device pointers
void launch_finish(hipStream_t stream, int rows, const double* partials, int nwg, size_t row_stride, size_t wg_stride, double* out);
#endif

}  // namespace reduce
}  // namespace mgb
