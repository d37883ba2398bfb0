// Time statistics of a run of snapshots on gfx950.  B snapshots on one geometry are reduced along the
// time axis, per node, by TWO plain launches on one stream, whatever B and nl are:
//   stats_kernel: grid (ceil(n / 256), 1 + ceil(nl / kChunk)) of 256 threads, one node per thread.  A thread walks m = 0..B-1
//     once, kAhead loads in flight, with the state of its slab in registers: blockIdx.y = 0 runs timestat.hpp's node_columns()
//     and writes its row of the n x 8 table, y >= 1 runs level_columns() on a chunk of at most kChunk levels and writes its
//     rows of the nl x n x 5 table.  The snapshot pointers, h, ts and the levels are uniform: the compiler reads them with
//     scalar loads.  Every workgroup folds its terms with reduce.hpp's block_reduce and writes ONE partial row per result row.
//   finish_kernel: one workgroup per result row folds the row's partials (reduce.hpp's finish_row) from the -inf identity.
// No atomics, no hand-off between workgroups, no thread returns in front of a barrier: idle threads carry the identity.  A
// level's state is its own, so its table and its row do not depend on nl, on the other levels or on kChunk.
// This file is compiled with fp contraction off (build.sh): kernel and host restatement run the same operations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

// Every function of the project's headers is inlined in this file, as in flowline.hip, so that this object file shares no
// out-of-line (weak) arithmetic with the files compiled with contraction on.
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "errors.hpp"
#include "timestat.hpp"
#pragma clang attribute pop

namespace mgb {
namespace timestat {
namespace {

__global__ void __launch_bounds__(kThreads) stats_kernel(Args A, double* __restrict__ partials, int nwg) {
  __shared__ double red[2][kWaves][kCols];
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < (size_t)A.n;
  const double w = live ? A.w[i] : 0.0;
  if (blockIdx.y == 0) {
    double c[kCols];
    NoItems{}(c);
    if (live) {
      double col[kNodeCols];
      node_columns(A, i, col);
      double* out = A.node + i * kNodeCols;
#pragma unroll
      for (int k = 0; k < kNodeCols; ++k) out[k] = col[k];
      node_term(w, col, c);
    }
    reduce::block_reduce<kCols>(c, reduce::Combine{}, red[0]);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kCols; ++k) partials[(size_t)blockIdx.x * kCols + k] = c[k];
    }
  }
  // y >= 1 (a workgroup-uniform choice; for y = 0 cnt is <= 0 and nothing below runs)
  const int l0 = ((int)blockIdx.y - 1) * kChunk;
  const int cnt = blockIdx.y == 0 ? 0 : (A.nl - l0 < kChunk ? A.nl - l0 : kChunk);
  double col[kChunk][kLevelCols];
  if (live && cnt > 0) level_columns(A, i, l0, cnt, col);
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    if (k < cnt) {      // the same for every thread of the workgroup: the barrier inside is reached by all or by none
      double c[kCols];
      NoItems{}(c);
      if (live) {
        double* out = A.level + ((size_t)(l0 + k) * (size_t)A.n + i) * kLevelCols;
#pragma unroll
        for (int j = 0; j < kLevelCols; ++j) out[j] = col[k][j];
        level_term(w, col[k], c);
      }
      reduce::block_reduce<kCols>(c, reduce::Combine{}, red[k & 1]);
      if (threadIdx.x == 0) {
        double* p = partials + ((size_t)(1 + l0 + k) * nwg + blockIdx.x) * kCols;
#pragma unroll
        for (int j = 0; j < kCols; ++j) p[j] = c[j];
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) finish_kernel(const double* __restrict__ partials, int nwg, double* __restrict__ out) {
  __shared__ double red[kWaves][kCols];
  reduce::finish_row(partials + (size_t)blockIdx.x * nwg * kCols, kCols, nwg, red, out + (size_t)blockIdx.x * kCols, NoItems{});
}

}  // namespace

void check(const std::string& who, const Call& c) {
  if (c.null_argument) throw ArgError(who + ": null argument");
  if (c.B < 2) throw ArgError(who + ": B must be >= 2 (a window holds at least two snapshots)");
  if (c.nl < 0 || c.nl > kMaxLevels) throw ArgError(who + ": nl must be 0..4096");
  if (c.nl > 0 && !c.levels) throw ArgError(who + ": null argument");
  if (c.S < 1) throw ArgError(who + ": S must be >= 1");
  if (c.u < 0 || c.u >= c.S) throw ArgError(who + ": column u outside [0, S)");
  for (int m = 0; m < c.B; ++m) {
    if (!interp::finite(c.ts[m])) throw ArgError(who + ": every time must be finite");
    if (m > 0 && !(c.ts[m] > c.ts[m - 1])) throw ArgError(who + ": the times must be strictly increasing");
  }
  for (int l = 0; l < c.nl; ++l)
    if (!interp::finite(c.levels[l])) throw ArgError(who + ": every level must be finite");
}

void launch_time_stats(hipStream_t stream, const Args& A, double* scratch) {
  if (A.n < 1 || A.B < 2 || A.nl < 0 || A.nl > kMaxLevels) throw ArgError("time_stats: nothing to launch");
  const long long nwg = reduce::workgroups(A.n);
  if (nwg > INT_MAX) throw ArgError("time_stats: more than INT_MAX workgroups");
  const dim3 grid((unsigned)nwg, (unsigned)(1 + level_chunks(A.nl)));
  hipLaunchKernelGGL(stats_kernel, grid, dim3(kThreads), 0, stream, A, scratch, (int)nwg);
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)(1 + A.nl)), dim3(kThreads), 0, stream, scratch, (int)nwg,
                     scratch + results_offset((size_t)A.nl, (size_t)nwg));
}

void time_stats_host(const Args& A, double* out) {
  const size_t rows = 1 + (size_t)A.nl;
  std::vector<levelset::SerialSum> sum(rows * 3);
  for (size_t r = 0; r < rows; ++r) NoItems{}(out + r * kCols);
  const auto add = [&](size_t r, const double* c) {
    for (int k = 0; k < 3; ++k) sum[r * 3 + k].add(c[k]);
    out[r * kCols + 3] = nanmax(out[r * kCols + 3], c[3]);
    out[r * kCols + 4] = nanmax(out[r * kCols + 4], c[4]);
  };
  for (size_t i = 0; i < (size_t)A.n; ++i) {
    double col[kNodeCols], c[kCols];
    node_columns(A, i, col);
    std::copy(col, col + kNodeCols, A.node + i * kNodeCols);
    node_term(A.w[i], col, c);
    add(0, c);
  }
  for (int l0 = 0; l0 < A.nl; l0 += kChunk) {
    const int cnt = std::min(kChunk, A.nl - l0);
    for (size_t i = 0; i < (size_t)A.n; ++i) {
      double col[kChunk][kLevelCols], c[kCols];
      level_columns(A, i, l0, cnt, col);
      for (int k = 0; k < cnt; ++k) {
        std::copy(col[k], col[k] + kLevelCols, A.level + ((size_t)(l0 + k) * (size_t)A.n + i) * kLevelCols);
        level_term(A.w[i], col[k], c);
        add(1 + (size_t)(l0 + k), c);
      }
    }
  }
  for (size_t r = 0; r < rows; ++r)
    for (int k = 0; k < 3; ++k) out[r * kCols + k] = sum[r * 3 + k].value();
}

}  // namespace timestat
}  // namespace mgb
