// Flow lines of nodal fields on gfx950.  B fields x m seeds on one geometry are traced by ONE plain
// launch on one stream:
//   trace_kernel<DIM, K, W>: grid (ceil(m / W), B) of W threads; one thread per (seed, field) runs flowline.hpp's trace() and
//     writes its own row, end point, status, count, end element and, with paths, its own row of max_steps + 2 slots.  No
//     atomics, no LDS, no barrier: a lane that finishes leaves the loop, the wave lives as long as its longest line.
// Where paths are asked for, after the counts have reached the host and their exclusive sums have come back:
//   compact_kernel<DIM>: grid (B m) of 64 threads; the workgroup of a row copies the row's count points and elements from the
//     fixed-stride row to the row's place in the CSR arrays.
// What a row's result is made of depends on its field and its seed alone, never on B, m, W or the row's place in the batch.
// This file is compiled with fp contraction off (build.sh): kernel and host restatement run trace() with the same operations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

// Every function of the project's headers is inlined in this file, so that this object file carries its OWN contraction-free
// copy of interp.hpp's bases and locator.  Left out of line they are weak symbols, which the linker merges with the copies of
// the files compiled with contraction on: whichever object came first on the link line would serve both, and either the bits
// of this host restatement or those of the other host restatements would change with the link order.  (The standard headers
// are included above, outside the pragma.)
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "flowline.hpp"
#pragma clang attribute pop

namespace mgb {
namespace flowline {
namespace {

template <int DIM, int K, int W>
__global__ void __launch_bounds__(W) trace_kernel(Args A) {
  const int i = (int)blockIdx.x * W + (int)threadIdx.x;
  if (i >= A.m) return;
  const size_t row = (size_t)blockIdx.y * A.m + i;
  trace<DIM, K>(A, A.z[blockIdx.y], A.seeds + (size_t)i * DIM, A.rows + row * kRowCols, A.end + row * DIM, A.status + row,
                A.count + row, A.end_element + row, A.pts ? A.pts + row * (size_t)A.stride * DIM : nullptr,
                A.pts ? A.pelem + row * (size_t)A.stride : nullptr);
}

template <int DIM>
__global__ void __launch_bounds__(64) compact_kernel(Args A, const long long* __restrict__ offsets, double* __restrict__ pts,
                                                     int32_t* __restrict__ pelem) {
  const size_t row = blockIdx.x;
  const long long at = offsets[row];
  long long n = offsets[row + 1] - at;
  n = n < A.stride ? n : A.stride;      // never beyond the row that was written
  const double* src = A.pts + row * (size_t)A.stride * DIM;
  const int32_t* sel = A.pelem + row * (size_t)A.stride;
  for (long long j = threadIdx.x; j < n * DIM; j += 64) pts[(size_t)at * DIM + j] = src[j];
  for (long long j = threadIdx.x; j < n; j += 64) pelem[(size_t)at + j] = sel[j];
}

template <int DIM, int K>
void launch_kind(hipStream_t stream, const Args& A, int wg) {
  const dim3 grid((unsigned)((A.m + wg - 1) / wg), (unsigned)A.B);
  if (wg == 64) hipLaunchKernelGGL((trace_kernel<DIM, K, 64>), grid, dim3(64), 0, stream, A);
  else if (wg == 128) hipLaunchKernelGGL((trace_kernel<DIM, K, 128>), grid, dim3(128), 0, stream, A);
  else hipLaunchKernelGGL((trace_kernel<DIM, K, 256>), grid, dim3(256), 0, stream, A);
}

template <int DIM, int K>
void host_rows(const Args& A, long long* offsets, double* pts, int32_t* pelem, long long capacity) {
  std::vector<double> rp;
  std::vector<int32_t> re;
  if (offsets && A.m > 0) {
    rp.resize((size_t)A.stride * DIM);
    re.resize((size_t)A.stride);
  }
  long long at = 0;
  for (int b = 0; b < A.B; ++b)
    for (int i = 0; i < A.m; ++i) {
      const size_t row = (size_t)b * A.m + i;
      trace<DIM, K>(A, A.z[b], A.seeds + (size_t)i * DIM, A.rows + row * kRowCols, A.end + row * DIM, A.status + row, A.count + row,
                    A.end_element + row, offsets ? rp.data() : nullptr, offsets ? re.data() : nullptr);
      if (!offsets) continue;
      offsets[row] = at;
      const long long n = A.count[row];
      if (at + n > capacity) throw ArgError("flow_lines_host: more points than the arrays hold");
      std::copy(rp.begin(), rp.begin() + (size_t)n * DIM, pts + (size_t)at * DIM);
      std::copy(re.begin(), re.begin() + (size_t)n, pelem + (size_t)at);
      at += n;
    }
  if (offsets) offsets[(size_t)A.B * A.m] = at;
}

}  // namespace

void check(const Args& A, int dim, bool paths) {
  if (dim != 2 && dim != 3) throw ArgError("flow_lines: a 2-D or 3-D geometry is needed");
  if (A.B < 1 || A.B > 65535) throw ArgError("flow_lines: B must be 1..65535");
  if (A.S < 1) throw ArgError("flow_lines: S must be >= 1");
  if (A.u < 0 || A.u >= A.S) throw ArgError("flow_lines: column u outside [0, S)");
  if (A.m < 0) throw ArgError("flow_lines: m must be >= 0");
  if (!(interp::finite(A.p) && A.p >= 1.0)) throw ArgError("flow_lines: p must be finite and >= 1");
  if (!(A.sgn == 1.0 || A.sgn == -1.0)) throw ArgError("flow_lines: direction must be +1 or -1");
  if (!(interp::finite(A.ds) && A.ds > 0.0)) throw ArgError("flow_lines: ds must be finite and > 0");
  if (A.max_steps < 1) throw ArgError("flow_lines: max_steps must be >= 1");
  if (!(interp::finite(A.gmin) && A.gmin >= 0.0)) throw ArgError("flow_lines: gmin must be finite and >= 0");
  if ((long long)A.B * A.m > (long long)INT_MAX) throw ArgError("flow_lines: more than INT_MAX rows (fields x seeds) per call");
  if (A.stride != (long long)A.max_steps + 2) throw ArgError("flow_lines: the stride of a row is max_steps + 2");
  // B m (max_steps + 2) dim <= INT_MAX, without overflow: every factor is at most INT_MAX
  if (paths && (long long)A.B * A.m > 0 && A.stride * dim > (long long)INT_MAX / ((long long)A.B * A.m))
    throw ArgError("flow_lines: the path buffer of B m (max_steps + 2) dim doubles has more than 2^31 - 1 entries");
}

void launch_trace(hipStream_t stream, int dim, int k, const Args& A, int wg) {
  check(A, dim, A.pts != nullptr);
  if (wg != 64 && wg != 128 && wg != 256) throw ArgError("flow_lines: the workgroup size is 64, 128 or 256");
  if (A.m == 0) return;
  if (dim == 2) launch_kind<2, 0>(stream, A, wg);
  else if (k == 1) launch_kind<3, 1>(stream, A, wg);
  else if (k == 2) launch_kind<3, 2>(stream, A, wg);
  else if (k == 3) launch_kind<3, 3>(stream, A, wg);
  else throw InternalError("flow_lines: unknown element kind");
}

void launch_compact(hipStream_t stream, int dim, const Args& A, const long long* offsets, double* pts, int32_t* pelem) {
  const unsigned rows = (unsigned)((size_t)A.B * A.m);
  if (rows == 0) return;
  if (dim == 2) hipLaunchKernelGGL(compact_kernel<2>, dim3(rows), dim3(64), 0, stream, A, offsets, pts, pelem);
  else hipLaunchKernelGGL(compact_kernel<3>, dim3(rows), dim3(64), 0, stream, A, offsets, pts, pelem);
}

void flow_lines_host(int dim, int k, const Args& A, long long* offsets, double* pts, int32_t* pelem, long long capacity) {
  check(A, dim, offsets != nullptr);
  if (offsets && (!pts || !pelem || capacity < 0)) throw ArgError("flow_lines_host: offsets, points and elements come together");
  if (dim == 2) host_rows<2, 0>(A, offsets, pts, pelem, capacity);
  else if (k == 1) host_rows<3, 1>(A, offsets, pts, pelem, capacity);
  else if (k == 2) host_rows<3, 2>(A, offsets, pts, pelem, capacity);
  else if (k == 3) host_rows<3, 3>(A, offsets, pts, pelem, capacity);
  else throw InternalError("flow_lines: unknown element kind");
}

}  // namespace flowline
}  // namespace mgb
