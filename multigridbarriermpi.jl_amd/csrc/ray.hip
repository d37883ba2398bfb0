// Line integrals of nodal fields on gfx950.  B fields x m segments on one geometry are integrated by
// ONE plain launch on one stream, the scheme of flowline.hip:
//   measure_kernel<DIM, K, W>: grid (ceil(m / W), B) of W threads; one lane per (ray, field) runs ray.hpp's integrate(): it
//     walks its segment through the bin grid and writes its own row of 8 doubles and its number of owned pieces.  No atomics,
//     no LDS, no barrier: a lane that finishes leaves the loop, the wave lives as long as its longest ray.
// Where pieces are asked for, after the counts have reached the host and their exclusive sums have come back:
//   emit_kernel<DIM, K, W>: the same grid; every lane walks its segment again and writes its pieces (t0, t1, int u) and their
//     elements at its own offsets of the CSR arrays.  There is no fixed-stride buffer.
// What a row's result is made of depends on its field and its ray alone, never on B, m, W or the row's place in the batch.
// This file is compiled with fp contraction off (build.sh): kernels and host restatement run integrate() with the same operations.
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

// Every function of the project's headers is inlined in this file, as in flowline.hip and section.hip, so that this object file
// carries its OWN contraction-free copy of interp.hpp's bases and locator: left out of line they are weak symbols, which the
// linker merges with the copies of the files compiled with contraction on, and the bits of this host restatement would depend
// on the link order.  (The standard headers are included above, outside the pragma.)
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "ray.hpp"
#pragma clang attribute pop

namespace mgb {
namespace ray {
namespace {

template <int DIM, int K, int W>
__global__ void __launch_bounds__(W) measure_kernel(Args A) {
  const long long i = (long long)blockIdx.x * W + threadIdx.x;
  if (i >= A.m) return;
  const size_t row = (size_t)blockIdx.y * A.m + i;
  integrate<DIM, K>(A, A.z[blockIdx.y], A.a + (size_t)i * DIM, A.b + (size_t)i * DIM, A.rows + row * kCols, A.count + row, nullptr,
                    nullptr, 0);
}

template <int DIM, int K, int W>
__global__ void __launch_bounds__(W) emit_kernel(Args A, const long long* __restrict__ offsets, double* __restrict__ piece,
                                                 int32_t* __restrict__ elem) {
  const long long i = (long long)blockIdx.x * W + threadIdx.x;
  if (i >= A.m) return;
  const size_t row = (size_t)blockIdx.y * A.m + i;
  const long long at = offsets[row], cap = offsets[row + 1] - at;
  if (cap <= 0) return;
  integrate<DIM, K>(A, A.z[blockIdx.y], A.a + (size_t)i * DIM, A.b + (size_t)i * DIM, nullptr, nullptr,
                    piece + (size_t)at * kPieceWidth, elem + (size_t)at, cap);
}

template <int DIM, int K>
void launch_kind(hipStream_t stream, const Args& A, int wg, const long long* offsets, double* piece, int32_t* elem) {
  const dim3 grid((unsigned)(((long long)A.m + wg - 1) / wg), (unsigned)A.B);      // 64-bit: m may be within wg of INT_MAX
  if (offsets == nullptr) {
    if (wg == 64) hipLaunchKernelGGL((measure_kernel<DIM, K, 64>), grid, dim3(64), 0, stream, A);
    else if (wg == 128) hipLaunchKernelGGL((measure_kernel<DIM, K, 128>), grid, dim3(128), 0, stream, A);
    else hipLaunchKernelGGL((measure_kernel<DIM, K, 256>), grid, dim3(256), 0, stream, A);
  } else {
    if (wg == 64) hipLaunchKernelGGL((emit_kernel<DIM, K, 64>), grid, dim3(64), 0, stream, A, offsets, piece, elem);
    else if (wg == 128) hipLaunchKernelGGL((emit_kernel<DIM, K, 128>), grid, dim3(128), 0, stream, A, offsets, piece, elem);
    else hipLaunchKernelGGL((emit_kernel<DIM, K, 256>), grid, dim3(256), 0, stream, A, offsets, piece, elem);
  }
}

void launch_any(hipStream_t stream, int dim, int k, const Args& A, int wg, const long long* offsets, double* piece, int32_t* elem) {
  if (wg != 64 && wg != 128 && wg != 256) throw ArgError("line_integrals: the workgroup size is 64, 128 or 256");
  if (A.m <= 0 || A.B < 1 || A.B > 65535) return;
  if (dim == 2) launch_kind<2, 0>(stream, A, wg, offsets, piece, elem);
  else if (dim == 3 && k == 1) launch_kind<3, 1>(stream, A, wg, offsets, piece, elem);
  else if (dim == 3 && k == 2) launch_kind<3, 2>(stream, A, wg, offsets, piece, elem);
  else if (dim == 3 && k == 3) launch_kind<3, 3>(stream, A, wg, offsets, piece, elem);
  else throw InternalError("line_integrals: unknown element kind");
}

template <int DIM, int K>
void host_rows(const Args& A, long long* offsets, double* piece, int32_t* elem, long long capacity) {
  long long at = 0;
  for (int b = 0; b < A.B; ++b)
    for (int i = 0; i < A.m; ++i) {
      const size_t row = (size_t)b * A.m + i;
      const long long cap = offsets ? capacity - at : 0;
      integrate<DIM, K>(A, A.z[b], A.a + (size_t)i * DIM, A.b + (size_t)i * DIM, A.rows + row * kCols, A.count + row,
                        offsets ? piece + (size_t)at * kPieceWidth : nullptr, offsets ? elem + (size_t)at : nullptr, cap);
      if (!offsets) continue;
      offsets[row] = at;
      if (A.count[row] > cap) throw ArgError("line_integrals_host: more pieces than the arrays hold");
      at += A.count[row];
    }
  if (offsets) offsets[(size_t)A.B * A.m] = at;
}

}  // namespace

void check(const std::string& who, const Call& c) {
  if (c.null_argument) throw ArgError(who + ": null argument");
  if (c.dim != 2 && c.dim != 3)
    throw ArgError(who + ": a 2-D or 3-D geometry is needed; the value of a 1-D field at a point comes from interpolate");
  if (c.B < 1 || c.B > 65535) throw ArgError(who + ": B must be 1..65535");
  if (!(interp::finite(c.p) && c.p >= 1.0)) throw ArgError(who + ": p must be one finite real >= 1");
  if (c.S < 1) throw ArgError(who + ": S must be >= 1");
  if (c.u < 0 || c.u >= c.S) throw ArgError(who + ": column u outside [0, S)");
  if (c.m < 0) throw ArgError(who + ": m must be >= 0");
  if ((long long)c.B * c.m > (long long)INT_MAX) throw ArgError(who + ": more than INT_MAX rows (fields x rays) per call");
  if (c.workgroup != 0 && c.workgroup != 64 && c.workgroup != 128 && c.workgroup != 256)
    throw ArgError(who + ": the workgroup size is 0 (default), 64, 128 or 256");
  if (c.field_len)
    for (int b = 0; b < c.B; ++b) {
      if (c.field_len[b] == -1) throw ArgError(who + ": null field");
      if (c.field_len[b] == -2) throw ArgError(who + ": vectors of another context");
      if (c.field_len[b] != c.want_len) throw ArgError(who + ": every z must hold n x S values");
    }
  if (c.world != 1) throw ArgError(who + ": sharded contexts are not supported");
}

void launch_measure(hipStream_t stream, int dim, int k, const Args& A, int wg) {
  launch_any(stream, dim, k, A, wg, nullptr, nullptr, nullptr);
}

void launch_emit(hipStream_t stream, int dim, int k, const Args& A, int wg, const long long* offsets, double* piece, int32_t* elem) {
  if (!offsets || !piece || !elem) throw InternalError("line_integrals: the emit launch needs offsets, pieces and elements");
  launch_any(stream, dim, k, A, wg, offsets, piece, elem);
}

void line_integrals_host(int dim, int k, const Args& A, long long* offsets, double* piece, int32_t* elem, long long capacity) {
  if (offsets && (!piece || !elem || capacity < 0)) throw ArgError("line_integrals_host: offsets, pieces and elements come together");
  if (dim == 2) host_rows<2, 0>(A, offsets, piece, elem, capacity);
  else if (dim == 3 && k == 1) host_rows<3, 1>(A, offsets, piece, elem, capacity);
  else if (dim == 3 && k == 2) host_rows<3, 2>(A, offsets, piece, elem, capacity);
  else if (dim == 3 && k == 3) host_rows<3, 3>(A, offsets, piece, elem, capacity);
  else throw InternalError("line_integrals: unknown element kind");
}

}  // namespace ray
}  // namespace mgb
