// Path lines through the snapshots of a parabolic run on gfx950.  m particles on one geometry are
// carried from their release times to ts[stop] by ONE plain launch on one stream:
//   advance_kernel<DIM, K, W>: grid ceil(m / W) of W threads; one thread per seed runs pathline.hpp's advance() and writes its
//     own row, end point, status, count, end element, rested count and, with paths, its own row of A.stride slots.  The
//     snapshots come through a device pointer table, the times and the release indices are device arrays.  No atomics, no
//     LDS, no barrier: a lane that finishes leaves the loop, the wave lives as long as its longest trajectory.
// Where paths are asked for the rows are gathered by flowline.hip's compact_kernel (launch_compact), unchanged.
// What a row's result is made of depends on its seed, its release index and the fields alone, never on m, W or the row's place
// in the batch.  This file is compiled with fp contraction off (build.sh): kernel and host restatement run advance() with the
// same operations.
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

// Every function of the project's headers is inlined in this file, as in flowline.hip and section.hip: this object file
// carries its own contraction-free copies of interp.hpp's and flowline.hpp's routines and defines no weak function that the
// linker could merge with another object's.  (The standard headers are included above, outside the pragma.)
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "pathline.hpp"
#pragma clang attribute pop

namespace mgb {
namespace pathline {
namespace {

template <int DIM, int K, int W>
__global__ void __launch_bounds__(W) advance_kernel(Args A) {
  const int i = (int)blockIdx.x * W + (int)threadIdx.x;
  if (i >= A.m) return;
  const size_t row = (size_t)i;
  advance<DIM, K>(A, A.seeds + row * DIM, A.release[i], A.rows + row * kRowCols, A.end + row * DIM, A.status + row, A.count + row,
                  A.end_element + row, A.rested + row, A.pts ? A.pts + row * (size_t)A.stride * DIM : nullptr,
                  A.pts ? A.pelem + row * (size_t)A.stride : nullptr);
}

template <int DIM, int K>
void launch_kind(hipStream_t stream, const Args& A, int wg) {
  const dim3 grid((unsigned)((A.m + wg - 1) / wg));
  if (wg == 64) hipLaunchKernelGGL((advance_kernel<DIM, K, 64>), grid, dim3(64), 0, stream, A);
  else if (wg == 128) hipLaunchKernelGGL((advance_kernel<DIM, K, 128>), grid, dim3(128), 0, stream, A);
  else hipLaunchKernelGGL((advance_kernel<DIM, K, 256>), grid, dim3(256), 0, stream, A);
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
  for (int i = 0; i < A.m; ++i) {
    const size_t row = (size_t)i;
    advance<DIM, K>(A, A.seeds + row * DIM, A.release[i], A.rows + row * kRowCols, A.end + row * DIM, A.status + row, A.count + row,
                    A.end_element + row, A.rested + row, offsets ? rp.data() : nullptr, offsets ? re.data() : nullptr);
    if (!offsets) continue;
    offsets[row] = at;
    const long long n = A.count[row];
    if (at + n > capacity) throw ArgError("path_lines_host: more points than the arrays hold");
    std::copy(rp.begin(), rp.begin() + (size_t)n * DIM, pts + (size_t)at * DIM);
    std::copy(re.begin(), re.begin() + (size_t)n, pelem + (size_t)at);
    at += n;
  }
  if (offsets) offsets[(size_t)A.m] = at;
}

}  // namespace

void check(const char* who, const Call& c, Args& A) {
  const std::string w(who);
  if (c.null_argument) throw ArgError(w + ": null argument");
  if (c.dim != 2 && c.dim != 3) throw ArgError(w + ": path lines need a 2-D or 3-D geometry");
  if (c.B < 2 || c.B > 65535) throw ArgError(w + ": B must be 2..65535");
  if (c.S < 1) throw ArgError(w + ": S must be >= 1");
  if (c.u < 0 || c.u >= c.S) throw ArgError(w + ": column u outside [0, S)");
  if (c.m < 0) throw ArgError(w + ": m must be >= 0");
  for (int b = 0; b < c.B; ++b) {
    if (!interp::finite(c.ts[b])) throw ArgError(w + ": every time must be finite");
    if (b > 0 && !(c.ts[b] > c.ts[b - 1])) throw ArgError(w + ": the times must be strictly increasing");
  }
  if (c.stop < 1 || c.stop > c.B - 1) throw ArgError(w + ": stop outside [1, B - 1]");
  if (c.substeps < 1) throw ArgError(w + ": substeps must be >= 1");
  if (!(interp::finite(c.p) && c.p >= 1.0)) throw ArgError(w + ": p must be finite and >= 1");
  if (!(interp::finite(c.speed) && c.speed > 0.0)) throw ArgError(w + ": speed must be finite and > 0");
  if (!(interp::finite(c.gmin) && c.gmin >= 0.0)) throw ArgError(w + ": gmin must be finite and >= 0");
  if (c.direction != 1 && c.direction != -1) throw ArgError(w + ": direction must be +1 or -1");
  if (c.workgroup != 0 && c.workgroup != 64 && c.workgroup != 128 && c.workgroup != 256)
    throw ArgError(w + ": the workgroup size is 0 (default), 64, 128 or 256");
  int first = c.m > 0 ? c.stop : 0;
  for (int i = 0; i < c.m; ++i) {
    if (c.release[i] < 0 || c.release[i] >= c.stop) throw ArgError(w + ": a release index outside [0, stop)");
    first = std::min(first, (int)c.release[i]);
  }
  if (c.world != 1) throw ArgError(w + ": sharded contexts are not supported");
  if (c.field_len)
    for (int b = 0; b < c.B; ++b) {
      if (c.field_len[b] == -1) throw ArgError(w + ": null field");
      if (c.field_len[b] == -2) throw ArgError(w + ": vectors of another context");
      if (c.field_len[b] != c.want_len) throw ArgError(w + ": every z must hold n x S values");
    }
  const long long stride = (long long)(c.stop - first) * c.substeps + 2;
  // m stride dim <= INT_MAX, without overflow: m and dim are at most INT_MAX, stride at most 2^47
  if (c.paths && c.m > 0 && stride > (long long)INT_MAX / ((long long)c.m * c.dim))
    throw ArgError(w + ": the path buffer of m ((stop - min release) substeps + 2) dim doubles has more than 2^31 - 1 entries");
  A.p = c.p, A.sgn = (double)c.direction, A.speed = c.speed, A.gmin = c.gmin;
  A.m = c.m, A.S = c.S, A.u = c.u, A.B = c.B, A.stop = c.stop, A.substeps = c.substeps;
  A.stride = stride;
}

void launch_advance(hipStream_t stream, int dim, int k, const Args& A, int wg) {
  if (wg != 64 && wg != 128 && wg != 256) throw InternalError("path_lines: the workgroup size is 64, 128 or 256");
  if (A.m == 0) return;
  if (dim == 2) launch_kind<2, 0>(stream, A, wg);
  else if (dim == 3 && k == 1) launch_kind<3, 1>(stream, A, wg);
  else if (dim == 3 && k == 2) launch_kind<3, 2>(stream, A, wg);
  else if (dim == 3 && k == 3) launch_kind<3, 3>(stream, A, wg);
  else throw InternalError("path_lines: unknown element kind");
}

void path_lines_host(int dim, int k, const Args& A, long long* offsets, double* pts, int32_t* pelem, long long capacity) {
  if (dim == 2) host_rows<2, 0>(A, offsets, pts, pelem, capacity);
  else if (dim == 3 && k == 1) host_rows<3, 1>(A, offsets, pts, pelem, capacity);
  else if (dim == 3 && k == 2) host_rows<3, 2>(A, offsets, pts, pelem, capacity);
  else if (dim == 3 && k == 3) host_rows<3, 3>(A, offsets, pts, pelem, capacity);
  else throw InternalError("path_lines: unknown element kind");
}

}  // namespace pathline
}  // namespace mgb
