// The finish launch of the two-stage field reductions on gfx950: see reduce.hpp.
#include "reduce.hpp"

#include "errors.hpp"

namespace mgb {
namespace reduce {
namespace {

__global__ void __launch_bounds__(kThreads) finish_kernel(const double* __restrict__ partials, int nwg, size_t row_stride,
                                                          size_t wg_stride, double* __restrict__ out) {
  __shared__ double red[kWaves][kCols];
  finish_row(partials + blockIdx.x * row_stride, wg_stride, nwg, red, out + (size_t)blockIdx.x * kCols);
}

}  // namespace

void launch_finish(hipStream_t stream, int rows, const double* partials, int nwg, size_t row_stride, size_t wg_stride, double* out) {
  if (rows < 1 || nwg < 1) throw ArgError("reduce finish: no row or no partial");
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)rows), dim3(kThreads), 0, stream, partials, nwg, row_stride, wg_stride, out);
}

}  // namespace reduce
}  // namespace mgb
