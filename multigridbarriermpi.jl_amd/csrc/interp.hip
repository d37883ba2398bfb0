// Evaluation of a nodal field at arbitrary points on gfx950: one thread per query point runs
// interp.hpp's eval_point -- cell lookup, walk of the ascending candidate list, basis once, loop over the S columns.
// No atomics, no LDS, no cross-thread communication: every output word is written by exactly one thread from its own inputs,
// so the result is bitwise reproducible from run to run.
#include "interp.hpp"

namespace mgb {
namespace interp {
namespace {

constexpr int kThreads = 256;

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads)
interp_kernel(BinsView B, int m, const double* __restrict__ pts, int S, const double* __restrict__ z, double* __restrict__ vals,
              double* __restrict__ grads, int32_t* __restrict__ elem) {
  const long long q = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (q >= m) return;
  double p[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) p[d] = pts[(size_t)q * DIM + d];
  eval_point<DIM, K>(B, p, S, z, vals + (size_t)q * S, grads ? grads + (size_t)q * S * DIM : nullptr, elem ? elem + q : nullptr);
}

struct Launch {
  hipStream_t stream;
  BinsView B;
  int m, S;
  const double *pts, *z;
  double *vals, *grads;
  int32_t* elem;
  template <int DIM, int K>
  void operator()() const {
    const unsigned blocks = (unsigned)(((long long)m + kThreads - 1) / kThreads);
    hipLaunchKernelGGL((interp_kernel<DIM, K>), dim3(blocks), dim3(kThreads), 0, stream, B, m, pts, S, z, vals, grads, elem);
  }
};

}  // namespace

void launch_interpolate(hipStream_t stream, const BinsView& B, int dim, int k, int m, const double* pts, int S, const double* z,
                        double* vals, double* grads, int32_t* elem) {
  if (m <= 0) return;
  Launch l{stream, B, m, S, pts, z, vals, grads, elem};
  dispatch(dim, k, l);
}

}  // namespace interp
}  // namespace mgb
