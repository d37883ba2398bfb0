// Step transition of parabolic_solve on gfx950: see parabolic.hpp.  Streaming wave64 kernels, one thread per node; the column
// reads of z (u, s1, s2 at stride n) are coalesced, the rows of Dz0 / c are K <= 6 contiguous doubles per thread.
// Where the result is compared bit for bit with numpy (the cost, u^2 - s1, the squared gradient) the arithmetic is kept as
// written: `#pragma clang fp contract(off)` keeps a product and the sum behind it from fusing into one fma.
#include "parabolic.hpp"

#include <cmath>

#include "errors.hpp"

namespace mgb {
namespace parabolic {
namespace {

__global__ void __launch_bounds__(kThreads) cost_kernel(int n, int K, double h, double c_s1, double c_s2, const double* __restrict__ f,
                                                        const double* __restrict__ z, double* __restrict__ c) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double* row = c + (size_t)i * K;
  row[0] = f[i] - z[i] / h;
  for (int k = 1; k < K - 2; ++k) row[k] = 0.0;
  row[K - 2] = c_s1;
  row[K - 1] = c_s2;
}

__global__ void __launch_bounds__(kThreads) boundary_kernel(int nb, const int* __restrict__ bidx, const double* __restrict__ gb,
                                                            double* __restrict__ z) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j < nb) z[bidx[j]] = gb[j];
}

__device__ inline bool finite(double v) { return (v - v) == 0.0; }

__global__ void __launch_bounds__(kThreads) violations_kernel(int n, int K, double half_p, const double* __restrict__ z,
                                                              const double* __restrict__ Dz0, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double red[kWaves][2];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  // idle threads of the last workgroup stay for the reduction and contribute the identity of max
  double v[2] = {-HUGE_VAL, -HUGE_VAL};
  if (i < n) {
    const double u = z[i], s1 = z[(size_t)n + i], s2 = z[(size_t)2 * n + i];
    const double* row = Dz0 + (size_t)i * K;
    double gs = 0.0;
    for (int d = 1; d < K - 2; ++d) gs = gs + row[d] * row[d];
    if (finite(u) && finite(s1) && finite(s2) && finite(gs)) {
      v[0] = u * u - s1;
      const double gp = half_p == 1.0 ? gs : (half_p == 0.5 ? sqrt(gs) : (gs == 0.0 ? 0.0 : pow(gs, half_p)));
      v[1] = gp - s2;
    } else {
      v[0] = v[1] = NAN;
    }
  }
  block_reduce<2>(v, NanMax<2>{}, red);
  if (threadIdx.x == 0) {
    partials[(size_t)blockIdx.x * 2] = v[0];
    partials[(size_t)blockIdx.x * 2 + 1] = v[1];
  }
}

__device__ inline double lift_of(double v) { return v != v ? v : (v >= 0.0 ? 1.0 + v : 0.0); }

// one workgroup finishes the partial pairs (reduce.hpp); out = v1, v2, lift_1, lift_2
__global__ void __launch_bounds__(kThreads) violations_finish(const double* __restrict__ partials, int nwg, double* __restrict__ out) {
  __shared__ double red[kWaves][2];
  const Run r = run_of(threadIdx.x, nwg);
  double v[2] = {-HUGE_VAL, -HUGE_VAL};
  for (long long b = r.b0; b < r.b1; ++b) NanMax<2>{}(v, partials + (size_t)b * 2);
  block_reduce<2>(v, NanMax<2>{}, red);
  if (threadIdx.x == 0) {
    out[0] = v[0];
    out[1] = v[1];
    out[2] = lift_of(v[0]);
    out[3] = lift_of(v[1]);
  }
}

__global__ void __launch_bounds__(kThreads) lift_kernel(int n, const double* __restrict__ lifts2, double* __restrict__ z) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double l1 = lifts2[0], l2 = lifts2[1];
  if (l1 != 0.0) z[(size_t)n + i] += l1;      // a zero lift leaves its column untouched, bit for bit
  if (l2 != 0.0) z[(size_t)2 * n + i] += l2;
}

__global__ void __launch_bounds__(kThreads) snapshot_kernel(int n, int S, const double* __restrict__ z, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  for (int s = 0; s < S; ++s) out[(size_t)i * S + s] = z[(size_t)s * n + i];
}

inline dim3 grid_of(int n) { return dim3((unsigned)workgroups(n)); }

}  // namespace

void launch_cost(hipStream_t stream, int n, int K, double h, double c_s1, double c_s2, const double* f, const double* z, double* c) {
  if (n <= 0 || K < 4) throw ArgError("parabolic cost: empty problem or fewer than 4 rows of D");
  hipLaunchKernelGGL(cost_kernel, grid_of(n), dim3(kThreads), 0, stream, n, K, h, c_s1, c_s2, f, z, c);
}

void launch_boundary(hipStream_t stream, int nb, const int* bidx, const double* gb, double* z) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(boundary_kernel, grid_of(nb), dim3(kThreads), 0, stream, nb, bidx, gb, z);
}

void launch_violations(hipStream_t stream, int n, int K, double p, const double* z, const double* Dz0, double* scratch) {
  if (n <= 0 || K < 4) throw ArgError("parabolic violations: empty problem or fewer than 4 rows of D");
  const long long nwg = workgroups(n);
  hipLaunchKernelGGL(violations_kernel, dim3((unsigned)nwg), dim3(kThreads), 0, stream, n, K, p / 2.0, z, Dz0, scratch);
  hipLaunchKernelGGL(violations_finish, dim3(1), dim3(kThreads), 0, stream, scratch, (int)nwg, scratch + results_offset(n));
}

void launch_lift(hipStream_t stream, int n, const double* lifts2, double* z) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lift_kernel, grid_of(n), dim3(kThreads), 0, stream, n, lifts2, z);
}

void launch_snapshot(hipStream_t stream, int n, int S, const double* z, double* out) {
  if (n <= 0 || S <= 0) return;
  hipLaunchKernelGGL(snapshot_kernel, grid_of(n), dim3(kThreads), 0, stream, n, S, z, out);
}

}  // namespace parabolic
}  // namespace mgb
