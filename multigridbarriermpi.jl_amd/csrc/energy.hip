// Energy, flux and cone margin of nodal fields on gfx950.  B fields on one geometry are reduced by ONE
// pair of plain launches on one stream:
//   energy_kernel<DIM, K>: grid (workgroups(n), B); one thread per node of field blockIdx.y runs energy.hpp's Node (own basis,
//     gradient of column u, the five contributions); the workgroup reduces them -- wave shuffles, then LDS across the four
//     waves, the three sums and the two maxima together -- and writes ONE partial row per (field, workgroup);
//   energy_finish: grid (B); the workgroup of a field combines that field's partials in ascending workgroup order (thread t
//     takes the t-th contiguous run of workgroups, then the same tree) and writes its 5 doubles.
// The fields come as a device table of B pointers: the snapshots of a parabolic run are separate allocations and are not copied.
// What a field's result is made of depends on n alone, never on B or on the field's place in the batch: a batch gives the bits
// of its fields reduced one by one.  No atomics and no hand-off between workgroups inside a launch; every word is written by
// one thread with a vector store.
//   flux_kernel<DIM, K>: one thread per node writes sigma = a^(p-2) g, dim doubles.
#include "energy.hpp"

namespace mgb {
namespace energy {
namespace {

static_assert(kThreads == 256, "four waves of 64");
constexpr int kWaves = kThreads / 64;

// Reduce c[0..4] over the workgroup; the result is valid in thread 0.
__device__ inline void block_combine(double* c, double (*red)[kCols]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double t[kCols];
#pragma unroll
    for (int k = 0; k < kCols; ++k) t[k] = __shfl_down(c[k], o, 64);
    combine(c, t);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kCols; ++k) red[wave][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 1; v < kWaves; ++v) combine(c, red[v]);
  }
}

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) energy_kernel(Args A, double* __restrict__ partials) {
  __shared__ double red[kWaves][kCols];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int b = blockIdx.y;
  double c[kCols];
  identity(c);      // idle threads of the last workgroup stay for the reduction and contribute nothing
  if (i < A.n) {
    Node<DIM, K> N;
    N.init(A, (int)i);
    N.contributions(A, A.z[b], A.f ? A.f + (size_t)b * A.f_stride : nullptr, c);
  }
  block_combine(c, red);
  if (threadIdx.x == 0) {
    double* row = partials + ((size_t)b * gridDim.x + blockIdx.x) * kCols;
#pragma unroll
    for (int k = 0; k < kCols; ++k) row[k] = c[k];
  }
}

__global__ void __launch_bounds__(kThreads) energy_finish(const double* __restrict__ partials, int nwg, double* __restrict__ out) {
  __shared__ double red[kWaves][kCols];
  const int b = blockIdx.x;
  const int chunk = (nwg + kThreads - 1) / kThreads;
  const long long b0 = (long long)threadIdx.x * chunk;
  const long long b1 = b0 + chunk < nwg ? b0 + chunk : nwg;
  double c[kCols];
  identity(c);
  for (long long g = b0; g < b1; ++g) combine(c, partials + ((size_t)b * nwg + g) * kCols);
  block_combine(c, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kCols; ++k) out[(size_t)b * kCols + k] = c[k];
  }
}

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) flux_kernel(Args A, const double* __restrict__ z, double* __restrict__ flux) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.n) return;
  Node<DIM, K> N;
  N.init(A, (int)i);
  double sigma[DIM];
  N.flux(z, A.S, A.u, sigma);
#pragma unroll
  for (int k = 0; k < DIM; ++k) flux[(size_t)i * DIM + k] = sigma[k];
}

struct LaunchEnergy {
  hipStream_t stream;
  Args A;
  double* scratch;
  template <int DIM, int K>
  void operator()() const {
    const long long nwg = workgroups(A.n);
    hipLaunchKernelGGL((energy_kernel<DIM, K>), dim3((unsigned)nwg, (unsigned)A.B), dim3(kThreads), 0, stream, A, scratch);
    hipLaunchKernelGGL(energy_finish, dim3((unsigned)A.B), dim3(kThreads), 0, stream, scratch, (int)nwg,
                       scratch + (size_t)nwg * A.B * kCols);
  }
};

struct LaunchFlux {
  hipStream_t stream;
  Args A;
  const double* z;
  double* flux;
  template <int DIM, int K>
  void operator()() const {
    hipLaunchKernelGGL((flux_kernel<DIM, K>), dim3((unsigned)workgroups(A.n)), dim3(kThreads), 0, stream, A, z, flux);
  }
};

}  // namespace

void launch_field_energy(hipStream_t stream, int dim, int k, const Args& A, double* scratch) {
  if (A.n <= 0 || A.S <= 0 || A.B <= 0 || A.B > 65535) throw ArgError("field_energy: empty field, or more than 65535 fields");
  LaunchEnergy l{stream, A, scratch};
  interp::dispatch(dim, k, l);
}

void launch_field_flux(hipStream_t stream, int dim, int k, const Args& A, const double* z, double* flux) {
  if (A.n <= 0 || A.S <= 0) throw ArgError("field_flux: empty field");
  LaunchFlux l{stream, A, z, flux};
  interp::dispatch(dim, k, l);
}

}  // namespace energy
}  // namespace mgb
