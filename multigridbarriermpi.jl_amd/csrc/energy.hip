// Energy, flux and cone margin of nodal fields on gfx950.  B fields on one geometry are reduced by ONE
// pair of plain launches on one stream, the two stages of reduce.hpp:
//   energy_kernel<DIM, K>: grid (workgroups(n), B); one thread per node of field blockIdx.y runs energy.hpp's Node (own basis,
//     gradient of column u, the five contributions); the workgroup reduces them and writes ONE partial row per (field,
//     workgroup);
//   reduce::launch_finish: grid (B); the workgroup of a field finishes that field's partials and writes its 5 doubles.
// The fields come as a device table of B pointers: the snapshots of a parabolic run are separate allocations and are not copied.
// What a field's result is made of depends on n alone, never on B or on the field's place in the batch: a batch gives the bits
// of its fields reduced one by one.
//   flux_kernel<DIM, K>: grid (workgroups(n), B); one thread per node of field blockIdx.y writes sigma = a^(p-2) g, dim
//     doubles, into row blockIdx.y of flux (B x n x dim).  The fields come through the device table A.z, or, where A.z is null,
//     as the ONE field z (mgb_geo_field_flux, mgb_estimate: no table to upload).
#include "energy.hpp"

namespace mgb {
namespace energy {
namespace {

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
  block_reduce<kCols>(c, Combine{}, red);
  if (threadIdx.x == 0) {
    double* row = partials + ((size_t)b * gridDim.x + blockIdx.x) * kCols;
#pragma unroll
    for (int k = 0; k < kCols; ++k) row[k] = c[k];
  }
}

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) flux_kernel(Args A, const double* __restrict__ z, double* __restrict__ flux) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.n) return;      // no barrier in this kernel
  const int b = blockIdx.y;
  Node<DIM, K> N;
  N.init(A, (int)i);
  double sigma[DIM];
  N.flux(A.z ? A.z[b] : z, A.S, A.u, sigma);
#pragma unroll
  for (int k = 0; k < DIM; ++k) flux[((size_t)b * A.n + i) * DIM + k] = sigma[k];
}

struct LaunchEnergy {
  hipStream_t stream;
  Args A;
  double* scratch;
  template <int DIM, int K>
  void operator()() const {
    const long long nwg = workgroups(A.n);
    hipLaunchKernelGGL((energy_kernel<DIM, K>), dim3((unsigned)nwg, (unsigned)A.B), dim3(kThreads), 0, stream, A, scratch);
    launch_finish(stream, A.B, scratch, (int)nwg, (size_t)nwg * kCols, kCols, scratch + results_offset(A.n, A.B));
  }
};

struct LaunchFlux {
  hipStream_t stream;
  Args A;
  const double* z;
  double* flux;
  template <int DIM, int K>
  void operator()() const {
    hipLaunchKernelGGL((flux_kernel<DIM, K>), dim3((unsigned)workgroups(A.n), (unsigned)A.B), dim3(kThreads), 0, stream, A, z, flux);
  }
};

}  // namespace

void launch_field_energy(hipStream_t stream, int dim, int k, const Args& A, double* scratch) {
  if (A.n <= 0 || A.S <= 0 || A.B <= 0 || A.B > 65535) throw ArgError("field_energy: empty field, or more than 65535 fields");
  LaunchEnergy l{stream, A, scratch};
  interp::dispatch(dim, k, l);
}

void launch_field_flux(hipStream_t stream, int dim, int k, const Args& A, const double* z, double* flux) {
  if (A.n <= 0 || A.S <= 0 || A.B <= 0 || A.B > 65535) throw ArgError("field_flux: empty field, or more than 65535 fields");
  if ((A.z == nullptr) == (z == nullptr) || (z && A.B != 1)) throw ArgError("field_flux: one field, or a table of B fields");
  LaunchFlux l{stream, A, z, flux};
  interp::dispatch(dim, k, l);
}

}  // namespace energy
}  // namespace mgb
