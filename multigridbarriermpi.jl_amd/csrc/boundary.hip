// Boundary integrals of nodal fields on gfx950.  B fields on one geometry are reduced over its boundary
// facets by ONE pair of plain launches on one stream, the two stages of reduce.hpp, the way energy.hip reduces over the nodes:
//   boundary_kernel<DIM, K>: grid (workgroups(nf, q), B); a workgroup takes 256 / q whole facets, one thread per (facet, facet
//     node) -- thread t is node t % q of the workgroup's facet t / q, so the facet tables are read contiguously and a facet never
//     straddles two workgroups; threads past the last whole facet, and those of facets the mask leaves out, contribute the
//     identity.  Each thread runs boundary.hpp's Node (sigma through energy.hpp's Node, sigma . n, the tangential part); the
//     workgroup reduces the five columns and writes ONE partial row per (field, workgroup).  With a per-facet output the threads leave omega sigma . n in LDS and node 0 of every facet sums its
//     facet's q values in ascending order.
//   reduce::launch_finish: grid (B); the workgroup of a field finishes that field's partials.
//   boundary_load_kernel / boundary_load_add_kernel: the Neumann load of DESIGN.md section 4i, see below.
// What a field's result is made of depends on the facet list alone, never on B or on the field's place in the batch.
#include "boundary.hpp"

namespace mgb {
namespace boundary {
namespace {

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) boundary_kernel(Args A, double* __restrict__ partials, double* __restrict__ facet_flux) {
  __shared__ double red[kWaves][kCols];
  __shared__ double per_node[kThreads];
  const int q = A.q, fpw = kThreads / q;
  const int lf = threadIdx.x / q, j = threadIdx.x - lf * q;
  const long long f = (long long)blockIdx.x * fpw + lf;
  const int b = blockIdx.y;
  const bool mine = lf < fpw && f < A.nf;      // idle threads stay for the reduction and contribute nothing
  double c[kCols];
  identity(c);
  if (mine && (!A.mask || A.mask[f])) Node<DIM, K>::contributions(A, A.E.z[b], (int)f, j, c);
  if (facet_flux) {      // uniform over the launch
    per_node[threadIdx.x] = c[0];
    __syncthreads();
    if (mine && j == 0) {
      double s = 0.0;
      for (int t = 0; t < q; ++t) s += per_node[threadIdx.x + t];
      facet_flux[(size_t)b * A.nf + f] = s;
    }
  }
  block_reduce<kCols>(c, Combine{}, red);
  if (threadIdx.x == 0) {
    double* row = partials + ((size_t)b * gridDim.x + blockIdx.x) * kCols;
#pragma unroll
    for (int k = 0; k < kCols; ++k) row[k] = c[k];
  }
}

struct LaunchFlux {
  hipStream_t stream;
  Args A;
  double* scratch;
  double* facet_flux;
  template <int DIM, int K>
  void operator()() const {
    const long long nwg = workgroups(A.nf, A.q);
    hipLaunchKernelGGL((boundary_kernel<DIM, K>), dim3((unsigned)nwg, (unsigned)A.E.B), dim3(kThreads), 0, stream, A, scratch,
                       facet_flux);
    // the partials hold boundary.hpp's zeros where reduce::identity has -inf: columns 3 and 4 are absolute values and thread 0
    // always holds a partial, so the finish gives the bits of a zero seed
    launch_finish(stream, A.E.B, scratch, (int)nwg, (size_t)nwg * kCols, kCols, scratch + results_offset(A.nf, A.q, A.E.B));
  }
};

// Neumann load (boundary.hpp: load_row): one thread per distinct boundary row, grid (ceil(nb / 256), B).  rows, start and the
// output are contiguous in the thread index; omega, h and the mask are gathered through the incidence table.  No atomics, no
// LDS, no hand-off: every word of the compact B x nb output is written by one thread with a vector store.
__global__ void __launch_bounds__(kThreads) boundary_load_kernel(LoadArgs A, const double* __restrict__ h, double* __restrict__ out) {
  const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= A.nb) return;
  const size_t b = blockIdx.y;
  out[b * A.nb + r] = load_row(A, h + b * A.nf * A.q, (int)r);
}

__global__ void __launch_bounds__(kThreads) boundary_load_add_kernel(int nb, const int* __restrict__ rows, const double* __restrict__ load,
                                                                     double alpha, long long stride, long long offset,
                                                                     double* __restrict__ y) {
#pragma clang fp contract(off)
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= nb) return;
  const long long at = (long long)rows[j] * stride + offset;
  y[at] = y[at] + alpha * load[j];
}

}  // namespace

void launch_boundary_load(hipStream_t stream, const LoadArgs& A, int B, const double* h, double* out) {
  if (A.nb < 0 || A.nf < 0 || A.q < 1 || B < 1 || B > 65535) throw ArgError("boundary_load: bad incidence table, or B outside [1, 65535]");
  if (A.nb == 0) return;
  const unsigned nwg = (unsigned)reduce::workgroups(A.nb);
  hipLaunchKernelGGL(boundary_load_kernel, dim3(nwg, (unsigned)B), dim3(kThreads), 0, stream, A, h, out);
}

void launch_boundary_load_add(hipStream_t stream, int nb, const int* rows, const double* load, double alpha, long long stride,
                              long long offset, double* y) {
  if (nb < 0 || stride < 1 || offset < 0 || offset >= stride) throw ArgError("boundary_load_add: bad stride or offset");
  if (nb == 0) return;
  const unsigned nwg = (unsigned)reduce::workgroups(nb);
  hipLaunchKernelGGL(boundary_load_add_kernel, dim3(nwg), dim3(kThreads), 0, stream, nb, rows, load, alpha, stride, offset, y);
}

void launch_boundary_flux(hipStream_t stream, int dim, int k, const Args& A, double* scratch, double* facet_flux) {
  if (A.E.n <= 0 || A.E.S <= 0 || A.E.B <= 0 || A.E.B > 65535) throw ArgError("boundary_flux: empty field, or more than 65535 fields");
  if (A.nf < 0 || A.q < 1 || A.q > kThreads) throw ArgError("boundary_flux: bad facet list");
  if (workgroups(A.nf, A.q) > 2147483647LL) throw ArgError("boundary_flux: too many facets");
  LaunchFlux l{stream, A, scratch, facet_flux};
  interp::dispatch(dim, k, l);
}

}  // namespace boundary
}  // namespace mgb
