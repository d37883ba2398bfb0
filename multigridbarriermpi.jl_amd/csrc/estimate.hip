// Residual error indicators on gfx950.  Behind the flux launch that wrote Sigma (energy.hip's
// flux_kernel), plain launches on one stream, 256 threads each, fp64, reduced by the two stages of reduce.hpp:
//   facet_terms_kernel<DIM, K>: one thread per (facet, facet node); the interior facets come first, then the boundary facets
//     when there are Neumann data.  A workgroup takes 256 / q whole facets -- thread t is node t % q of the workgroup's facet
//     t / q, so the facet tables are read contiguously and a facet never straddles two workgroups.  Every thread runs
//     estimate.hpp's Terms::jump or Terms::neumann and leaves its term in LDS; node 0 of a facet adds its q terms in ascending
//     order and writes J[F] or N[F] (0 for a facet the mask leaves out).  The workgroup reduces |J_Fj| with the NaN-sticky
//     maximum and writes ONE partial maximum.  Left out when there is no facet at all.
//   element_indicator_kernel<DIM, K>: one thread per node, 256 / block whole elements per workgroup.  Every thread runs
//     Terms::node and leaves w_i |rho_i|^r and w_i in LDS; the first lane of an element adds both in ascending local order,
//     gathers J / N through the element -> facet table and leaves the element's three numbers in LDS; the workgroup's threads
//     write them (nel x 3, contiguous in the thread index) and thread 0 combines the elements' columns in ascending element
//     order into ONE partial row.
//   estimate_finish: one workgroup finishes the element partials; every thread folds its run of the facet maxima into column
//     4 in front of the tree.
#include "estimate.hpp"

namespace mgb {
namespace estimate {
namespace {

constexpr int kMaxElems = kThreads / 2;      // elements per workgroup at the smallest block

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) facet_terms_kernel(Args A, double* __restrict__ J, double* __restrict__ N,
                                                               double* __restrict__ partial_max) {
  __shared__ double per_node[kThreads];
  __shared__ double red[kWaves][1];
  const int q = A.q, fpw = kThreads / q;
  const int lf = threadIdx.x / q, j = threadIdx.x - lf * q;
  const long long F = (long long)blockIdx.x * fpw + lf;
  const long long total = (long long)A.nif + (A.h ? A.nf : 0);
  const bool mine = lf < fpw && F < total;      // idle threads stay for the barriers and contribute nothing
  const bool interior = F < A.nif;
  double term = 0.0, aj = 0.0;
  if (mine) {
    if (interior) {
      term = Terms<DIM, K>::jump(A, (int)F, j, aj);
    } else {
      const int fb = (int)(F - A.nif);
      if (!A.mask || A.mask[fb]) term = Terms<DIM, K>::neumann(A, fb, j);
    }
  }
  per_node[threadIdx.x] = term;
  __syncthreads();
  if (mine && j == 0) {
    double s = 0.0;
    for (int t = 0; t < q; ++t) s += per_node[threadIdx.x + t];
    if (interior) J[F] = s;
    else N[F - A.nif] = s;
  }
  block_reduce<1>(&aj, NanMax<1>{}, red);
  if (threadIdx.x == 0) partial_max[blockIdx.x] = aj;
}

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) element_indicator_kernel(Args A, const double* __restrict__ J, const double* __restrict__ N,
                                                                     double* __restrict__ eta, double* __restrict__ partials) {
  __shared__ double term[kThreads];
  __shared__ double wts[kThreads];
  __shared__ double parts[kMaxElems * kParts];
  const int block = A.own.block, epw = kThreads / block;
  const int le = threadIdx.x / block, li = threadIdx.x - le * block;
  const long long e0 = (long long)blockIdx.x * epw;
  const long long e = e0 + le;
  const bool mine = le < epw && e < A.nel;      // idle threads stay for the barriers and contribute nothing
  double t = 0.0, wi = 0.0;
  if (mine) {
    const int i = (int)(e * block + li);
    t = Terms<DIM, K>::node(A, i);
    wi = A.w[i];
  }
  term[threadIdx.x] = t;
  wts[threadIdx.x] = wi;
  __syncthreads();
  if (mine && li == 0) {
    double ts = 0.0, ws = 0.0;
    for (int k = 0; k < block; ++k) {
      ts += term[threadIdx.x + k];
      ws += wts[threadIdx.x + k];
    }
    Terms<DIM, K>::element(A, (int)e, ts, ws, J, N, parts + le * kParts);
  }
  __syncthreads();
  const long long left = A.nel - e0;
  const int here = left < epw ? (int)left : epw;      // elements of this workgroup
  for (int k = threadIdx.x; k < here * kParts; k += kThreads) eta[(size_t)e0 * kParts + k] = parts[k];
  if (threadIdx.x == 0) {
    double acc[kCols];
    identity(acc);
    for (int k = 0; k < here; ++k) {
      double c[kCols];
      element_columns(parts + k * kParts, c);
      combine(acc, c);
    }
    double* row = partials + (size_t)blockIdx.x * kCols;
#pragma unroll
    for (int k = 0; k < kCols; ++k) row[k] = acc[k];
  }
}

__global__ void __launch_bounds__(kThreads) estimate_finish(const double* __restrict__ partials, int nwg,
                                                            const double* __restrict__ partial_max, int nwgf, double* __restrict__ out) {
  __shared__ double red[kWaves][kCols];
  // empty runs carry reduce::identity, -inf in column 4, where the partials hold zeros: the maxima are absolute values and
  // thread 0 always holds an element partial, so either seed gives the same bits
  double c[kCols];
  run_combine(partials, kCols, nwg, c);
  const Run r = run_of(threadIdx.x, nwgf);
  for (long long g = r.b0; g < r.b1; ++g) c[4] = nanmax(c[4], partial_max[g]);
  block_reduce<kCols>(c, Combine{}, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kCols; ++k) out[k] = c[k];
  }
}

struct Launch {
  hipStream_t stream;
  Args A;
  double *J, *N, *eta, *scratch;
  template <int DIM, int K>
  void operator()() const {
    const long long nwge = element_workgroups(A.nel, A.own.block), nwgf = facet_workgroups(facets_launched(A), A.q);
    double* partials = scratch;
    double* partial_max = scratch + (size_t)nwge * kCols;
    double* out = scratch + results_offset(A.nel, A.own.block, facets_launched(A), A.q);
    if (nwgf > 0)
      hipLaunchKernelGGL((facet_terms_kernel<DIM, K>), dim3((unsigned)nwgf), dim3(kThreads), 0, stream, A, J, N, partial_max);
    hipLaunchKernelGGL((element_indicator_kernel<DIM, K>), dim3((unsigned)nwge), dim3(kThreads), 0, stream, A, J, A.h ? N : nullptr,
                       eta, partials);
    hipLaunchKernelGGL(estimate_finish, dim3(1), dim3(kThreads), 0, stream, partials, (int)nwge, partial_max, (int)nwgf, out);
  }
};

}  // namespace

void launch_estimate(hipStream_t stream, int dim, int k, const Args& A, double* J, double* N, double* eta, double* scratch) {
  if (A.n <= 0 || A.nel <= 0 || A.own.block < 1 || A.own.block > kThreads || (long long)A.nel * A.own.block != A.n)
    throw ArgError("estimate: empty field or bad element size");
  if (A.nif < 0 || A.nf < 0 || A.q < 1 || A.q > kThreads || A.nlf < 1) throw ArgError("estimate: bad facet lists");
  if (kThreads / A.own.block > kMaxElems) throw ArgError("estimate: elements of fewer than 2 nodes");
  if (element_workgroups(A.nel, A.own.block) > 2147483647LL || facet_workgroups(facets_launched(A), A.q) > 2147483647LL)
    throw ArgError("estimate: too many elements or facets");
  Launch l{stream, A, J, N, eta, scratch};
  interp::dispatch(dim, k, l);
}

}  // namespace estimate
}  // namespace mgb
