// Residual error indicators on gfx950.  Behind the flux launch that wrote Sigma (energy.hip's
// flux_kernel), plain launches on one stream, 256 threads each, fp64:
//   facet_terms_kernel<DIM, K>: one thread per (facet, facet node); the interior facets come first, then the boundary facets
//     when there are Neumann data.  A workgroup takes 256 / q whole facets -- thread t is node t % q of the workgroup's facet
//     t / q, so the facet tables are read contiguously and a facet never straddles two workgroups.  Every thread runs
//     estimate.hpp's Terms::jump or Terms::neumann and leaves its term in LDS; node 0 of a facet adds its q terms in ascending
//     order and writes J[F] or N[F] (0 for a facet the mask leaves out).  The workgroup reduces |J_Fj| with the NaN-sticky
//     maximum -- wave shuffles, then LDS across the four waves -- and writes ONE partial maximum.  Left out when there is no
//     facet at all.
//   element_indicator_kernel<DIM, K>: one thread per node, 256 / block whole elements per workgroup.  Every thread runs
//     Terms::node and leaves w_i |rho_i|^r and w_i in LDS; the first lane of an element adds both in ascending local order,
//     gathers J / N through the element -> facet table and leaves the element's three numbers in LDS; the workgroup's threads
//     write them (nel x 3, contiguous in the thread index) and thread 0 combines the elements' columns in ascending element
//     order into ONE partial row.
//   estimate_finish: one workgroup combines the element partials and the facet maxima in ascending workgroup order (thread t
//     takes the t-th contiguous run, then the tree of energy.hip).
// No atomics and no hand-off between workgroups inside a launch; no thread returns in front of a barrier -- threads past the
// end idle through them; every word is written by one thread with a vector store.
#include "estimate.hpp"

namespace mgb {
namespace estimate {
namespace {

static_assert(kThreads == 256, "four waves of 64");
constexpr int kWaves = kThreads / 64;
constexpr int kMaxElems = kThreads / 2;      // elements per workgroup at the smallest block

// NaN-sticky maximum of v over the workgroup; the result is valid in thread 0
__device__ inline double block_nanmax(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kWaves; ++k) v = nanmax(v, red[k]);
  }
  return v;
}

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
__global__ void __launch_bounds__(kThreads) facet_terms_kernel(Args A, double* __restrict__ J, double* __restrict__ N,
                                                               double* __restrict__ partial_max) {
  __shared__ double per_node[kThreads];
  __shared__ double red[kWaves];
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
  const double m = block_nanmax(aj, red);
  if (threadIdx.x == 0) partial_max[blockIdx.x] = m;
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
  double c[kCols];
  identity(c);
  {
    const int chunk = (nwg + kThreads - 1) / kThreads;
    const long long b0 = (long long)threadIdx.x * chunk;
    const long long b1 = b0 + chunk < nwg ? b0 + chunk : nwg;
    for (long long g = b0; g < b1; ++g) combine(c, partials + (size_t)g * kCols);
  }
  {
    const int chunk = (nwgf + kThreads - 1) / kThreads;
    const long long b0 = (long long)threadIdx.x * chunk;
    const long long b1 = b0 + chunk < nwgf ? b0 + chunk : nwgf;
    for (long long g = b0; g < b1; ++g) c[4] = nanmax(c[4], partial_max[g]);
  }
  block_combine(c, red);
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
    double* out = partial_max + nwgf;
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
