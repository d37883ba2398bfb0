// Norms and errors of nodal fields on gfx950.  Two plain launches on one stream:
//   norms_kernel<DIM, K>: one thread per node runs norms.hpp's Node (own basis once, the other mesh's element by the nudged
//     point, then the S columns); per column the workgroup reduces the five contributions -- wave shuffles, then LDS across
//     the four waves, the three sums and the two maxima together -- and writes ONE partial row per (workgroup, column);
//   norms_finish: one workgroup combines the partials in ascending workgroup order (thread t takes the t-th contiguous run
//     of workgroups, then the same tree) and writes S x 5 doubles and the count of outside nodes.
// No atomics and no hand-off between workgroups inside a launch: every word is written by one thread, every sum has a fixed
// order, so the result is bitwise reproducible from run to run, and the second launch cannot wait on the first.
#include "norms.hpp"

namespace mgb {
namespace norms {
namespace {

static_assert(kThreads == 256, "four waves of 64");
constexpr int kWaves = kThreads / 64;

// Reduce c[0..4] (sums 0..2, NaN-sticky maxima 3..4) over the workgroup; the result is valid in thread 0.  `red` is one of
// two alternating LDS buffers: a caller that alternates them needs no second barrier between consecutive reductions.
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

__device__ inline long long block_count(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kWaves; ++k) v += red[k];
  }
  return v;
}

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) norms_kernel(Args A, double* __restrict__ partials, long long* __restrict__ counts) {
  __shared__ double red[2][kWaves][kCols];
  __shared__ long long redc[kWaves];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool active = i < A.n;      // idle threads of the last workgroup stay for the reductions and contribute nothing
  Node<DIM, K> N;
  if (active) N.init(A, (int)i);
  const long long cnt = block_count(active && N.outside ? 1 : 0, redc);
  if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
  for (int s = 0; s < A.S; ++s) {
    double c[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (active) N.column(A, s, c);
    block_combine(c, red[s & 1]);
    if (threadIdx.x == 0) {
      double* row = partials + ((size_t)blockIdx.x * A.S + s) * kCols;
#pragma unroll
      for (int k = 0; k < kCols; ++k) row[k] = c[k];
    }
  }
}

__global__ void __launch_bounds__(kThreads) norms_finish(const double* __restrict__ partials, const long long* __restrict__ counts,
                                                         int nwg, int S, double* __restrict__ out, long long* __restrict__ outside) {
  __shared__ double red[2][kWaves][kCols];
  __shared__ long long redc[kWaves];
  const int chunk = (nwg + kThreads - 1) / kThreads;
  const long long b0 = (long long)threadIdx.x * chunk;
  const long long b1 = b0 + chunk < nwg ? b0 + chunk : nwg;
  long long cnt = 0;
  for (long long b = b0; b < b1; ++b) cnt += counts[b];
  cnt = block_count(cnt, redc);
  if (threadIdx.x == 0) *outside = cnt;
  for (int s = 0; s < S; ++s) {
    double c[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long b = b0; b < b1; ++b) combine(c, partials + ((size_t)b * S + s) * kCols);
    block_combine(c, red[s & 1]);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kCols; ++k) out[(size_t)s * kCols + k] = c[k];
    }
  }
}

struct Launch {
  hipStream_t stream;
  Args A;
  double* scratch;
  long long* counts;
  template <int DIM, int K>
  void operator()() const {
    const long long nwg = workgroups(A.n);
    hipLaunchKernelGGL((norms_kernel<DIM, K>), dim3((unsigned)nwg), dim3(kThreads), 0, stream, A, scratch, counts);
    hipLaunchKernelGGL(norms_finish, dim3(1), dim3(kThreads), 0, stream, scratch, counts, (int)nwg, A.S,
                       scratch + (size_t)nwg * A.S * kCols, counts + nwg);
  }
};

}  // namespace

void launch_field_norms(hipStream_t stream, int dim, int k, const Args& A, double* scratch, long long* counts) {
  if (A.n <= 0 || A.S <= 0) throw ArgError("field_norms: empty field");
  Launch l{stream, A, scratch, counts};
  interp::dispatch(dim, k, l);
}

}  // namespace norms
}  // namespace mgb
