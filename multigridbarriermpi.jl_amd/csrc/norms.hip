// Norms and errors of nodal fields on gfx950.  The two launches of reduce.hpp on one stream:
//   norms_kernel<DIM, K>: one thread per node runs norms.hpp's Node (own basis once, the other mesh's element by the nudged
//     point, then the S columns); per column the workgroup reduces the five contributions and writes ONE partial row per
//     (workgroup, column), and one count of outside nodes per workgroup;
//   norms_finish: grid (S); the workgroup of a column finishes that column, the first one the count of outside nodes as well.
#include "norms.hpp"

namespace mgb {
namespace norms {
namespace {

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) norms_kernel(Args A, double* __restrict__ partials, long long* __restrict__ counts) {
  __shared__ double red[2][kWaves][kCols];
  __shared__ long long redc[kWaves][1];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool active = i < A.n;      // idle threads of the last workgroup stay for the reductions and contribute nothing
  Node<DIM, K> N;
  if (active) N.init(A, (int)i);
  long long cnt = active && N.outside ? 1 : 0;
  block_reduce<1>(&cnt, Count{}, redc);
  if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
  for (int s = 0; s < A.S; ++s) {
    double c[kCols] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (active) N.column(A, s, c);
    block_reduce<kCols>(c, Combine{}, red[s & 1]);
    if (threadIdx.x == 0) {
      double* row = partials + ((size_t)blockIdx.x * A.S + s) * kCols;
#pragma unroll
      for (int k = 0; k < kCols; ++k) row[k] = c[k];
    }
  }
}

__global__ void __launch_bounds__(kThreads) norms_finish(const double* __restrict__ partials, const long long* __restrict__ counts,
                                                         int nwg, int S, double* __restrict__ out, long long* __restrict__ outside) {
  __shared__ double red[kWaves][kCols];
  __shared__ long long redc[kWaves][1];
  const int s = blockIdx.x;
  if (s == 0) {      // uniform over the workgroup
    const Run r = run_of(threadIdx.x, nwg);
    long long cnt = 0;
    for (long long b = r.b0; b < r.b1; ++b) cnt += counts[b];
    block_reduce<1>(&cnt, Count{}, redc);
    if (threadIdx.x == 0) *outside = cnt;
  }
  // empty runs carry reduce::identity, -inf in column 4, where norms_kernel seeds zeros: both maxima are absolute values and
  // thread 0 always holds a partial (n >= 1), so either seed gives the same bits
  finish_row(partials + (size_t)s * kCols, (size_t)S * kCols, nwg, red, out + (size_t)s * kCols);
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
    hipLaunchKernelGGL(norms_finish, dim3((unsigned)A.S), dim3(kThreads), 0, stream, scratch, counts, (int)nwg, A.S,
                       scratch + results_offset(A.n, A.S), counts + count_offset(A.n));
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
