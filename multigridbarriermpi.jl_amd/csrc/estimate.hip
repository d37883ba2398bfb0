// Residual error indicators on gfx950 (DESIGN.md sections 4j and 4m).  Behind the flux launch that wrote Sigma (energy.hip's
// flux_kernel), plain launches on one stream, 256 threads each, fp64, reduced by the two stages of reduce.hpp.  Every launch has
// the field in blockIdx.y: ONE field for mgb_estimate, the B steps of a parabolic run for mgb_estimate_steps, whose field b reads
// Sigma^(b+1), Sigma^b and the snapshots b + 1 and b (estimate.hpp's Terms::field).  What a field's numbers are made of does
// not depend on B or on its place in the batch.
//   facet_terms_kernel<DIM, K>: grid (workgroups, B); one thread per (facet, facet node); the interior facets come first, then
//     the boundary facets when there are Neumann data.  A workgroup takes 256 / q whole facets -- thread t is node t % q of the
//     workgroup's facet t / q, so the facet tables are read contiguously and a facet never straddles two workgroups.  Every
//     thread runs estimate.hpp's Terms::jump or Terms::neumann and leaves its term in LDS; node 0 of a facet adds its q terms in
//     ascending order and writes J[F] or N[F] (0 for a facet the mask leaves out).  The workgroup reduces |J_Fj| with the
//     NaN-sticky maximum and writes ONE partial maximum.  Left out when there is no facet at all.
//   element_indicator_kernel<DIM, K>: grid (workgroups, B); one thread per node, 256 / block whole elements per workgroup.
//     Every thread runs Terms::node (for a step behind Terms::quotient and Terms::step) and leaves w_i |rho_i|^r and w_i -- for a
//     step also its time term, its rate term and |d_i| -- in LDS; the first lane of an element adds them in ascending local
//     order, gathers J / N through the element -> facet table and leaves the element's three (four) numbers in LDS; the
//     workgroup's threads write them (nel x 3 or nel x 4, contiguous in the thread index) and thread 0 combines the elements'
//     columns in ascending element order into ONE partial row (two for a step).
//   estimate_finish: grid (B x rows); one workgroup finishes the element partials of one row of totals; for row 0 every thread
//     folds its run of the field's facet maxima into column 4 in front of the tree.
#include "estimate.hpp"

namespace mgb {
namespace estimate {
namespace {

constexpr int kMaxElems = kThreads / 2;      // elements per workgroup at the smallest block

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) facet_terms_kernel(Args A0, double* __restrict__ J, double* __restrict__ N,
                                                               double* __restrict__ partial_max) {
  __shared__ double per_node[kThreads];
  __shared__ double red[kWaves][1];
  const int b = blockIdx.y;
  const Args A = Terms<DIM, K>::field(A0, b);
  J += (size_t)b * A.nif;
  N += (size_t)b * A.nf;
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
  if (threadIdx.x == 0) partial_max[(size_t)b * gridDim.x + blockIdx.x] = aj;
}

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) element_indicator_kernel(Args A0, const double* __restrict__ J, const double* __restrict__ N,
                                                                     double* __restrict__ eta, double* __restrict__ partials) {
  __shared__ double term[kThreads];
  __shared__ double wts[kThreads];
  __shared__ double tims[kThreads];      // the three step-only values of a node: written and read for a step alone
  __shared__ double rates[kThreads];
  __shared__ double dabs[kThreads];
  __shared__ double parts[kMaxElems * kStepParts];
  __shared__ double srow[kMaxElems * 2];      // rate sum and largest |d_i| of an element of a step
  const int b = blockIdx.y;
  const Args A = Terms<DIM, K>::field(A0, b);
  const bool steps = A.steps;
  const int np = steps ? kStepParts : kParts;
  J += (size_t)b * A.nif;
  if (N) N += (size_t)b * A.nf;
  eta += (size_t)b * A.nel * np;
  const int block = A.own.block, epw = kThreads / block;
  const int le = threadIdx.x / block, li = threadIdx.x - le * block;
  const long long e0 = (long long)blockIdx.x * epw;
  const long long e = e0 + le;
  const bool mine = le < epw && e < A.nel;      // idle threads stay for the barriers and contribute nothing
  double t = 0.0, wi = 0.0;
  if (mine) {
    const int i = (int)(e * block + li);
    double d = 0.0;
    if (steps) {
      double tm, rt, ad;
      d = Terms<DIM, K>::quotient(A, i);
      Terms<DIM, K>::step(A, i, d, tm, rt, ad);
      tims[threadIdx.x] = tm;
      rates[threadIdx.x] = rt;
      dabs[threadIdx.x] = ad;
    }
    t = Terms<DIM, K>::node(A, i, d);
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
    Terms<DIM, K>::element(A, (int)e, ts, ws, J, N, parts + le * np);
    if (steps) {
      double tim = 0.0, rate = 0.0, dmax = 0.0;
      for (int k = 0; k < block; ++k) {
        tim += tims[threadIdx.x + k];
        rate += rates[threadIdx.x + k];
        dmax = nanmax(dmax, dabs[threadIdx.x + k]);
      }
      parts[le * np + 3] = tim;
      srow[le * 2] = rate;
      srow[le * 2 + 1] = dmax;
    }
  }
  __syncthreads();
  const long long left = A.nel - e0;
  const int here = left < epw ? (int)left : epw;      // elements of this workgroup
  for (int k = threadIdx.x; k < here * np; k += kThreads) eta[(size_t)e0 * np + k] = parts[k];
  if (threadIdx.x == 0) {
    double acc[kCols], acc1[kCols];
    identity(acc);
    identity(acc1);
    for (int k = 0; k < here; ++k) {
      double c[kCols];
      element_columns(parts + k * np, c);
      combine(acc, c);
      if (steps) {
        step_columns(parts[k * np + 3], srow[k * 2], srow[k * 2 + 1], c);
        combine(acc1, c);
      }
    }
    // the partial rows of field b: row 0, then row 1 of a step, gridDim.x workgroups each
    double* row = partials + ((size_t)b * (steps ? 2 : 1) * gridDim.x + blockIdx.x) * kCols;
#pragma unroll
    for (int k = 0; k < kCols; ++k) row[k] = acc[k];
    if (steps) {
      row += (size_t)gridDim.x * kCols;
#pragma unroll
      for (int k = 0; k < kCols; ++k) row[k] = acc1[k];
    }
  }
}

// workgroup blockIdx.x finishes row blockIdx.x % rows of field blockIdx.x / rows
__global__ void __launch_bounds__(kThreads) estimate_finish(const double* __restrict__ partials, int nwg,
                                                            const double* __restrict__ partial_max, int nwgf, int rows,
                                                            double* __restrict__ out) {
  __shared__ double red[kWaves][kCols];
  // empty runs carry reduce::identity, -inf in column 4, where the partials hold zeros: the maxima are absolute values and
  // thread 0 always holds an element partial, so either seed gives the same bits
  double c[kCols];
  run_combine(partials + (size_t)blockIdx.x * nwg * kCols, kCols, nwg, c);
  if (blockIdx.x % rows == 0) {      // uniform in the workgroup
    const double* pm = partial_max + (size_t)(blockIdx.x / rows) * nwgf;
    const Run r = run_of(threadIdx.x, nwgf);
    for (long long g = r.b0; g < r.b1; ++g) c[4] = nanmax(c[4], pm[g]);
  }
  block_reduce<kCols>(c, Combine{}, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < kCols; ++k) out[(size_t)blockIdx.x * kCols + k] = c[k];
  }
}

struct Launch {
  hipStream_t stream;
  Args A;
  double *J, *N, *eta, *scratch;
  template <int DIM, int K>
  void operator()() const {
    const long long nwge = element_workgroups(A.nel, A.own.block), nwgf = facet_workgroups(facets_launched(A), A.q);
    const int R = rows_of(A);
    double* partials = scratch;
    double* partial_max = scratch + (size_t)A.B * R * nwge * kCols;
    double* out = scratch + results_offset(A.nel, A.own.block, facets_launched(A), A.q, A.B, R);
    if (nwgf > 0)
      hipLaunchKernelGGL((facet_terms_kernel<DIM, K>), dim3((unsigned)nwgf, (unsigned)A.B), dim3(kThreads), 0, stream, A, J, N,
                         partial_max);
    hipLaunchKernelGGL((element_indicator_kernel<DIM, K>), dim3((unsigned)nwge, (unsigned)A.B), dim3(kThreads), 0, stream, A, J,
                       A.h ? N : nullptr, eta, partials);
    hipLaunchKernelGGL(estimate_finish, dim3((unsigned)(A.B * R)), dim3(kThreads), 0, stream, partials, (int)nwge, partial_max,
                       (int)nwgf, R, out);
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
  if (A.B < 1 || A.B > 65535) throw ArgError("estimate: between 1 and 65535 fields per call");
  if (A.steps && (!A.z || !A.dt || A.S < 1 || A.u < 0 || A.u >= A.S)) throw ArgError("estimate: a step needs its snapshots and its step size");
  if (!A.steps && A.B != 1) throw ArgError("estimate: several fields are the steps of a parabolic run");
  Launch l{stream, A, J, N, eta, scratch};
  interp::dispatch(dim, k, l);
}

}  // namespace estimate
}  // namespace mgb
