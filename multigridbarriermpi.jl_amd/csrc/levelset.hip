// Level sets of nodal fields on gfx950.  B fields x nl levels on one geometry are measured by ONE set
// of plain launches on one stream:
//   measure_kernel<DIM>: grid (workgroups(items), nl, B); one thread per item runs levelset.hpp's item(); the workgroup reduces
//     the five contributions and the number of emitted segments and writes ONE partial row and ONE count per (row, workgroup);
//   finish_kernel (behind launch_finish, which isosurface.hip calls too): grid (B nl); the workgroup of a row folds that
//     row's partials into its 5 doubles with reduce.hpp's finish_row, started from the identity of these rows (both maxima may be negative), and turns the row's nwg counts
//     into nwg + 1 exclusive offsets, the total last.
// Where segments are asked for, after the totals have reached the host:
//   emit_kernel<DIM>: the measure's grid; every thread recomputes its item, ranks itself among the emitting threads of its
//     workgroup (__ballot and __popcll of the lower lanes, the wave totals through LDS with one barrier) and writes its segment
//     and item index to slot row_base + offsets[workgroup] + rank: ascending item order, no atomics.
// What a row's result is made of depends on the items alone, never on B, nl or the row's place in the batch.
// This file is compiled with fp contraction off (build.sh): kernels and host restatement run item() with the same operations.
#include "levelset.hpp"

#include <climits>

namespace mgb {
namespace levelset {
namespace {

template <int DIM>
__global__ void __launch_bounds__(kThreads) measure_kernel(Args A, double* __restrict__ partials, long long* __restrict__ counts) {
  __shared__ double red[kWaves][kCols];
  __shared__ long long redc[kWaves][1];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const size_t row = (size_t)blockIdx.z * A.nl + blockIdx.y;
  Term T;
  no_items(T.c);      // idle threads of the last workgroup stay for the reductions and contribute nothing
  T.emit = 0;
  if (i < A.items) item<DIM>(A, A.z[blockIdx.z], A.levels[blockIdx.y], i, T);
  long long cnt = T.emit;
  reduce::block_reduce<kCols>(T.c, reduce::Combine{}, red);
  reduce::block_reduce<1>(&cnt, reduce::Count{}, redc);
  if (threadIdx.x == 0) {
    double* out = partials + (row * gridDim.x + blockIdx.x) * kCols;
#pragma unroll
    for (int k = 0; k < kCols; ++k) out[k] = T.c[k];
    counts[row * gridDim.x + blockIdx.x] = cnt;
  }
}

// One workgroup per row finishes the row: reduce.hpp's finish_row folds the nwg partial rows into the row's 5 doubles, started
// from the identity of THESE rows; the nwg counts become nwg + 1 exclusive offsets, the total last (thread t sums its run_of
// chunk, the workgroup scans the 256 chunk totals, thread t writes its offsets).
__global__ void __launch_bounds__(kThreads) finish_kernel(const double* __restrict__ partials, const long long* __restrict__ counts,
                                                          int nwg, double* __restrict__ results, long long* __restrict__ offsets,
                                                          long long* __restrict__ totals) {
  __shared__ double red[kWaves][kCols];
  __shared__ long long wave_total[kWaves];
  reduce::finish_row(partials + (size_t)blockIdx.x * nwg * kCols, kCols, nwg, red, results + (size_t)blockIdx.x * kCols, NoItems{});
  const long long* c = counts + (size_t)blockIdx.x * nwg;
  long long* o = offsets + (size_t)blockIdx.x * ((size_t)nwg + 1);
  const reduce::Run r = reduce::run_of(threadIdx.x, nwg);
  long long mine = 0;
  for (long long g = r.b0; g < r.b1; ++g) mine += c[g];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = mine;      // inclusive scan over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long t = __shfl_up(inc, d, 64);
    inc += lane >= d ? t : 0;
  }
  if (lane == 63) wave_total[wave] = inc;
  __syncthreads();
  long long at = inc - mine;
  for (int w = 0; w < wave; ++w) at += wave_total[w];
  for (long long g = r.b0; g < r.b1; ++g) {
    o[g] = at;
    at += c[g];
  }
  if (threadIdx.x == kThreads - 1) {      // its run is the last one, or empty behind the last one: `at` is the row's total
    o[nwg] = at;
    totals[blockIdx.x] = at;
  }
}

template <int DIM>
__global__ void __launch_bounds__(kThreads) emit_kernel(Args A, const long long* __restrict__ offsets,
                                                        const long long* __restrict__ row_base, long long total,
                                                        double* __restrict__ seg, int32_t* __restrict__ item_out) {
  __shared__ int wave_total[kWaves];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const size_t row = (size_t)blockIdx.z * A.nl + blockIdx.y;
  Term T;
  T.emit = 0;
  if (i < A.items) item<DIM>(A, A.z[blockIdx.z], A.levels[blockIdx.y], i, T);
  const unsigned long long mask = __ballot(T.emit);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int rank = __popcll(mask & ((1ull << lane) - 1ull));
  if (lane == 0) wave_total[wave] = __popcll(mask);
  __syncthreads();
  for (int w = 0; w < wave; ++w) rank += wave_total[w];
  if (T.emit) {
    const long long slot = row_base[row] + offsets[row * ((size_t)gridDim.x + 1) + blockIdx.x] + rank;
    if (slot < total) {
      constexpr int W = DIM == 2 ? 4 : 2;
#pragma unroll
      for (int k = 0; k < W; ++k) seg[(size_t)slot * W + k] = T.seg[k];
      item_out[slot] = (int32_t)i;
    }
  }
}

void check(const Args& A, int dim) {
  if (dim != 1 && dim != 2) throw ArgError("level_sets: isosurfaces of 3-D fields are not covered");
  if (A.B < 1 || A.nl < 1 || A.S < 1 || A.nel < 1) throw ArgError("level_sets: empty batch, level list or field");
  if (A.u < 0 || A.u >= A.S) throw ArgError("level_sets: column u outside [0, S)");
  if (A.refine < 0 || A.refine > (dim == 2 ? kMaxRefine : 0)) throw ArgError("level_sets: refine must be 0..3 (1-D: 0)");
  if (A.items != items_per_row(dim, A.nel, A.refine) || A.items > INT_MAX) throw ArgError("level_sets: more than INT_MAX items per row");
}

}  // namespace

void launch_measure(hipStream_t stream, int dim, const Args& A, double* scratch, long long* counts) {
  check(A, dim);
  if (A.B > 65535 || A.nl > 65535) throw ArgError("level_sets: at most 65535 fields and 65535 levels per call");
  const long long nwg = workgroups(A.items);
  const size_t rows = (size_t)A.B * A.nl;
  if (rows > (size_t)INT_MAX) throw ArgError("level_sets: more than INT_MAX rows (fields x levels) per call");
  const dim3 grid((unsigned)nwg, (unsigned)A.nl, (unsigned)A.B);
  if (dim == 2) hipLaunchKernelGGL(measure_kernel<2>, grid, dim3(kThreads), 0, stream, A, scratch, counts);
  else hipLaunchKernelGGL(measure_kernel<1>, grid, dim3(kThreads), 0, stream, A, scratch, counts);
  double* results = scratch + results_offset(rows, (size_t)nwg);
  launch_finish(stream, (int)rows, scratch, counts, (int)nwg, results, counts + offsets_offset(rows, (size_t)nwg),
                reinterpret_cast<long long*>(results + rows * kCols));
}

void launch_finish(hipStream_t stream, int rows, const double* partials, const long long* counts, int nwg, double* results,
                   long long* offsets, long long* totals) {
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)rows), dim3(kThreads), 0, stream, partials, counts, nwg, results, offsets, totals);
}

void launch_emit(hipStream_t stream, int dim, const Args& A, const long long* offsets, const long long* row_base, long long total,
                 double* seg, int32_t* item_out) {
  check(A, dim);
  const dim3 grid((unsigned)workgroups(A.items), (unsigned)A.nl, (unsigned)A.B);
  if (dim == 2) hipLaunchKernelGGL(emit_kernel<2>, grid, dim3(kThreads), 0, stream, A, offsets, row_base, total, seg, item_out);
  else hipLaunchKernelGGL(emit_kernel<1>, grid, dim3(kThreads), 0, stream, A, offsets, row_base, total, seg, item_out);
}

namespace {
template <int DIM>
void host_rows(const Args& A, double* out, long long* counts, long long* row_offsets, double* seg, int32_t* item_out,
               long long capacity) {
  constexpr int W = DIM == 2 ? 4 : 2;
  long long at = 0;
  for (int b = 0; b < A.B; ++b)
    for (int l = 0; l < A.nl; ++l) {
      const size_t row = (size_t)b * A.nl + l;
      double* acc = out + row * kCols;
      no_items(acc);
      SerialSum sum[3];
      if (row_offsets) row_offsets[row] = at;
      long long cnt = 0;
      for (long long i = 0; i < A.items; ++i) {
        Term T;
        item<DIM>(A, A.z[b], A.levels[l], i, T);
        for (int k = 0; k < 3; ++k) sum[k].add(T.c[k]);
        acc[3] = nanmax(acc[3], T.c[3]);
        acc[4] = nanmax(acc[4], T.c[4]);
        if (!T.emit) continue;
        if (seg) {
          if (at >= capacity) throw ArgError("level_sets_host: more segments than the arrays hold");
          for (int k = 0; k < W; ++k) seg[(size_t)at * W + k] = T.seg[k];
          item_out[at] = (int32_t)i;
        }
        ++cnt;
        ++at;
      }
      for (int k = 0; k < 3; ++k) acc[k] = sum[k].value();
      counts[row] = cnt;
    }
  if (row_offsets) row_offsets[(size_t)A.B * A.nl] = at;
}
}  // namespace

void level_sets_host(int dim, const Args& A, double* out, long long* counts, long long* row_offsets, double* seg, int32_t* item_out,
                     long long capacity) {
  check(A, dim);
  if ((seg == nullptr) != (item_out == nullptr)) throw ArgError("level_sets_host: seg and item come together");
  if (dim == 2) host_rows<2>(A, out, counts, row_offsets, seg, item_out, capacity);
  else host_rows<1>(A, out, counts, row_offsets, seg, item_out, capacity);
}

}  // namespace levelset
}  // namespace mgb
