// Isosurfaces of 3-D nodal fields on gfx950.  B fields x nl levels on one geometry are measured by ONE
// set of plain launches on one stream, the scheme of levelset.hip:
//   measure_kernel<K>: grid (workgroups(items), nl, B); one thread per item (one Kuhn tetrahedron of one lattice cell) runs
//     isosurface.hpp's item(); the workgroup reduces the five contributions and the number of emitted triangles (0, 1 or 2 per
//     thread) and writes ONE partial row and ONE count per (row, workgroup);
//   levelset::launch_finish: one workgroup per row folds the partials and scans the per-workgroup counts (levelset.hip).
// Where triangles are asked for, after the totals have reached the host:
//   emit_kernel<K>: the measure's grid; every thread recomputes its item; its rank in the workgroup is the exclusive prefix sum
//     of the 0..2 counts: two ballots (count >= 1, count == 2) popcounted over the lower lanes, the wave totals through LDS
//     behind one barrier.  Its first triangle goes to slot row_base + offsets[workgroup] + rank, its second one to the next
//     slot: ascending item order, no atomics.
// What a row's result is made of depends on the items alone, never on B, nl or the row's place in the batch.
// This file is compiled with fp contraction off (build.sh): kernels and host restatement run item() with the same operations.
#include "isosurface.hpp"

#include <climits>

namespace mgb {
namespace isosurface {
namespace {

template <int K>
__global__ void __launch_bounds__(kThreads) measure_kernel(Args A, double* __restrict__ partials, long long* __restrict__ counts) {
  __shared__ double red[kWaves][kCols];
  __shared__ long long redc[kWaves][1];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const size_t row = (size_t)blockIdx.z * A.nl + blockIdx.y;
  Term T;
  no_items(T.c);      // idle threads of the last workgroup stay for the reductions and contribute nothing
  T.emit = 0;
  if (i < A.items) item<K>(A, A.z[blockIdx.z], A.levels[blockIdx.y], i, T);
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

template <int K>
__global__ void __launch_bounds__(kThreads) emit_kernel(Args A, const long long* __restrict__ offsets,
                                                        const long long* __restrict__ row_base, long long total,
                                                        double* __restrict__ tri, int32_t* __restrict__ item_out) {
  __shared__ int wave_total[kWaves];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const size_t row = (size_t)blockIdx.z * A.nl + blockIdx.y;
  Term T;
  T.emit = 0;
  if (i < A.items) item<K>(A, A.z[blockIdx.z], A.levels[blockIdx.y], i, T);
  const unsigned long long some = __ballot(T.emit >= 1), two = __ballot(T.emit == 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  int rank = __popcll(some & lower) + __popcll(two & lower);
  if (lane == 0) wave_total[wave] = __popcll(some) + __popcll(two);
  __syncthreads();
  for (int w = 0; w < wave; ++w) rank += wave_total[w];
  if (T.emit >= 1) {
    const long long slot = row_base[row] + offsets[row * ((size_t)gridDim.x + 1) + blockIdx.x] + rank;
    if (slot < total) {
#pragma unroll
      for (int k = 0; k < kTriWidth; ++k) tri[(size_t)slot * kTriWidth + k] = T.tri[0][k];
      item_out[slot] = (int32_t)i;
    }
    if (T.emit == 2 && slot + 1 < total) {
#pragma unroll
      for (int k = 0; k < kTriWidth; ++k) tri[(size_t)(slot + 1) * kTriWidth + k] = T.tri[1][k];
      item_out[slot + 1] = (int32_t)i;
    }
  }
}

void check(const Args& A, int k) {
  if (k < 1 || k > 3) throw ArgError("isosurfaces: the elements must have (k+1)^3 nodes, k = 1..3");
  if (A.B < 1 || A.nl < 1 || A.S < 1 || A.nel < 1) throw ArgError("isosurfaces: empty batch, level list or field");
  if (A.u < 0 || A.u >= A.S) throw ArgError("isosurfaces: column u outside [0, S)");
  if (A.refine < 0 || A.refine > kMaxRefine) throw ArgError("isosurfaces: refine must be 0, 1 or 2");
  if (A.items != items_per_row(k, A.nel, A.refine) || A.items > INT_MAX) throw ArgError("isosurfaces: more than INT_MAX items per row");
}

}  // namespace

void launch_measure(hipStream_t stream, int k, const Args& A, double* scratch, long long* counts) {
  check(A, k);
  if (A.B > 65535 || A.nl > 65535) throw ArgError("isosurfaces: at most 65535 fields and 65535 levels per call");
  const long long nwg = workgroups(A.items);
  const size_t rows = (size_t)A.B * A.nl;
  if (rows > (size_t)INT_MAX) throw ArgError("isosurfaces: more than INT_MAX rows (fields x levels) per call");
  const dim3 grid((unsigned)nwg, (unsigned)A.nl, (unsigned)A.B);
  if (k == 1) hipLaunchKernelGGL(measure_kernel<1>, grid, dim3(kThreads), 0, stream, A, scratch, counts);
  else if (k == 2) hipLaunchKernelGGL(measure_kernel<2>, grid, dim3(kThreads), 0, stream, A, scratch, counts);
  else hipLaunchKernelGGL(measure_kernel<3>, grid, dim3(kThreads), 0, stream, A, scratch, counts);
  double* results = scratch + levelset::results_offset(rows, (size_t)nwg);
  levelset::launch_finish(stream, (int)rows, scratch, counts, (int)nwg, results, counts + levelset::offsets_offset(rows, (size_t)nwg),
                          reinterpret_cast<long long*>(results + rows * kCols));
}

void launch_emit(hipStream_t stream, int k, const Args& A, const long long* offsets, const long long* row_base, long long total,
                 double* tri, int32_t* item_out) {
  check(A, k);
  const dim3 grid((unsigned)workgroups(A.items), (unsigned)A.nl, (unsigned)A.B);
  if (k == 1) hipLaunchKernelGGL(emit_kernel<1>, grid, dim3(kThreads), 0, stream, A, offsets, row_base, total, tri, item_out);
  else if (k == 2) hipLaunchKernelGGL(emit_kernel<2>, grid, dim3(kThreads), 0, stream, A, offsets, row_base, total, tri, item_out);
  else hipLaunchKernelGGL(emit_kernel<3>, grid, dim3(kThreads), 0, stream, A, offsets, row_base, total, tri, item_out);
}

namespace {
template <int K>
void host_rows(const Args& A, double* out, long long* counts, long long* row_offsets, double* tri, int32_t* item_out,
               long long capacity) {
  long long at = 0;
  for (int b = 0; b < A.B; ++b)
    for (int l = 0; l < A.nl; ++l) {
      const size_t row = (size_t)b * A.nl + l;
      double* acc = out + row * kCols;
      no_items(acc);
      levelset::SerialSum sum[3];
      if (row_offsets) row_offsets[row] = at;
      long long cnt = 0;
      for (long long i = 0; i < A.items; ++i) {
        Term T;
        item<K>(A, A.z[b], A.levels[l], i, T);
        for (int k = 0; k < 3; ++k) sum[k].add(T.c[k]);
        acc[3] = nanmax(acc[3], T.c[3]);
        acc[4] = nanmax(acc[4], T.c[4]);
        for (int q = 0; q < T.emit; ++q) {
          if (tri) {
            if (at >= capacity) throw ArgError("isosurfaces_host: more triangles than the arrays hold");
            for (int k = 0; k < kTriWidth; ++k) tri[(size_t)at * kTriWidth + k] = T.tri[q][k];
            item_out[at] = (int32_t)i;
          }
          ++cnt;
          ++at;
        }
      }
      for (int k = 0; k < 3; ++k) acc[k] = sum[k].value();
      counts[row] = cnt;
    }
  if (row_offsets) row_offsets[(size_t)A.B * A.nl] = at;
}
}  // namespace

void isosurfaces_host(int k, const Args& A, double* out, long long* counts, long long* row_offsets, double* tri, int32_t* item_out,
                      long long capacity) {
  check(A, k);
  if ((tri == nullptr) != (item_out == nullptr)) throw ArgError("isosurfaces_host: tri and item come together");
  if (k == 1) host_rows<1>(A, out, counts, row_offsets, tri, item_out, capacity);
  else if (k == 2) host_rows<2>(A, out, counts, row_offsets, tri, item_out, capacity);
  else host_rows<3>(A, out, counts, row_offsets, tri, item_out, capacity);
}

}  // namespace isosurface
}  // namespace mgb
