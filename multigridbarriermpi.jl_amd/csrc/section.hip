// Plane sections of nodal fields on gfx950.  B fields x nc planes on one geometry are cut by ONE set of
// plain launches on one stream, the scheme of levelset.hip and isosurface.hip:
//   measure_kernel<DIM, K>: grid (workgroups(items), nc, B); one thread per item (a triangle in 2-D, one Kuhn tetrahedron of an
//     element's box in 3-D) runs section.hpp's item(): it classifies the corners against the plane first, so the large
//     majority of threads leave with the identity and read no field value; a cut item runs the quadrature on its one or two
//     pieces.  The workgroup reduces the five contributions and the number of emitted pieces (0, 1 or 2 per thread) and writes
//     ONE partial row and ONE count per (row, workgroup);
//   levelset::launch_finish: one workgroup per row folds the partials and scans the per-workgroup counts (levelset.hip).
// Where pieces are asked for, after the totals have reached the host:
//   emit_kernel<DIM, K>: the measure's grid; every thread recomputes its item; its rank in the workgroup is the exclusive
//     prefix sum of the 0..2 counts: two ballots (count >= 1, count == 2) popcounted over the lower lanes, the wave totals
//     through LDS behind one barrier.  Its first piece goes to slot row_base + offsets[workgroup] + rank, its second one to the
//     next slot: ascending item order, no atomics.
// What a row's result is made of depends on the items alone, never on B, nc or the row's place in the batch.
// This file is compiled with fp contraction off (build.sh): kernels and host restatement run item() with the same operations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

// Every function of the project's headers is inlined in this file, as in flowline.hip, so that this object file carries its
// OWN contraction-free copy of interp.hpp's bases: left out of line they are weak symbols, which the linker merges with the
// copies of the files compiled with contraction on, and the bits of this host restatement would depend on the link order.
// (The standard headers are included above, outside the pragma.)
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "section.hpp"
#pragma clang attribute pop

namespace mgb {
namespace section {
namespace {

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) measure_kernel(Args A, double* __restrict__ partials, long long* __restrict__ counts) {
  __shared__ double red[kWaves][kCols];
  __shared__ long long redc[kWaves][1];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const size_t row = (size_t)blockIdx.z * A.nc + blockIdx.y;
  Term<DIM> T;
  no_items(T.c);      // idle threads of the last workgroup stay for the reductions and contribute nothing
  T.emit = 0;
  if (i < A.items) item<DIM, K>(A, A.z[blockIdx.z], A.planes + (size_t)blockIdx.y * (DIM + 1), i, T);
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

template <int DIM, int K>
__global__ void __launch_bounds__(kThreads) emit_kernel(Args A, const long long* __restrict__ offsets,
                                                        const long long* __restrict__ row_base, long long total,
                                                        double* __restrict__ piece, int32_t* __restrict__ item_out) {
  constexpr int W = piece_width(DIM);
  __shared__ int wave_total[kWaves];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const size_t row = (size_t)blockIdx.z * A.nc + blockIdx.y;
  Term<DIM> T;
  T.emit = 0;
  if (i < A.items) item<DIM, K>(A, A.z[blockIdx.z], A.planes + (size_t)blockIdx.y * (DIM + 1), i, T);
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
      for (int k = 0; k < W; ++k) piece[(size_t)slot * W + k] = T.piece[0][k];
      item_out[slot] = (int32_t)i;
    }
    if (T.emit == 2 && slot + 1 < total) {
#pragma unroll
      for (int k = 0; k < W; ++k) piece[(size_t)(slot + 1) * W + k] = T.piece[1][k];
      item_out[slot + 1] = (int32_t)i;
    }
  }
}

// f.template operator()<DIM, K>() for the element kind
template <class F>
void dispatch(int dim, int k, F&& f) {
  if (dim == 2) f.template operator()<2, 0>();
  else if (k == 1) f.template operator()<3, 1>();
  else if (k == 2) f.template operator()<3, 2>();
  else f.template operator()<3, 3>();
}

struct Measure {
  hipStream_t stream;
  dim3 grid;
  const Args& A;
  double* scratch;
  long long* counts;
  template <int DIM, int K>
  void operator()() const {
    hipLaunchKernelGGL((measure_kernel<DIM, K>), grid, dim3(kThreads), 0, stream, A, scratch, counts);
  }
};

struct Emit {
  hipStream_t stream;
  dim3 grid;
  const Args& A;
  const long long *offsets, *row_base;
  long long total;
  double* piece;
  int32_t* item_out;
  template <int DIM, int K>
  void operator()() const {
    hipLaunchKernelGGL((emit_kernel<DIM, K>), grid, dim3(kThreads), 0, stream, A, offsets, row_base, total, piece, item_out);
  }
};

struct HostRows {
  const Args& A;
  double* out;
  long long *counts, *row_offsets;
  double* piece;
  int32_t* item_out;
  long long capacity;
  template <int DIM, int K>
  void operator()() const {
    constexpr int W = piece_width(DIM);
    long long at = 0;
    for (int b = 0; b < A.B; ++b)
      for (int l = 0; l < A.nc; ++l) {
        const size_t row = (size_t)b * A.nc + l;
        double* acc = out + row * kCols;
        no_items(acc);
        levelset::SerialSum sum[3];
        if (row_offsets) row_offsets[row] = at;
        long long cnt = 0;
        for (long long i = 0; i < A.items; ++i) {
          Term<DIM> T;
          item<DIM, K>(A, A.z[b], A.planes + (size_t)l * (DIM + 1), i, T);
          for (int k = 0; k < 3; ++k) sum[k].add(T.c[k]);
          acc[3] = nanmax(acc[3], T.c[3]);
          acc[4] = nanmax(acc[4], T.c[4]);
          for (int q = 0; q < T.emit; ++q) {
            if (piece) {
              if (at >= capacity) throw ArgError("sections_host: more pieces than the arrays hold");
              for (int k = 0; k < W; ++k) piece[(size_t)at * W + k] = T.piece[q][k];
              item_out[at] = (int32_t)i;
            }
            ++cnt;
            ++at;
          }
        }
        for (int k = 0; k < 3; ++k) acc[k] = sum[k].value();
        counts[row] = cnt;
      }
    if (row_offsets) row_offsets[(size_t)A.B * A.nc] = at;
  }
};

}  // namespace

void check(const std::string& who, const Args& A, int dim, int k) {
  if (dim != 2 && dim != 3)
    throw ArgError(who + ": a 2-D or 3-D geometry is needed; the value of a 1-D field at a point comes from interpolate");
  if (A.B < 1) throw ArgError(who + ": B must be >= 1");
  if (A.nc < 1) throw ArgError(who + ": nc must be >= 1");
  if (A.S < 1) throw ArgError(who + ": S must be >= 1");
  if (A.u < 0 || A.u >= A.S) throw ArgError(who + ": column u outside [0, S)");
  if (!(interp::finite(A.p) && A.p >= 1.0)) throw ArgError(who + ": p must be one finite real >= 1");
  if ((long long)A.B * A.nc > INT_MAX) throw ArgError(who + ": more than INT_MAX rows (fields x planes) per call");
  // Through the C ABI a geometry reaches this point only behind build_locator, which has refused every block other than 7 in
  // 2-D and (k+1)^3, k = 1..3, in 3-D with a message of its own: these two lines guard the kernels' indexing for any other caller.
  if (dim == 2 && A.own.block != 7) throw ArgError(who + ": 2-D elements must have 7 nodes");
  if (dim == 3 && (k < 1 || k > 3 || A.own.block != (k + 1) * (k + 1) * (k + 1)))
    throw ArgError(who + ": the elements must have (k+1)^3 nodes, k = 1..3");
  if (A.nel < 1) throw ArgError(who + ": a geometry without elements");
  if (A.items != items_per_row(dim, A.nel) || A.items > INT_MAX) throw ArgError(who + ": more than INT_MAX items per row");
}

void launch_measure(hipStream_t stream, int dim, int k, const Args& A, double* scratch, long long* counts) {
  check("sections", A, dim, k);
  if (A.B > 65535 || A.nc > 65535) throw ArgError("sections: at most 65535 fields and 65535 planes per call");
  const long long nwg = workgroups(A.items);
  const size_t rows = (size_t)A.B * A.nc;
  const dim3 grid((unsigned)nwg, (unsigned)A.nc, (unsigned)A.B);
  dispatch(dim, k, Measure{stream, grid, A, scratch, counts});
  double* results = scratch + levelset::results_offset(rows, (size_t)nwg);
  levelset::launch_finish(stream, (int)rows, scratch, counts, (int)nwg, results, counts + levelset::offsets_offset(rows, (size_t)nwg),
                          reinterpret_cast<long long*>(results + rows * kCols));
}

void launch_emit(hipStream_t stream, int dim, int k, const Args& A, const long long* offsets, const long long* row_base,
                 long long total, double* piece, int32_t* item_out) {
  check("sections", A, dim, k);
  const dim3 grid((unsigned)workgroups(A.items), (unsigned)A.nc, (unsigned)A.B);
  dispatch(dim, k, Emit{stream, grid, A, offsets, row_base, total, piece, item_out});
}

void sections_host(int dim, int k, const Args& A, double* out, long long* counts, long long* row_offsets, double* piece,
                   int32_t* item_out, long long capacity) {
  check("sections", A, dim, k);
  if ((piece == nullptr) != (item_out == nullptr)) throw ArgError("sections_host: piece and item come together");
  dispatch(dim, k, HostRows{A, out, counts, row_offsets, piece, item_out, capacity});
}

}  // namespace section
}  // namespace mgb
