// Norms and errors of nodal fields by the nodal quadrature rule: what ONE node contributes, written
// ONCE.  The gfx950 kernel (norms.hip) and the host restatement (mgb_geo_field_norms_host) both run Node below; the element
// maths (inverse maps, bases, locator) is interp.hpp's.
//   d = a - r at every node i of a's geometry, in i's own element e = i / block: the value is z[i], the gradient is the
//   physical gradient of e's nodal basis at x_i (what the dx / dy / dz operator rows give).  r is nothing, nodal reference
//   values (optionally with reference gradients), or a field on another geometry of the same element kind.  The other mesh's
//   element is the one containing the NUDGED point x_i + theta (c_e - x_i), theta = 2^-20, c_e = mean of the nodes of e;
//   its polynomial and gradient are then evaluated at x_i itself.  A node whose nudged point lies in no element of the other
//   mesh contributes nothing and is counted.
// Per column five contributions: w d | w |d|^q | w |grad d|_2^q | |d| | |grad d|_2 (three sums, two maxima).
#pragma once
#include "interp.hpp"
#include "reduce.hpp"

namespace mgb {
namespace norms {

using namespace reduce;                       // kCols (MGB_NORM_COLS), kThreads, combine, workgroups
constexpr double kTheta = 1.0 / 1048576.0;    // 2^-20

struct Args {
  interp::BinsView own;               // a's geometry: x and block (its bins are not used)
  const double* w = nullptr;          // n quadrature weights
  const double* z = nullptr;          // n x S
  const double* ref_vals = nullptr;   // n x S or null
  const double* ref_grads = nullptr;  // n x S x dim or null
  interp::BinsView other;             // the other geometry's locator (cross only)
  const double* z_other = nullptr;    // n_other x S
  bool cross = false;
  int n = 0, S = 0;
  double q = 2.0;
};

// a^q for a >= 0 (or NaN, which it returns): no pow for q = 2 and q = 1, zero for a = 0
MGB_HD double powq(double a, double q) {
  if (q == 2.0) return a * a;
  if (q == 1.0) return a;
  return a == 0.0 ? 0.0 : pow(a, q);
}

template <int DIM, int K>
struct Node {
  interp::ElemBasis<DIM, K> own, oth;
  const double *ze, *re, *zo;      // the contiguous block * S nodal values of the own / reference / other element
  int i;
  bool outside;
  double w;

  // basis of the own element at x_i (reference coordinates through ref_coords, the inside flag ignored); across meshes the
  // other element by the nudged point and its basis at x_i
  MGB_HD void init(const Args& A, int node) {
    i = node;
    outside = false;
    w = A.w[i];
    const int block = A.own.block, e = i / block;
    const double* p = A.own.x + (size_t)i * DIM;
    double r[DIM];
    interp::ref_coords<DIM>(A.own.x, block, e, p, r);
    own.init(A.own.x, block, e, r);
    ze = A.z + (size_t)e * block * A.S;
    re = A.ref_vals ? A.ref_vals + (size_t)e * block * A.S : nullptr;
    zo = nullptr;
    if (A.cross) {
      const double* xe = A.own.x + (size_t)e * block * DIM;
      double pn[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) {
        double c = 0.0;
        for (int j = 0; j < block; ++j) c += xe[(size_t)j * DIM + d];
        c /= (double)block;
        pn[d] = p[d] + kTheta * (c - p[d]);
      }
      const int f = interp::find_element<DIM>(A.other, pn);
      outside = f < 0;
      if (!outside) {
        interp::ref_coords<DIM>(A.other.x, A.other.block, f, p, r);
        oth.init(A.other.x, A.other.block, f, r);
        zo = A.z_other + (size_t)f * A.other.block * A.S;
      }
    }
  }

  // the five contributions of this node to column s
  MGB_HD void column(const Args& A, int s, double* c) const {
    if (outside) {
      c[0] = c[1] = c[2] = c[3] = c[4] = 0.0;
      return;
    }
    const int S = A.S;
    double d = A.z[(size_t)i * S + s], unused, g[DIM];
    if (re && !A.ref_grads) {
      own.template eval<true>(ze, re, S, s, unused, g);      // the element gradient of the nodal field a - ref_vals
    } else {
      own.template eval<false>(ze, nullptr, S, s, unused, g);
    }
    if (re) {
      d -= A.ref_vals[(size_t)i * S + s];
      if (A.ref_grads) {
#pragma unroll
        for (int k = 0; k < DIM; ++k) g[k] -= A.ref_grads[((size_t)i * S + s) * DIM + k];
      }
    } else if (zo) {
      double vb, gb[DIM];
      oth.template eval<false>(zo, nullptr, S, s, vb, gb);
      d -= vb;
#pragma unroll
      for (int k = 0; k < DIM; ++k) g[k] -= gb[k];
    }
    double gs = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) gs += g[k] * g[k];
    const double ad = fabs(d), gn = sqrt(gs);
    c[0] = w * d;
    c[1] = w * powq(ad, A.q);
    c[2] = w * (A.q == 2.0 ? gs : powq(gn, A.q));
    c[3] = ad;
    c[4] = gn;
  }
};

// host restatement: the same per-node routine, serially, in ascending node order
struct HostNorms {
  Args A;
  double* out;      // S x kCols
  long long* outside;
  template <int DIM, int K>
  void operator()() const {
    for (int k = 0; k < A.S * kCols; ++k) out[k] = 0.0;
    long long cnt = 0;
    for (int i = 0; i < A.n; ++i) {
      Node<DIM, K> N;
      N.init(A, i);
      cnt += N.outside;
      for (int s = 0; s < A.S; ++s) {
        double c[kCols];
        N.column(A, s, c);
        combine(out + (size_t)s * kCols, c);
      }
    }
    if (outside) *outside = cnt;
  }
};

inline void field_norms_host(int dim, int k, const Args& A, double* out, long long* outside) {
  HostNorms h{A, out, outside};
  interp::dispatch(dim, k, h);
}

// the doubles / counters of scratch the two launches need, and where the finish leaves its results in them
inline size_t scratch_doubles(int n, int S) { return (size_t)(workgroups(n) + 1) * S * kCols; }      // partials, then S x kCols results
inline size_t results_offset(int n, int S) { return (size_t)workgroups(n) * S * kCols; }
inline size_t scratch_counts(int n) { return (size_t)workgroups(n) + 1; }                            // partials, then the total
inline size_t count_offset(int n) { return (size_t)workgroups(n); }

#if defined(__HIPCC__)
// norms.hip: two launches on `stream` (partials per workgroup and column, then the finish of reduce.hpp, one workgroup per
// column); all pointers are device pointers; the S x kCols results are at scratch + results_offset, the count of outside
// nodes at counts + count_offset
void launch_field_norms(hipStream_t stream, int dim, int k, const Args& A, double* scratch, long long* counts);
#endif

}  // namespace norms
}  // namespace mgb
