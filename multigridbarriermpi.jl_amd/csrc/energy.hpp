// Energy, flux and cone margin of p-Laplace solutions by the nodal quadrature rule: what ONE node
// contributes, written ONCE.  The gfx950 kernels (energy.hip) and the host restatement (mgb_geo_field_energy_host) both run
// Node below; the element maths is interp.hpp's, powq is norms.hpp's, combine and identity are reduce.hpp's.
//   At node i of a field z (n x S row-major), in i's own element e = i / block:
//     g = physical gradient of column u at x_i (what the dx / dy / dz operator rows give), a = |g|_2, p = the exponent at i,
//     P = a^p (no pow for p = 2 and p = 1, zero for a = 0), s_i = column s, f_i = nodal forcing (null: 0), w_i the weight.
//   Five contributions: w P / p | w f u | w (s - P) / p | a^(p-1) | P - s   (three sums, two NaN-sticky maxima).
//   A non-finite u_i, s_i, f_i or gradient, or an exponent that is not a finite real >= 1, makes all five NaN.
//   Flux: sigma = a^(p-2) g -- g itself (bit for bit) at p = 2, g / a at p = 1, exactly 0 where a = 0.
// The arithmetic of Node::contributions and Node::flux is kept as written (fp contract off): products and the sums behind
// them do not fuse, so a batch of fields and the same fields one by one run the same operations.
#pragma once
#include "norms.hpp"

namespace mgb {
namespace energy {

using namespace reduce;      // kCols (MGB_ENERGY_COLS), kThreads, combine, identity, workgroups
using norms::powq;

// what all fields of one call share: geometry, exponent, columns
struct Args {
  interp::BinsView own;               // the geometry: x and block (its bins are not used)
  const double* w = nullptr;          // n quadrature weights
  const double* p_nodal = nullptr;    // n exponents, or null: p everywhere
  double p = 2.0;
  const double* const* z = nullptr;   // B pointers to n x S fields
  const double* f = nullptr;          // forcing: null, n values shared by all fields (f_stride 0) or B x n (f_stride n)
  long long f_stride = 0;
  int n = 0, S = 0, u = 0, s = 0, B = 0;
};

// a^(p-1) for a >= 0: 1 at p = 1 where a > 0, 0 at a = 0
MGB_HD double powm1(double a, double p) {
  if (p == 2.0) return a;
  if (a == 0.0) return 0.0;
  if (p == 1.0) return 1.0;
  return pow(a, p - 1.0);
}

template <int DIM, int K>
struct Node {
  interp::ElemBasis<DIM, K> own;
  size_t first;      // first node of the own element
  int i;
  double w, p;

  // basis of the own element at x_i, as norms::Node takes it
  MGB_HD void init(const Args& A, int node) {
    i = node;
    w = A.w[i];
    p = A.p_nodal ? A.p_nodal[i] : A.p;
    const int block = A.own.block, e = i / block;
    double r[DIM];
    interp::ref_coords<DIM>(A.own.x, block, e, A.own.x + (size_t)i * DIM, r);
    own.init(A.own.x, block, e, r);
    first = (size_t)e * block;
  }

  MGB_HD void gradient(const double* z, int S, int u, double* g) const {
    double unused;
    own.template eval<false>(z + first * S, nullptr, S, u, unused, g);
  }

  // the five contributions of this node for the field z with forcing row f (nullable)
  MGB_HD void contributions(const Args& A, const double* z, const double* f, double* c) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double g[DIM];
    gradient(z, A.S, A.u, g);
    double gs = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) gs += g[k] * g[k];
    const double ui = z[(size_t)i * A.S + A.u], si = z[(size_t)i * A.S + A.s], fi = f ? f[i] : 0.0;
    bool good = p >= 1.0;
    good = good & interp::finite(p);
    good = good & interp::finite(ui);
    good = good & interp::finite(si);
    good = good & interp::finite(fi);
    good = good & interp::finite(gs);
    if (!good) {
      c[0] = c[1] = c[2] = c[3] = c[4] = std::numeric_limits<double>::quiet_NaN();
      return;
    }
    const double a = sqrt(gs), P = powq(a, p);
    c[0] = w * P / p;
    c[1] = w * fi * ui;
    c[2] = w * (si - P) / p;
    c[3] = powm1(a, p);
    c[4] = P - si;
  }

  // sigma[DIM] = a^(p-2) g
  MGB_HD void flux(const double* z, int S, int u, double* sigma) const {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double g[DIM];
    gradient(z, S, u, g);
    if (p == 2.0) {
#pragma unroll
      for (int k = 0; k < DIM; ++k) sigma[k] = g[k];
      return;
    }
    double gs = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) gs += g[k] * g[k];
    const double a = sqrt(gs);
    const bool one = p == 1.0;
    double m = std::numeric_limits<double>::quiet_NaN();      // stays for an exponent that is not a finite real >= 1
    const bool fin = interp::finite(p);
    if (fin & (p >= 1.0)) m = one ? 1.0 : pow(a, p - 2.0);
#pragma unroll
    for (int k = 0; k < DIM; ++k) sigma[k] = a == 0.0 ? 0.0 : (one ? g[k] / a : m * g[k]);
  }
};

// host restatement: the same per-node routine, serially, field after field in ascending node order
struct HostEnergy {
  Args A;
  double* out;       // B x kCols
  double* flux;      // B x n x dim or null
  template <int DIM, int K>
  void operator()() const {
    for (int b = 0; b < A.B; ++b) {
      double* acc = out + (size_t)b * kCols;
      identity(acc);
      const double* f = A.f ? A.f + (size_t)b * A.f_stride : nullptr;
      for (int i = 0; i < A.n; ++i) {
        Node<DIM, K> N;
        N.init(A, i);
        double c[kCols];
        N.contributions(A, A.z[b], f, c);
        combine(acc, c);
        if (flux) N.flux(A.z[b], A.S, A.u, flux + ((size_t)b * A.n + i) * DIM);
      }
    }
  }
};

inline void field_energy_host(int dim, int k, const Args& A, double* out, double* flux) {
  HostEnergy h{A, out, flux};
  interp::dispatch(dim, k, h);
}

// the doubles of scratch the two launches need, and where the finish leaves its results in them
inline size_t scratch_doubles(int n, int B) { return (size_t)(workgroups(n) + 1) * B * kCols; }      // partials, then B x kCols results
inline size_t results_offset(int n, int B) { return (size_t)workgroups(n) * B * kCols; }

#if defined(__HIPCC__)
// energy.hip: two launches on `stream` -- partials on grid (workgroups, B), then the finish of reduce.hpp, one workgroup per
// field; all pointers of A are device pointers (A.z a device table of B device pointers); the B x kCols results are at
// scratch + results_offset
void launch_field_energy(hipStream_t stream, int dim, int k, const Args& A, double* scratch);
// one launch on grid (workgroups, A.B), one thread per node: flux (A.B x n x dim) of the fields of the device table A.z, or of
// the ONE field z where A.z is null (then A.B = 1); of A the geometry, exponent, S, u, B and z are read
void launch_field_flux(hipStream_t stream, int dim, int k, const Args& A, const double* z, double* flux);
#endif

}  // namespace energy
}  // namespace mgb
