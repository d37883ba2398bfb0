// Residual error indicators of p-Laplace solutions: what ONE node, ONE facet node and ONE element
// contribute, written ONCE.  The gfx950 kernels (estimate.hip) and the host restatement (mgb_geo_estimate_host) both run the
// routines below; sigma is energy.hpp's Node::flux (the launch of mgb_geo_field_flux, the same bits), the element maths is
// interp.hpp's, powq is norms.hpp's, combine and nanmax are reduce.hpp's, the facet lists are boundary.hpp's.
//   Sigma (n x dim) is the nodal flux |grad u|^(p-2) grad u, every node in its own element.  lambda_i is the scale: a scalar,
//   or p_i (the problem  min int f u + s,  s >= |grad u|^p  has the strong form  f - p div sigma = 0  and the natural condition
//   p sigma . n + h = 0; lambda = 1 is energy()'s convention).  r >= 1 is the power.
//   Node i of element e:      rho_i = f_i - lambda_i sum_k d_k (I Sigma_k)(x_i), the divergence of the element interpolant of
//                             the nodal flux through ElemBasis::eval on Sigma as a field of dim columns, k ascending;
//                             term  w_i |rho_i|^r.
//   Interior facet F, node j: rows a, b of the two sides, lambda at a:  J_Fj = lambda ((Sigma_a - Sigma_b) . n_F), k ascending;
//                             J_F = sum_j omega_Fj |J_Fj|^r, j ascending.
//   Neumann facet F, node j:  row i:  N_F = sum_j omega_Fj |lambda_i (Sigma_i . n) + h_Fj|^r, j ascending; a facet the mask
//                             leaves out gives 0 and its h is not read.
//   Element e:  h_e = (sum_{i in e} w_i)^(1/dim);  vol = h_e^r sum_i w_i |rho_i|^r (local i ascending);  jump = (h_e / 2) sum J_F
//               over its interior facets and  neu = h_e sum N_F over its boundary facets (local facet ascending, through the
//               element -> facet table);  eta_e^r = (vol + jump) + neu.
//   Totals, through reduce::combine: sum vol | sum jump | sum neu | max_e eta_e^r | max |J_Fj|.
//   A non-finite Sigma, f or h, or an exponent that is not a finite real >= 1, makes the term it feeds NaN, and with it the
//   numbers of the element and the totals; the maxima are NaN-sticky.
// The arithmetic is kept as written (fp contract off), as energy.hpp's is.
#pragma once
#include "boundary.hpp"

namespace mgb {
namespace estimate {

using namespace reduce;       // kCols (MGB_ESTIMATE_COLS), kThreads, combine, nanmax
constexpr int kParts = 3;     // vol, jump, neu
using norms::powq;

struct Args {
  interp::BinsView own;                    // the geometry: x and block (its bins are not used)
  const double* w = nullptr;               // n quadrature weights
  const double* p_nodal = nullptr;         // n exponents, or null: p everywhere
  double p = 2.0;
  const double* sigma = nullptr;           // n x dim nodal flux
  const double* f = nullptr;               // n forcing values or null: 0
  double r = 2.0;
  double scale = 1.0;                      // lambda where own_scale, else lambda_i = p_i
  bool own_scale = false;
  int n = 0, nel = 0, nlf = 0, q = 0;
  // interior facets
  const int* inodes = nullptr;             // nif x 2 x q
  const double* iweights = nullptr;        // nif x q
  const double* inormal = nullptr;         // nif x dim, out of the first side
  int nif = 0;
  // boundary facets; h null: no Neumann data, the boundary contributes nothing
  const int* bnodes = nullptr;             // nf x q
  const double* bweights = nullptr;        // nf x q
  const double* bnormal = nullptr;         // nf x dim
  const unsigned char* mask = nullptr;     // nf bytes or null: 0 leaves the facet out
  const double* h = nullptr;               // nf x q
  int nf = 0;
  const int* elem_facet = nullptr;         // nel x nlf: interior facet, or -1 - boundary facet
};

// every column is a sum or a maximum of non-negative values: zeros, which hides reduce::identity and its -inf
MGB_HD void identity(double* c) { c[0] = c[1] = c[2] = c[3] = c[4] = 0.0; }

MGB_HD double exponent(const Args& A, int i) { return A.p_nodal ? A.p_nodal[i] : A.p; }
MGB_HD bool good_exponent(double p) { return (p >= 1.0) & interp::finite(p); }
MGB_HD double lambda(const Args& A, int i) { return A.own_scale ? A.scale : exponent(A, i); }
MGB_HD double nan() { return std::numeric_limits<double>::quiet_NaN(); }

// h_e from the sum of the weights of an element
template <int DIM>
MGB_HD double diameter(double ws) {
  if constexpr (DIM == 1) return ws;
  else if constexpr (DIM == 2) return sqrt(ws);
  else return cbrt(ws);
}

template <int DIM, int K>
struct Terms {
  // w_i |rho_i|^r of node i
  MGB_HD static double node(const Args& A, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int block = A.own.block, e = i / block;
    double rc[DIM];
    interp::ref_coords<DIM>(A.own.x, block, e, A.own.x + (size_t)i * DIM, rc);
    interp::ElemBasis<DIM, K> own;
    own.init(A.own.x, block, e, rc);
    const double* se = A.sigma + (size_t)e * block * DIM;
    double div = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      double unused, g[DIM];
      own.template eval<false>(se, nullptr, DIM, k, unused, g);
      div += g[k];
    }
    const double pi = exponent(A, i), fi = A.f ? A.f[i] : 0.0;
    bool good = good_exponent(pi);
    good = good & interp::finite(fi);
    good = good & interp::finite(div);
    if (!good) return nan();
    const double rho = fi - lambda(A, i) * div;
    return A.w[i] * powq(fabs(rho), A.r);
  }

  // omega |J_Fj|^r of node j of interior facet F; aj = |J_Fj|
  MGB_HD static double jump(const Args& A, int F, int j, double& aj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int a = A.inodes[((size_t)F * 2 + 0) * A.q + j], b = A.inodes[((size_t)F * 2 + 1) * A.q + j];
    const double* n = A.inormal + (size_t)F * DIM;
    const double* sa = A.sigma + (size_t)a * DIM;
    const double* sb = A.sigma + (size_t)b * DIM;
    const double pa = exponent(A, a);
    bool good = good_exponent(pa);
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      d += (sa[k] - sb[k]) * n[k];
      good = good & interp::finite(sa[k]);
      good = good & interp::finite(sb[k]);
    }
    if (!good) {
      aj = nan();
      return nan();
    }
    aj = fabs(lambda(A, a) * d);
    return A.iweights[(size_t)F * A.q + j] * powq(aj, A.r);
  }

  // omega |lambda_i Sigma_i . n + h_Fj|^r of node j of boundary facet F (the caller has looked at the mask)
  MGB_HD static double neumann(const Args& A, int F, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int i = A.bnodes[(size_t)F * A.q + j];
    const double* n = A.bnormal + (size_t)F * DIM;
    const double* si = A.sigma + (size_t)i * DIM;
    const double pi = exponent(A, i), hj = A.h[(size_t)F * A.q + j];
    bool good = good_exponent(pi);
    good = good & interp::finite(hj);
    double sn = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      sn += si[k] * n[k];
      good = good & interp::finite(si[k]);
    }
    if (!good) return nan();
    return A.bweights[(size_t)F * A.q + j] * powq(fabs(lambda(A, i) * sn + hj), A.r);
  }

  // the three numbers of element e from  ts = sum_i w_i |rho_i|^r,  ws = sum_i w_i  and the per-facet values J (nif), N (nf or
  // null)
  MGB_HD static void element(const Args& A, int e, double ts, double ws, const double* J, const double* N, double* parts) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double he = diameter<DIM>(ws);
    double js = 0.0, ns = 0.0;
    for (int lf = 0; lf < A.nlf; ++lf) {
      const int t = A.elem_facet[(size_t)e * A.nlf + lf];
      if (t >= 0) js += J[t];
      else if (N) ns += N[-1 - t];
    }
    parts[0] = powq(he, A.r) * ts;
    parts[1] = (0.5 * he) * js;
    parts[2] = he * ns;
  }
};

// eta_e^r and the element's contribution to the five columns
MGB_HD void element_columns(const double* parts, double* c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  c[0] = parts[0];
  c[1] = parts[1];
  c[2] = parts[2];
  c[3] = (parts[0] + parts[1]) + parts[2];
  c[4] = 0.0;
}

// host restatement: the same routines, serially -- facets, then elements in ascending order
struct HostEstimate {
  Args A;
  double* eta;      // nel x kParts
  double* J;        // nif
  double* N;        // nf or null (no Neumann data)
  double* out;      // kCols
  template <int DIM, int K>
  void operator()() const {
    using T = Terms<DIM, K>;
    double acc[kCols];
    identity(acc);
    for (int F = 0; F < A.nif; ++F) {
      double s = 0.0;
      for (int j = 0; j < A.q; ++j) {
        double aj;
        s += T::jump(A, F, j, aj);
        acc[4] = nanmax(acc[4], aj);
      }
      J[F] = s;
    }
    if (A.h)
      for (int F = 0; F < A.nf; ++F) {
        double s = 0.0;
        if (!A.mask || A.mask[F])
          for (int j = 0; j < A.q; ++j) s += T::neumann(A, F, j);
        N[F] = s;
      }
    const int block = A.own.block;
    for (int e = 0; e < A.nel; ++e) {
      double ts = 0.0, ws = 0.0;
      for (int li = 0; li < block; ++li) {
        ts += T::node(A, e * block + li);
        ws += A.w[e * block + li];
      }
      double* parts = eta + (size_t)e * kParts;
      T::element(A, e, ts, ws, J, A.h ? N : nullptr, parts);
      double c[kCols];
      element_columns(parts, c);
      combine(acc, c);
    }
    for (int k = 0; k < kCols; ++k) out[k] = acc[k];
  }
};

inline void estimate_host(int dim, int k, const Args& A, double* eta, double* J, double* N, double* out) {
  HostEstimate h{A, eta, J, N, out};
  interp::dispatch(dim, k, h);
}

// the nodal flux on the host: energy.hpp's Node::flux node after node, what flux_kernel runs
struct HostFlux {
  const energy::Args& E;
  const double* z;
  double* sigma;
  template <int DIM, int K>
  void operator()() const {
    for (int i = 0; i < E.n; ++i) {
      energy::Node<DIM, K> N;
      N.init(E, i);
      N.flux(z, E.S, E.u, sigma + (size_t)i * DIM);
    }
  }
};

inline void field_flux_host(int dim, int k, const energy::Args& E, const double* z, double* sigma) {
  HostFlux h{E, z, sigma};
  interp::dispatch(dim, k, h);
}

// grouping of the two launches: whole facets and whole elements per workgroup
inline int facets_launched(const Args& A) { return A.nif + (A.h ? A.nf : 0); }
inline long long facet_workgroups(int facets, int q) {
  const int fpw = kThreads / q;
  return ((long long)facets + fpw - 1) / fpw;      // 0 for no facet: the launch is left out
}
inline long long element_workgroups(int nel, int block) {
  const int epw = kThreads / block;
  return ((long long)nel + epw - 1) / epw;
}
// doubles of scratch: element partials (kCols each), facet partial maxima, then the kCols results
inline size_t scratch_doubles(int nel, int block, int facets, int q) {
  return (size_t)element_workgroups(nel, block) * kCols + (size_t)facet_workgroups(facets, q) + kCols;
}
inline size_t results_offset(int nel, int block, int facets, int q) {
  return (size_t)element_workgroups(nel, block) * kCols + (size_t)facet_workgroups(facets, q);
}

#if defined(__HIPCC__)
// estimate.hip: up to three launches on `stream` behind the flux launch that wrote A.sigma -- facet_terms_kernel (left out when
// there is no facet), element_indicator_kernel, estimate_finish.  All pointers are device pointers; J: nif, N: nf (read only
// where A.h is set), eta: nel x kParts; the kCols results are at scratch + results_offset
void launch_estimate(hipStream_t stream, int dim, int k, const Args& A, double* J, double* N, double* eta, double* scratch);
#endif

}  // namespace estimate
}  // namespace mgb
