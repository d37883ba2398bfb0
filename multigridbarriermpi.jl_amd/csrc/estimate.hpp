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
//
// Steps of a parabolic run.  Snapshots Z_0 .. Z_B at strictly increasing times, h_k = ts[k] - ts[k-1];
// step k = 1..B solved  min int (1/2h_k)(s1 - 2 u u_(k-1)) + (1/p) s2 + f_k u,  whose strong form is
// (u_k - u_(k-1)) / h_k + f_k - div sigma_k = 0  with the natural condition  sigma_k . n + h_k^N = 0: the residual above with
// lambda = scale (own_scale) and ONE more term.  Field b = k - 1 of a call with Args::steps set:
//   Sigma^m, m = 0..B: the nodal flux of snapshot m, (B + 1) x n x dim; step k reads Sigma^k and Sigma^(k-1).
//   Node i:     d_i = (u^k_i - u^(k-1)_i) / h_k, a subtraction, then a division;  rho_i = (f_k,i + d_i) - lambda div(I Sigma^k)(x_i);
//               rate term  w_i |d_i|^r;  time term  w_i |Sigma^k_i - Sigma^(k-1)_i|_2^r, the 2-norm a square root of the squares
//               summed in ascending component order, the power through powq.
//   Element e:  vol, jump, neu from Sigma^k as above (Neumann data of the step's new time);  tim_e = sum_{i in e} of the time terms,
//               local i ascending.  Four numbers per (step, element): vol, jump, neu, tim.
//   Two rows of totals per step, through reduce::combine:  row 0 as above;
//               row 1:  sum tim | sum_i w_i |d_i|^r | 0 | max_e tim_e | max_i |d_i|  (the rate sum per element in ascending local
//               order, then over the elements).
//   A non-finite u^k_i, u^(k-1)_i or h_k makes d_i NaN, a non-finite Sigma^k_i or Sigma^(k-1)_i the time term; a NaN in snapshot m
//   reaches steps m and m + 1 and no other.  What a step's numbers are made of depends on its two snapshots, its f, h and h_k
//   alone: a batch of B steps gives the bits of B calls with B = 1.  Where both snapshots of a step hold the same values, d = 0
//   exactly, rho = (f + 0.0) - lambda div, and row 0 and vol, jump, neu are those of the single field with own_scale.
#pragma once
#include "boundary.hpp"

namespace mgb {
namespace estimate {

using namespace reduce;       // kCols (MGB_ESTIMATE_COLS), kThreads, combine, nanmax
constexpr int kParts = 3;     // vol, jump, neu
constexpr int kStepParts = 4; // vol, jump, neu, tim of a step
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
  // B fields in one call (blockIdx.y); steps: field b is step b + 1 of a parabolic run and the members below are read.  In a
  // call, sigma is the first flux ((B + 1) x n x dim for steps), f and h the first rows; field() moves them to one field
  int B = 1;
  bool steps = false;
  const double* const* z = nullptr;        // B + 1 snapshots of n x S
  int S = 0, u = 0;
  const double* dt = nullptr;              // B step sizes h_k
  long long f_stride = 0, h_stride = 0;    // 0: one row for every step; n and nf x q: a row per step
  // of ONE field, set by field(): the previous flux, the two snapshots and the step size
  const double* sigma_prev = nullptr;
  const double* z_new = nullptr;
  const double* z_old = nullptr;
  double hk = 1.0;
};

inline int parts_of(const Args& A) { return A.steps ? kStepParts : kParts; }
inline int rows_of(const Args& A) { return A.steps ? 2 : 1; }

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
  // field b of a call: what the routines below read
  MGB_HD static Args field(const Args& A, int b) {
    Args a = A;
    if (!A.steps) return a;      // one field: the call's pointers are the field's
    const size_t nsig = (size_t)A.n * DIM;
    a.sigma_prev = A.sigma + (size_t)b * nsig;
    a.sigma = A.sigma + ((size_t)b + 1) * nsig;
    if (A.f) a.f = A.f + (size_t)b * A.f_stride;
    if (A.h) a.h = A.h + (size_t)b * A.h_stride;
    a.z_old = A.z[b];
    a.z_new = A.z[b + 1];
    a.hk = A.dt[b];
    return a;
  }

  // d_i = (u^k_i - u^(k-1)_i) / h_k of node i of a step
  MGB_HD static double quotient(const Args& A, int i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = A.z_new[(size_t)i * A.S + A.u], b = A.z_old[(size_t)i * A.S + A.u];
    bool good = interp::finite(a);
    good = good & interp::finite(b);
    good = good & interp::finite(A.hk);
    if (!good) return nan();
    const double diff = a - b;
    return diff / A.hk;
  }

  // the step-only numbers of node i from its d:  tim = w_i |Sigma^k_i - Sigma^(k-1)_i|_2^r,  rate = w_i |d_i|^r,  ad = |d_i|
  MGB_HD static void step(const Args& A, int i, double d, double& tim, double& rate, double& ad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double* sn = A.sigma + (size_t)i * DIM;
    const double* so = A.sigma_prev + (size_t)i * DIM;
    bool good = true;
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const double diff = sn[k] - so[k];
      ss += diff * diff;
      good = good & interp::finite(sn[k]);
      good = good & interp::finite(so[k]);
    }
    tim = good ? A.w[i] * powq(sqrt(ss), A.r) : nan();
    ad = fabs(d);      // NaN stays NaN
    rate = A.w[i] * powq(ad, A.r);
  }

  // w_i |rho_i|^r of node i; d = d_i of a step, not read for a single field
  MGB_HD static double node(const Args& A, int i, double d = 0.0) {
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
    if (A.steps) good = good & (d == d);
    if (!good) return nan();
    const double rho = (A.steps ? fi + d : fi) - lambda(A, i) * div;
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

// the element's contribution to row 1 of a step: tim_e, its rate sum and its largest |d_i|
MGB_HD void step_columns(double tim, double rate, double dmax, double* c) {
  c[0] = tim;
  c[1] = rate;
  c[2] = 0.0;
  c[3] = tim;
  c[4] = dmax;
}

// host restatement: the same routines, serially -- field after field; in a field the facets, then the elements in ascending order
struct HostEstimate {
  Args A;           // the call: A.B fields
  double* eta;      // B x nel x parts_of(A)
  double* J;        // B x nif
  double* N;        // B x nf or null (no Neumann data)
  double* out;      // B x rows_of(A) x kCols
  template <int DIM, int K>
  void operator()() const {
    using T = Terms<DIM, K>;
    const int block = A.own.block, np = parts_of(A), nr = rows_of(A);
    for (int b = 0; b < A.B; ++b) {
      const Args Ab = T::field(A, b);
      double* Jb = J + (size_t)b * A.nif;
      double* Nb = A.h ? N + (size_t)b * A.nf : nullptr;
      double acc[kCols], acc1[kCols];
      identity(acc);
      identity(acc1);
      for (int F = 0; F < A.nif; ++F) {
        double s = 0.0;
        for (int j = 0; j < A.q; ++j) {
          double aj;
          s += T::jump(Ab, F, j, aj);
          acc[4] = nanmax(acc[4], aj);
        }
        Jb[F] = s;
      }
      if (A.h)
        for (int F = 0; F < A.nf; ++F) {
          double s = 0.0;
          if (!A.mask || A.mask[F])
            for (int j = 0; j < A.q; ++j) s += T::neumann(Ab, F, j);
          Nb[F] = s;
        }
      for (int e = 0; e < A.nel; ++e) {
        double ts = 0.0, ws = 0.0, tim = 0.0, rate = 0.0, dmax = 0.0;
        for (int li = 0; li < block; ++li) {
          const int i = e * block + li;
          double d = 0.0;
          if (A.steps) {
            double t, rt, ad;
            d = T::quotient(Ab, i);
            T::step(Ab, i, d, t, rt, ad);
            tim += t;
            rate += rt;
            dmax = nanmax(dmax, ad);
          }
          ts += T::node(Ab, i, d);
          ws += A.w[i];
        }
        double* parts = eta + ((size_t)b * A.nel + e) * np;
        T::element(Ab, e, ts, ws, Jb, Nb, parts);
        double c[kCols];
        element_columns(parts, c);
        combine(acc, c);
        if (A.steps) {
          parts[3] = tim;
          step_columns(tim, rate, dmax, c);
          combine(acc1, c);
        }
      }
      double* row = out + (size_t)b * nr * kCols;
      for (int k = 0; k < kCols; ++k) row[k] = acc[k];
      if (A.steps)
        for (int k = 0; k < kCols; ++k) row[kCols + k] = acc1[k];
    }
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
// doubles of scratch of a call of B fields with R rows of totals each: element partials (B x R x workgroups x kCols), facet
// partial maxima (B x workgroups), then the B x R x kCols results
inline size_t results_offset(int nel, int block, int facets, int q, int B = 1, int R = 1) {
  return (size_t)B * ((size_t)R * element_workgroups(nel, block) * kCols + (size_t)facet_workgroups(facets, q));
}
inline size_t scratch_doubles(int nel, int block, int facets, int q, int B = 1, int R = 1) {
  return results_offset(nel, block, facets, q, B, R) + (size_t)B * R * kCols;
}

#if defined(__HIPCC__)
// estimate.hip: up to three launches on `stream` behind the flux launch that wrote A.sigma -- facet_terms_kernel (left out when
// there is no facet), element_indicator_kernel, estimate_finish, each with the field in blockIdx.y (the finish: one workgroup
// per row of totals).  All pointers are device pointers; J: B x nif, N: B x nf (read only where A.h is set), eta: B x nel x
// parts_of(A); the B x rows_of(A) x kCols results are at scratch + results_offset
void launch_estimate(hipStream_t stream, int dim, int k, const Args& A, double* J, double* N, double* eta, double* scratch);
#endif

}  // namespace estimate
}  // namespace mgb
