// Evaluation of a nodal field at arbitrary points: inverse element maps, nodal bases, the containment
// rule and the bin grid that finds an element, written ONCE.  The gfx950 kernel (interp.hip) and the host restatement
// (mgb_geo_interpolate_host) both run eval_point below, the way kernels_tpl.hpp is shared; norms.hpp builds on the same
// pieces (ElemBasis, find_element).
//   1-D: block 2 (left, right), P1.          2-D: block 7 (v1 v2 v3 m12 m23 m31 centroid, geometry.cpp), P2 + cubic bubble.
//   3-D: block (k+1)^3, k = 1..3, equispaced tensor nodes (x fastest) on the axis-aligned box of the first and last row.
// Containment (public contract): reference coordinates, tau = 1e-12; inside when min(lambda) >= -tau (2-D) or every
// xi_a in [-tau, 1 + tau] (1-D, 3-D); of all elements containing a point the LOWEST index wins; a point in no element, or
// with a non-finite coordinate, is outside: NaN in every output column, element -1.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "errors.hpp"
#include "geometry.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MGB_HD __host__ __device__ inline
#else
#define MGB_HD inline
#endif

namespace mgb {
namespace interp {

constexpr double kTau = 1e-12;

// the locator as the evaluation sees it: plain pointers, host or device
struct BinsView {
  int nel = 0, block = 0;
  int nc[3] = {1, 1, 1};            // cells per axis
  double lo[3] = {0, 0, 0};         // lower corner of the bounding box
  double inv[3] = {0, 0, 0};        // cells per unit length
  const int* cellptr = nullptr;     // CSR: cell -> ascending elements whose grown bounding box overlaps it
  const int* cellelem = nullptr;
  const double* x = nullptr;        // n x dim node coordinates
};

MGB_HD bool finite(double v) { return (v - v) == 0.0; }

// cell coordinate of p along one axis, clamped to the grid (monotone in p: an element's points stay inside its cell range)
MGB_HD int cell_coord(double p, double lo, double inv, int nc) {
  double t = (p - lo) * inv;
  const double top = (double)(nc - 1);
  t = t > 0.0 ? t : 0.0;
  t = t < top ? t : top;
  return (int)t;
}

// reference coordinates r[DIM] of p in element e; true when p is inside by the containment rule.  Comparisons, not fmin:
// a NaN coordinate is never inside.
template <int DIM>
MGB_HD bool ref_coords(const double* x, int block, int e, const double* p, double* r) {
  if constexpr (DIM == 2) {
    const double* v = x + (size_t)e * 14;
    const double ax = v[2] - v[0], ay = v[3] - v[1], bx = v[4] - v[0], by = v[5] - v[1];
    const double det = ax * by - ay * bx, px = p[0] - v[0], py = p[1] - v[1];
    r[0] = (px * by - py * bx) / det;
    r[1] = (ax * py - ay * px) / det;
    const double l0 = 1.0 - r[0] - r[1];
    return (l0 >= -kTau) & (r[0] >= -kTau) & (r[1] >= -kTau);
  } else {
    const double* a = x + (size_t)e * block * DIM;
    const double* b = a + (size_t)(block - 1) * DIM;
    bool in = true;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      r[d] = (p[d] - a[d]) / (b[d] - a[d]);
      in = in & (r[d] >= -kTau) & (r[d] <= 1.0 + kTau);
    }
    return in;
  }
}

// P2 + cubic-bubble nodal basis at (xi, eta): values and reference gradients (the closed form of geometry.cpp: tri_basis)
MGB_HD void tri_basis(double xi, double et, double* val, double* dxi, double* det) {
  const double l[3] = {1.0 - xi - et, xi, et};
  const double gx[3] = {-1.0, 1.0, 0.0}, gy[3] = {-1.0, 0.0, 1.0};
  const double b = l[0] * l[1] * l[2];
  const double bx = gx[0] * l[1] * l[2] + l[0] * gx[1] * l[2] + l[0] * l[1] * gx[2];
  const double by = gy[0] * l[1] * l[2] + l[0] * gy[1] * l[2] + l[0] * l[1] * gy[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int j = i == 2 ? 0 : i + 1;      // edges m12, m23, m31
    val[i] = l[i] * (2.0 * l[i] - 1.0) + 3.0 * b;
    dxi[i] = (4.0 * l[i] - 1.0) * gx[i] + 3.0 * bx;
    det[i] = (4.0 * l[i] - 1.0) * gy[i] + 3.0 * by;
    val[3 + i] = 4.0 * l[i] * l[j] - 12.0 * b;
    dxi[3 + i] = 4.0 * (l[i] * gx[j] + l[j] * gx[i]) - 12.0 * bx;
    det[3 + i] = 4.0 * (l[i] * gy[j] + l[j] * gy[i]) - 12.0 * by;
  }
  val[6] = 27.0 * b;
  dxi[6] = 27.0 * bx;
  det[6] = 27.0 * by;
}

// Lagrange basis of degree K on the equispaced nodes j / K of [0, 1]: values and derivatives at xi
template <int K>
MGB_HD void lagrange(double xi, double* v, double* d) {
  const double t = K * xi;
#pragma unroll
  for (int j = 0; j <= K; ++j) {
    double prod = 1.0, dsum = 0.0;
#pragma unroll
    for (int i = 0; i <= K; ++i)
      if (i != j) prod *= (t - i) / (double)(j - i);
#pragma unroll
    for (int m = 0; m <= K; ++m) {
      if (m == j) continue;
      double q = 1.0 / (double)(j - m);
#pragma unroll
      for (int i = 0; i <= K; ++i)
        if (i != j && i != m) q *= (t - i) / (double)(j - i);
      dsum += q;
    }
    v[j] = prod;
    d[j] = K * dsum;
  }
}

// The basis of ONE element at ONE point, evaluated once and applied to any number of columns: init() takes the reference
// coordinates r of the point in element e (ref_coords), eval() one column s of the element's block * S contiguous nodal
// values ze (row-major n x S) and gives the value and the physical gradient g[DIM].  SUB: the nodal field is ze - sub, the
// difference taken node by node before the sums (norms.hpp).  K = degree of the tensor elements (unused in 2-D).
template <int DIM, int K>
struct ElemBasis {
  static constexpr int M1 = K + 1;
  double bv[DIM][M1], bd[DIM][M1], ih[DIM];
  MGB_HD void init(const double* x, int block, int e, const double* r) {
    const double* a = x + (size_t)e * block * DIM;
    const double* b = a + (size_t)(block - 1) * DIM;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      lagrange<K>(r[d], bv[d], bd[d]);
      ih[d] = 1.0 / (b[d] - a[d]);
    }
  }
  template <bool SUB>
  MGB_HD void eval(const double* ze, const double* sub, int S, int s, double& val, double* g) const {
    if constexpr (DIM == 1) {
      double acc = 0.0, g0 = 0.0;
#pragma unroll
      for (int i = 0; i < M1; ++i) {
        double zz = ze[(size_t)i * S + s];
        if constexpr (SUB) zz -= sub[(size_t)i * S + s];
        acc += bv[0][i] * zz;
        g0 += bd[0][i] * zz;
      }
      val = acc;
      g[0] = g0 * ih[0];
    } else {
      double acc = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
      for (int m = 0; m < M1; ++m)
#pragma unroll
        for (int j = 0; j < M1; ++j) {
          double line = 0.0, dline = 0.0;      // the x-line of nodes (., j, m)
#pragma unroll
          for (int i = 0; i < M1; ++i) {
            double zz = ze[(size_t)(i + M1 * (j + M1 * m)) * S + s];
            if constexpr (SUB) zz -= sub[(size_t)(i + M1 * (j + M1 * m)) * S + s];
            line += bv[0][i] * zz;
            dline += bd[0][i] * zz;
          }
          acc += line * (bv[1][j] * bv[2][m]);
          g0 += dline * (bv[1][j] * bv[2][m]);
          g1 += line * (bd[1][j] * bv[2][m]);
          g2 += line * (bv[1][j] * bd[2][m]);
        }
      val = acc;
      g[0] = g0 * ih[0];
      g[1] = g1 * ih[1];
      g[2] = g2 * ih[2];
    }
  }
};

template <int K>
struct ElemBasis<2, K> {
  double N[7], Nx[7], Ny[7], xx, ex, xy, ey;
  MGB_HD void init(const double* x, int, int e, const double* r) {
    tri_basis(r[0], r[1], N, Nx, Ny);
    const double* v = x + (size_t)e * 14;
    const double ax = v[2] - v[0], ay = v[3] - v[1], bx = v[4] - v[0], by = v[5] - v[1];
    const double idet = 1.0 / (ax * by - ay * bx);
    // physical gradient = T^-T (reference gradient), T = [v2 - v1, v3 - v1]
    xx = by * idet, ex = -ay * idet, xy = -bx * idet, ey = ax * idet;
  }
  template <bool SUB>
  MGB_HD void eval(const double* ze, const double* sub, int S, int s, double& val, double* g) const {
    double acc = 0.0, g0 = 0.0, g1 = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      double zz = ze[(size_t)j * S + s];
      if constexpr (SUB) zz -= sub[(size_t)j * S + s];
      acc += N[j] * zz;
      g0 += Nx[j] * zz;
      g1 += Ny[j] * zz;
    }
    val = acc;
    g[0] = g0 * xx + g1 * ex;
    g[1] = g0 * xy + g1 * ey;
  }
};

// Find the element of a point: the cell, then the ascending candidate list, the first element that contains p; -1 when no
// element does or a coordinate is not finite.
template <int DIM>
MGB_HD int find_element(const BinsView& B, const double* p) {
  bool fin = true;
#pragma unroll
  for (int d = 0; d < DIM; ++d) fin = fin & finite(p[d]);
  int found = -1;
  if (fin) {
    int cell = 0, stride = 1;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      cell += stride * cell_coord(p[d], B.lo[d], B.inv[d], B.nc[d]);
      stride *= B.nc[d];
    }
    const int k1 = B.cellptr[cell + 1];
    for (int k = B.cellptr[cell]; k < k1 && found < 0; ++k) {
      const int e = B.cellelem[k];
      double r[DIM];
      found = ref_coords<DIM>(B.x, B.block, e, p, r) ? e : found;
    }
  }
  return found;
}

// Evaluate the S columns of the row-major n x S matrix z and (grads non-null) their gradients in element e at point p: the
// basis once, then the columns (the block * S values of an element are one contiguous run).  p need not lie inside e.
template <int DIM, int K>
MGB_HD void eval_in_element(const BinsView& B, int e, const double* p, int S, const double* z, double* vals, double* grads) {
  double r[DIM];
  ref_coords<DIM>(B.x, B.block, e, p, r);
  ElemBasis<DIM, K> E;
  E.init(B.x, B.block, e, r);
  const double* ze = z + (size_t)e * B.block * S;
  for (int s = 0; s < S; ++s) {
    double g[DIM];
    E.template eval<false>(ze, nullptr, S, s, vals[s], g);
    if (grads) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) grads[DIM * s + d] = g[d];
    }
  }
}

// One query point: find its element, evaluate there.  vals: S values; grads (nullable): S x DIM; elem (nullable): one int.
template <int DIM, int K>
MGB_HD void eval_point(const BinsView& B, const double* p, int S, const double* z, double* vals, double* grads,
                       int32_t* elem) {
  const int found = find_element<DIM>(B, p);
  if (elem) *elem = found;
  if (found < 0) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int s = 0; s < S; ++s) vals[s] = nan;
    if (grads)
      for (int s = 0; s < S * DIM; ++s) grads[s] = nan;
    return;
  }
  eval_in_element<DIM, K>(B, found, p, S, z, vals, grads);
}

// ---------------------------------------------------------------------------------------------------- host setup
// The locator: a uniform bin grid over the bounding box of the nodes, roughly one cell per element, CSR cell -> elements.
// Built from x, dim, block and n alone (no refinement order), for 1, 2 and 3 dimensions by the same code.
struct Locator {
  int dim = 0, block = 0, n = 0, nel = 0, k = 0;      // k: degree of the tensor elements (0 in 2-D)
  int nc[3] = {1, 1, 1};
  double lo[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
  double min_extent = 0.0;      // the smallest element extent: the largest side of an element's bounding box (flowline.hpp's default step)
  std::vector<int> cellptr, cellelem;
  BinsView view(const int* ptr, const int* el, const double* x) const {
    BinsView B;
    B.nel = nel;
    B.block = block;
    for (int d = 0; d < 3; ++d) {
      B.nc[d] = nc[d];
      B.lo[d] = lo[d];
      B.inv[d] = inv[d];
    }
    B.cellptr = ptr;
    B.cellelem = el;
    B.x = x;
    return B;
  }
};

// the elements must be what the inverse maps assume
inline void validate_elements(const GeometryHost& g, int k) {
  const int dim = g.dim, block = g.block, nel = g.n / g.block;
  const double* x = g.x.data();
  for (int e = 0; e < nel; ++e) {
    const double* v = x + (size_t)e * block * dim;
    if (dim == 2) {
      const double ax = v[2] - v[0], ay = v[3] - v[1], bx = v[4] - v[0], by = v[5] - v[1];
      const double diam = std::max(std::max(std::fabs(ax), std::fabs(ay)), std::max(std::fabs(bx), std::fabs(by)));
      if (!(std::fabs(ax * by - ay * bx) > 1e-14 * diam * diam))
        throw ArgError("locator: degenerate triangle " + std::to_string(e));
      const int ea[3] = {0, 1, 2}, eb[3] = {1, 2, 0};
      for (int d = 0; d < 2; ++d) {
        bool ok = true;
        for (int i = 0; i < 3; ++i) ok = ok && std::fabs(v[2 * (3 + i) + d] - 0.5 * (v[2 * ea[i] + d] + v[2 * eb[i] + d])) <= 1e-10 * diam;
        ok = ok && std::fabs(v[12 + d] - (v[d] + v[2 + d] + v[4 + d]) / 3.0) <= 1e-10 * diam;
        if (!ok) throw ArgError("locator: rows 3..6 of element " + std::to_string(e) + " are not the edge midpoints and the centroid of rows 0..2");
      }
    } else {
      const double* b = v + (size_t)(block - 1) * dim;
      double diam = 0.0;
      for (int d = 0; d < dim; ++d) diam = std::max(diam, std::fabs(b[d] - v[d]));
      for (int d = 0; d < dim; ++d)
        if (!(std::fabs(b[d] - v[d]) > 1e-14 * diam)) throw ArgError("locator: degenerate element " + std::to_string(e));
      const int m1 = k + 1;
      for (int q = 0; q < block; ++q) {
        int idx[3] = {q % m1, (q / m1) % m1, q / (m1 * m1)};
        for (int d = 0; d < dim; ++d) {
          const double want = v[d] + (b[d] - v[d]) * ((double)idx[d] / k);
          if (!(std::fabs(v[(size_t)q * dim + d] - want) <= 1e-10 * diam))
            throw ArgError("locator: the nodes of element " + std::to_string(e) + " are not the tensor grid of its corner box");
        }
      }
    }
  }
}

inline Locator build_locator(const GeometryHost& g) {
  Locator L;
  if (g.dim < 1 || g.dim > 3 || g.n <= 0 || g.x.size() != (size_t)g.n * g.dim) throw ArgError("locator: bad geometry");
  const int dim = g.dim;
  int k = 0;
  if (dim == 1) {
    if (g.block != 2) throw ArgError("locator: 1-D elements must have 2 nodes");
    k = 1;
  } else if (dim == 2) {
    if (g.block != 7) throw ArgError("locator: 2-D elements must have 7 nodes");
  } else {
    k = g.block == 8 ? 1 : g.block == 27 ? 2 : g.block == 64 ? 3 : 0;
    if (!k) throw ArgError("locator: 3-D elements must have (k+1)^3 nodes, k = 1..3");
  }
  if (g.n % g.block != 0) throw ArgError("locator: n is not a multiple of the element size");
  const double* x = g.x.data();
  for (size_t i = 0; i < g.x.size(); ++i)
    if (!finite(x[i])) throw ArgError("locator: non-finite node coordinate");
  L.dim = dim;
  L.block = g.block;
  L.n = g.n;
  L.nel = g.n / g.block;
  L.k = k;
  validate_elements(g, k);
  L.min_extent = std::numeric_limits<double>::infinity();
  for (int e = 0; e < L.nel; ++e) {
    const double* v = x + (size_t)e * L.block * dim;
    double ext = 0.0;
    for (int d = 0; d < dim; ++d) {
      double bl = v[d], bh = v[d];
      for (int q = 1; q < L.block; ++q) {
        bl = std::min(bl, v[(size_t)q * dim + d]);
        bh = std::max(bh, v[(size_t)q * dim + d]);
      }
      ext = std::max(ext, bh - bl);
    }
    L.min_extent = std::min(L.min_extent, ext);
  }
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, amax = 0.0;
  for (int d = 0; d < dim; ++d) lo[d] = hi[d] = x[d];
  for (int q = 0; q < g.n; ++q)
    for (int d = 0; d < dim; ++d) {
      const double v = x[(size_t)q * dim + d];
      lo[d] = std::min(lo[d], v);
      hi[d] = std::max(hi[d], v);
      amax = std::max(amax, std::fabs(v));
    }
  // roughly one cell per element: cubic cells of the volume of an average element, then halve the longest axis while the
  // grid has more than twice as many cells as there are elements (flat or thin boxes)
  double vol = 1.0;
  for (int d = 0; d < dim; ++d) {
    if (!(hi[d] > lo[d])) throw ArgError("locator: the nodes span no volume");
    vol *= hi[d] - lo[d];
  }
  const double h = std::pow(vol / L.nel, 1.0 / dim);
  long long cells = 1;
  for (int d = 0; d < dim; ++d) {
    const double c = std::floor((hi[d] - lo[d]) / h + 0.5);
    L.nc[d] = (int)std::min(std::max(c, 1.0), 1048576.0);
    cells *= L.nc[d];
  }
  while (cells > 2LL * L.nel + 1) {
    int big = 0;
    for (int d = 1; d < dim; ++d)
      if (L.nc[d] > L.nc[big]) big = d;
    if (L.nc[big] == 1) break;
    cells /= L.nc[big];
    L.nc[big] = (L.nc[big] + 1) / 2;
    cells *= L.nc[big];
  }
  for (int d = 0; d < dim; ++d) {
    L.lo[d] = lo[d];
    L.inv[d] = L.nc[d] / (hi[d] - lo[d]);
  }
  // cell range of every element's bounding box grown by the tolerance: tau is a reference-coordinate tolerance, i.e. at most
  // tau * diameter in physical units; 1e-9 * diameter plus the rounding of the coordinates covers it with room
  auto range = [&](int e, int* c0, int* c1) {
    const double* v = x + (size_t)e * L.block * dim;
    double bl[3], bh[3], diam = 0.0;
    for (int d = 0; d < dim; ++d) bl[d] = bh[d] = v[d];
    for (int q = 1; q < L.block; ++q)
      for (int d = 0; d < dim; ++d) {
        bl[d] = std::min(bl[d], v[(size_t)q * dim + d]);
        bh[d] = std::max(bh[d], v[(size_t)q * dim + d]);
      }
    for (int d = 0; d < dim; ++d) diam = std::max(diam, bh[d] - bl[d]);
    const double eps = 1e-9 * diam + 1e-14 * amax;
    for (int d = 0; d < 3; ++d) c0[d] = c1[d] = 0;
    for (int d = 0; d < dim; ++d) {
      c0[d] = cell_coord(bl[d] - eps, L.lo[d], L.inv[d], L.nc[d]);
      c1[d] = cell_coord(bh[d] + eps, L.lo[d], L.inv[d], L.nc[d]);
    }
  };
  std::vector<size_t> count((size_t)cells + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    for (int e = 0; e < L.nel; ++e) {
      int c0[3], c1[3];
      range(e, c0, c1);
      for (int cz = c0[2]; cz <= c1[2]; ++cz)
        for (int cy = c0[1]; cy <= c1[1]; ++cy)
          for (int cx = c0[0]; cx <= c1[0]; ++cx) {
            const size_t cell = cx + (size_t)L.nc[0] * (cy + (size_t)L.nc[1] * cz);
            if (pass == 0) ++count[cell + 1];
            else L.cellelem[count[cell]++] = e;      // e ascending: every list comes out ascending
          }
    }
    if (pass == 0) {
      for (size_t c = 0; c < (size_t)cells; ++c) count[c + 1] += count[c];
      if (count[cells] > (size_t)INT_MAX) throw ArgError("locator: bin lists too long");
      L.cellptr.resize((size_t)cells + 1);
      for (size_t c = 0; c <= (size_t)cells; ++c) L.cellptr[c] = (int)count[c];
      L.cellelem.resize(count[cells]);
      count.assign(L.cellptr.begin(), L.cellptr.end());
    }
  }
  return L;
}

// f.template operator()<DIM, K>() for the element kind of the locator
template <class F>
inline void dispatch(int dim, int k, F&& f) {
  if (dim == 1) f.template operator()<1, 1>();
  else if (dim == 2) f.template operator()<2, 0>();
  else if (k == 1) f.template operator()<3, 1>();
  else if (k == 2) f.template operator()<3, 2>();
  else if (k == 3) f.template operator()<3, 3>();
  else throw InternalError("interp: unknown element kind");
}

struct HostEval {
  BinsView B;
  int m, S;
  const double *pts, *z;
  double *vals, *grads;
  int32_t* elem;
  template <int DIM, int K>
  void operator()() const {
    for (int q = 0; q < m; ++q)
      eval_point<DIM, K>(B, pts + (size_t)q * DIM, S, z, vals + (size_t)q * S, grads ? grads + (size_t)q * S * DIM : nullptr,
                         elem ? elem + q : nullptr);
  }
};

// host restatement: the same bins, containment rule and bases, no GPU
inline void interpolate_host(const Locator& L, const double* x, int m, const double* pts, int S, const double* z, double* vals,
                             double* grads, int32_t* elem) {
  HostEval ev{L.view(L.cellptr.data(), L.cellelem.data(), x), m, S, pts, z, vals, grads, elem};
  dispatch(L.dim, L.k, ev);
}

#if defined(__HIPCC__)
// interp.hip: one thread per query point on `stream`; all pointers are device pointers, grads / elem may be null
void launch_interpolate(hipStream_t stream, const BinsView& B, int dim, int k, int m, const double* pts, int S, const double* z,
                        double* vals, double* grads, int32_t* elem);
#endif

}  // namespace interp
}  // namespace mgb
