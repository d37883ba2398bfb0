// Boundary facets of a geometry and boundary integrals of p-Laplace solutions: the facet list, built
// ONCE per geometry on the host, and what ONE facet node contributes, written ONCE.  The gfx950 kernels (boundary.hip) and the
// host restatement (mgb_geo_boundary_flux_host) both run Node below; sigma is energy.hpp's Node::flux, combine is reduce.hpp's.
//   The elements are broken and their quadrature is nodal: every node of a boundary facet is a row of x and z already, so a
//   boundary rule is a list of (row, weight) pairs per facet plus the facet's outward unit normal.
//   A facet of an element is a BOUNDARY facet when the sorted tuple of the continuous dofs (subspaces["full"][L-1], one entry 1
//   per row) of its corner nodes occurs in exactly one element.  Facets come in ascending (element, local facet) order.
//     1-D: local facets = local nodes 0, 1; q = 1; weight 1; normal sign(x - element centre).
//     2-D: edge i = (v_i, m_{i,i+1}, v_{i+1}) = local rows i, 3 + i, (i + 1) % 3; q = 3; Simpson |e| (1/6, 4/6, 1/6); the normal is
//          perpendicular to v_a -> v_b with n . (edge midpoint - centroid of the own triangle) > 0.
//     3-D: x-, x+, y-, y+, z-, z+; the (k+1)^2 nodes of the side in ascending local index; face area times the tensor of the
//          closed Newton-Cotes weights of degree k (fem3d_native's); normal +- the axis by sign(face coordinate - element centre).
//   At facet node j of facet f, row i = nodes[f q + j], for a field z (n x S row-major):
//     sigma = |grad u|^(p-2) grad u in i's own element (energy::Node::init + flux),  sn = sigma . n,  t = sigma - sn n.
//   Five contributions: omega sn | omega u_i | omega | |sn| | |t|_2   (three sums, two NaN-sticky maxima).
//   A non-finite u_i or sigma, or an exponent that is not a finite real >= 1, makes all five NaN.  A facet left out by the mask
//   contributes nothing; its per-facet value is 0.  The per-facet value is the sum of omega sn over j = 0..q-1 in that order.
//   The same key sort also gives the INTERIOR facets (exactly two elements) and the element -> facet table of the error
//   indicators (estimate.hpp): struct Interior below.
// The arithmetic of Node::contributions is kept as written (fp contract off), as energy.hpp's is.
#pragma once
#include <array>

#include "energy.hpp"

namespace mgb {
namespace boundary {

using namespace reduce;      // kCols (MGB_BOUNDARY_COLS), kThreads, combine

// the facet list of one geometry, on the host
struct Facets {
  int dim = 0, k = 0, q = 0, nf = 0;
  std::vector<int> element;        // nf
  std::vector<int> nodes;          // nf x q global rows
  std::vector<double> weights;     // nf x q
  std::vector<double> normal;      // nf x dim outward unit normals
  std::vector<double> measure;     // nf
  std::vector<double> centre;      // nf x dim
};

// what all fields of one call share
struct Args {
  energy::Args E;                          // geometry, exponent, the table of fields, S and u (s, f unused)
  const int* nodes = nullptr;              // nf x q
  const double* weights = nullptr;         // nf x q
  const double* normal = nullptr;          // nf x dim
  const unsigned char* mask = nullptr;     // nf bytes or null: 0 leaves the facet out
  int nf = 0, q = 0;
};

// all five columns are sums of, or maxima over, non-negative or signed terms whose empty value is 0: an empty or wholly masked
// facet list gives zeros, not reduce::identity's -inf, which this hides
MGB_HD void identity(double* c) { c[0] = c[1] = c[2] = c[3] = c[4] = 0.0; }

template <int DIM, int K>
struct Node {
  // the five contributions of facet node j of facet f for the field z
  MGB_HD static void contributions(const Args& A, const double* z, int f, int j, double* c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int i = A.nodes[(size_t)f * A.q + j];
    const double om = A.weights[(size_t)f * A.q + j];
    const double* n = A.normal + (size_t)f * DIM;
    energy::Node<DIM, K> N;
    N.init(A.E, i);
    double sigma[DIM];
    N.flux(z, A.E.S, A.E.u, sigma);
    const double ui = z[(size_t)i * A.E.S + A.E.u];
    double sn = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) sn += sigma[k] * n[k];
    double ts = 0.0;
    bool good = N.p >= 1.0;
    good = good & interp::finite(N.p);
    good = good & interp::finite(ui);
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const double t = sigma[k] - sn * n[k];
      ts += t * t;
      good = good & interp::finite(sigma[k]);
    }
    if (!good) {
      c[0] = c[1] = c[2] = c[3] = c[4] = std::numeric_limits<double>::quiet_NaN();
      return;
    }
    c[0] = om * sn;
    c[1] = om * ui;
    c[2] = om;
    c[3] = fabs(sn);
    c[4] = sqrt(ts);
  }
};

// host restatement: the same per-node routine, serially, field after field in ascending (facet, facet node) order
struct HostFlux {
  Args A;
  double* out;          // B x kCols
  double* facets;       // B x nf or null
  template <int DIM, int K>
  void operator()() const {
    for (int b = 0; b < A.E.B; ++b) {
      double* acc = out + (size_t)b * kCols;
      identity(acc);
      for (int f = 0; f < A.nf; ++f) {
        double fsum = 0.0;
        if (!A.mask || A.mask[f])
          for (int j = 0; j < A.q; ++j) {
            double c[kCols];
            Node<DIM, K>::contributions(A, A.E.z[b], f, j, c);
            combine(acc, c);
            fsum += c[0];
          }
        if (facets) facets[(size_t)b * A.nf + f] = fsum;
      }
    }
  }
};

inline void boundary_flux_host(int dim, int k, const Args& A, double* out, double* facets) {
  HostFlux h{A, out, facets};
  interp::dispatch(dim, k, h);
}

// ---------------------------------------------------------------------------------------------------- host setup
// continuous dof of every row from subspaces["full"][L-1]
inline std::vector<int> continuous_dofs(const GeometryHost& g) {
  auto it = g.subspaces.find("full");
  if (it == g.subspaces.end() || g.L < 1 || (int)it->second.size() < g.L)
    throw ArgError("boundary: the geometry has no full subspace");
  const Csr& F = it->second[g.L - 1];
  if (F.rows != g.n || (int)F.rowptr.size() != g.n + 1) throw ArgError("boundary: the finest full subspace must have one row per node");
  std::vector<int> dof((size_t)g.n);
  for (int r = 0; r < g.n; ++r) {
    if (F.rowptr[r + 1] - F.rowptr[r] != 1 || F.vals[F.rowptr[r]] != 1.0)
      throw ArgError("boundary: the finest full subspace must have exactly one entry of value 1 per row");
    dof[r] = F.colidx[F.rowptr[r]];
  }
  return dof;
}

// local rows of local facet lf in ascending local index, and the positions (within them) of its corner nodes
inline void local_facet(int dim, int k, int lf, std::vector<int>& rows, std::vector<int>& corners) {
  rows.clear();
  corners.clear();
  if (dim == 1) {
    rows = {lf};
    corners = {0};
  } else if (dim == 2) {
    rows = {lf, 3 + lf, (lf + 1) % 3};
    corners = {0, 2};
  } else {
    const int m1 = k + 1, axis = lf / 2, fixed = (lf & 1) ? k : 0;
    for (int b = 0; b < m1; ++b)
      for (int a = 0; a < m1; ++a) {      // a runs along the lower of the two free axes: ascending local index
        int idx[3];
        idx[axis] = fixed;
        idx[axis == 0 ? 1 : 0] = a;
        idx[axis == 2 ? 1 : 2] = b;
        if ((a == 0 || a == k) && (b == 0 || b == k)) corners.push_back((int)rows.size());
        rows.push_back(idx[0] + m1 * (idx[1] + m1 * idx[2]));
      }
  }
}

// weights (q), outward unit normal (dim, zeroed by the caller), measure and centre (dim) of local facet lf of element e
inline void facet_geometry(const GeometryHost& g, int dim, int k, int block, int e, int lf, const std::vector<int>& rows, double* w,
                           double* n, double* c, double& measure) {
  const double nc[3][4] = {{0.5, 0.5, 0, 0}, {1.0 / 6, 4.0 / 6, 1.0 / 6, 0}, {1.0 / 8, 3.0 / 8, 3.0 / 8, 1.0 / 8}};      // fem3d_native's
  const double* xe = g.x.data() + (size_t)e * block * dim;
  if (dim == 2) {
    const double* a = xe + 2 * rows[0];
    const double* m = xe + 2 * rows[1];
    const double* b = xe + 2 * rows[2];
    const double dx = b[0] - a[0], dy = b[1] - a[1], len = std::sqrt(dx * dx + dy * dy);
    const double cx = (xe[0] + xe[2] + xe[4]) / 3.0, cy = (xe[1] + xe[3] + xe[5]) / 3.0;
    n[0] = dy / len, n[1] = -dx / len;
    if (n[0] * (m[0] - cx) + n[1] * (m[1] - cy) < 0.0) n[0] = -n[0], n[1] = -n[1];
    w[0] = len * (1.0 / 6), w[1] = len * (4.0 / 6), w[2] = len * (1.0 / 6);
    measure = len;
    c[0] = m[0], c[1] = m[1];
  } else {
    const double* lo = xe;                                   // first and last row: opposite corners of the box, in either order
    const double* hi = xe + (size_t)(block - 1) * dim;
    const int axis = dim == 1 ? 0 : lf / 2;
    const double* p = xe + (size_t)rows[0] * dim;            // a node of the facet: it carries the facet coordinate
    double area = 1.0;
    for (int d = 0; d < dim; ++d) {
      c[d] = d == axis ? p[d] : 0.5 * (lo[d] + hi[d]);
      if (d != axis) area *= std::fabs(hi[d] - lo[d]);
    }
    n[axis] = p[axis] > 0.5 * (lo[axis] + hi[axis]) ? 1.0 : -1.0;
    measure = area;
    if (dim == 1) {
      w[0] = 1.0;
    } else {
      const int m1 = k + 1;
      for (int b = 0; b < m1; ++b)
        for (int a = 0; a < m1; ++a) w[a + m1 * b] = area * (nc[k - 1][a] * nc[k - 1][b]);
    }
  }
}

// The interior facets of one geometry, on the host: a facet whose sorted corner dofs occur in exactly
// two elements.  The first side is the one with the smaller (element, local facet); facets come in ascending (element, local
// facet) order of their first side.  Weights, measure, centre and normal are those of the first side (the formulas of the
// boundary facets), the normal pointing out of it.  nodes holds the q rows of the first side in local_facet order, then the q
// rows of the second side permuted so that node j of both sides has the same continuous dof.  elem_facet (nel x nlf): the
// interior facet of (element, local facet), or -1 - f for boundary facet f -- every local facet is one or the other.
struct Interior {
  int dim = 0, k = 0, q = 0, nif = 0, nel = 0, nlf = 0;
  std::vector<int> elements;       // nif x 2
  std::vector<int> nodes;          // nif x 2 x q global rows
  std::vector<double> weights;     // nif x q
  std::vector<double> normal;      // nif x dim, out of the first side
  std::vector<double> measure;     // nif
  std::vector<double> centre;      // nif x dim
  std::vector<int> elem_facet;     // nel x nlf
};

// one key sort for both lists; each output is nullable
inline void build_facet_lists(const GeometryHost& g, Facets* Fout, Interior* Iout) {
  const interp::Locator L = interp::build_locator(g);      // validates x, dim, block and the shape of every element
  const std::vector<int> dof = continuous_dofs(g);
  const int dim = L.dim, k = L.k, block = L.block, nel = L.nel;
  const int nlf = dim == 1 ? 2 : dim == 2 ? 3 : 6;
  const int q = dim == 1 ? 1 : dim == 2 ? 3 : (k + 1) * (k + 1);
  std::vector<std::vector<int>> rows(nlf), corners(nlf);
  for (int lf = 0; lf < nlf; ++lf) local_facet(dim, k, lf, rows[lf], corners[lf]);
  // (sorted corner dofs, element, local facet), sorted: facets with the same dofs are neighbours
  struct Key {
    std::array<int, 4> d;
    int e, lf;
  };
  std::vector<Key> keys;
  keys.reserve((size_t)nel * nlf);
  for (int e = 0; e < nel; ++e)
    for (int lf = 0; lf < nlf; ++lf) {
      Key key{{-1, -1, -1, -1}, e, lf};
      for (size_t c = 0; c < corners[lf].size(); ++c) key.d[c] = dof[(size_t)e * block + rows[lf][corners[lf][c]]];
      std::sort(key.d.begin(), key.d.end());
      keys.push_back(key);
    }
  std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) {
    if (a.d != b.d) return a.d < b.d;
    return a.e != b.e ? a.e < b.e : a.lf < b.lf;
  });
  std::vector<std::pair<int, int>> bnd;                          // (element, local facet)
  std::vector<std::array<int, 4>> pairs;                         // (element, local facet) of the first side, then of the second
  for (size_t i = 0; i < keys.size();) {
    size_t j = i + 1;
    while (j < keys.size() && keys[j].d == keys[i].d) ++j;
    if (j - i > 2) throw ArgError("boundary: a facet is shared by more than two elements (non-manifold mesh)");
    if (j - i == 2 && keys[i].e == keys[i + 1].e) throw ArgError("boundary: two facets of one element share their corner dofs");
    if (j - i == 1) bnd.emplace_back(keys[i].e, keys[i].lf);
    else pairs.push_back({keys[i].e, keys[i].lf, keys[i + 1].e, keys[i + 1].lf});      // the sort put the smaller side first
    i = j;
  }
  std::sort(bnd.begin(), bnd.end());
  std::sort(pairs.begin(), pairs.end());
  if (Fout) {
    Facets& F = *Fout;
    F = Facets();
    F.dim = dim, F.k = k, F.q = q, F.nf = (int)bnd.size();
    F.element.resize(F.nf);
    F.nodes.resize((size_t)F.nf * q);
    F.weights.resize((size_t)F.nf * q);
    F.normal.assign((size_t)F.nf * dim, 0.0);
    F.measure.resize(F.nf);
    F.centre.resize((size_t)F.nf * dim);
    for (int f = 0; f < F.nf; ++f) {
      const int e = bnd[f].first, lf = bnd[f].second;
      F.element[f] = e;
      for (int j = 0; j < q; ++j) F.nodes[(size_t)f * q + j] = e * block + rows[lf][j];
      facet_geometry(g, dim, k, block, e, lf, rows[lf], F.weights.data() + (size_t)f * q, F.normal.data() + (size_t)f * dim,
                     F.centre.data() + (size_t)f * dim, F.measure[f]);
    }
  }
  if (Iout) {
    Interior& I = *Iout;
    I = Interior();
    I.dim = dim, I.k = k, I.q = q, I.nif = (int)pairs.size(), I.nel = nel, I.nlf = nlf;
    I.elements.resize((size_t)I.nif * 2);
    I.nodes.resize((size_t)I.nif * 2 * q);
    I.weights.resize((size_t)I.nif * q);
    I.normal.assign((size_t)I.nif * dim, 0.0);
    I.measure.resize(I.nif);
    I.centre.resize((size_t)I.nif * dim);
    I.elem_facet.assign((size_t)nel * nlf, INT_MIN);
    for (int f = 0; f < (int)bnd.size(); ++f) I.elem_facet[(size_t)bnd[f].first * nlf + bnd[f].second] = -1 - f;
    std::vector<char> used((size_t)q);
    for (int f = 0; f < I.nif; ++f) {
      const int ea = pairs[f][0], la = pairs[f][1], eb = pairs[f][2], lb = pairs[f][3];
      I.elements[2 * (size_t)f] = ea, I.elements[2 * (size_t)f + 1] = eb;
      I.elem_facet[(size_t)ea * nlf + la] = f;
      I.elem_facet[(size_t)eb * nlf + lb] = f;
      int* na = I.nodes.data() + (size_t)f * 2 * q;
      int* nb = na + q;
      std::fill(used.begin(), used.end(), 0);
      for (int j = 0; j < q; ++j) {
        na[j] = ea * block + rows[la][j];
        int hit = -1;
        for (int t = 0; t < q && hit < 0; ++t)
          if (!used[t] && dof[(size_t)eb * block + rows[lb][t]] == dof[na[j]]) hit = t;
        if (hit < 0) throw ArgError("boundary: the two sides of an interior facet cannot be matched node by node");
        used[hit] = 1;
        nb[j] = eb * block + rows[lb][hit];
      }
      facet_geometry(g, dim, k, block, ea, la, rows[la], I.weights.data() + (size_t)f * q, I.normal.data() + (size_t)f * dim,
                     I.centre.data() + (size_t)f * dim, I.measure[f]);
    }
    for (size_t t = 0; t < I.elem_facet.size(); ++t)
      if (I.elem_facet[t] == INT_MIN) throw InternalError("boundary: a local facet is neither interior nor on the boundary");
  }
}

inline Facets build_facets(const GeometryHost& g) {
  Facets F;
  build_facet_lists(g, &F, nullptr);
  return F;
}

inline Interior build_interior(const GeometryHost& g) {
  Interior I;
  build_facet_lists(g, nullptr, &I);
  return I;
}

// facets per workgroup (a facet never straddles two workgroups), workgroups per field, doubles of scratch of the two launches
// and where the finish leaves its results in them
inline int facets_per_workgroup(int q) { return kThreads / q; }
inline long long workgroups(int nf, int q) {
  const int fpw = facets_per_workgroup(q);
  return nf > 0 ? ((long long)nf + fpw - 1) / fpw : 1;
}
inline size_t scratch_doubles(int nf, int q, int B) { return (size_t)(workgroups(nf, q) + 1) * B * kCols; }      // partials, then B x kCols results
inline size_t results_offset(int nf, int q, int B) { return (size_t)workgroups(nf, q) * B * kCols; }

// ---------------------------------------------------------------------------------------------------- Neumann load
//   The objective is sum_i w_i c_i . (Dz)_i, so  int_Gamma h u ds  adds
//     l_i = (sum over the facet nodes (f, j) with row(f, j) = i of  omega_fj h_fj) / w_i
// to the (u, id) column of c at the boundary rows.  A row can sit in several facets of its own element (a triangle with two
// boundary edges: 2; a cube corner: 3), so the facet list carries a row-sorted incidence table, built once on the host:
//   rows   the nb distinct rows of the facet nodes, ascending
//   start  nb + 1 row starts into idx
//   idx    facet-node indices f q + j, ascending within a row
// load_row below is the contract, run by boundary_load_kernel (boundary.hip) and by the host restatement: for boundary row r add
// omega h over its incidences in table order, skipping the facets the mask leaves out -- their h is not read, so a NaN there
// is not seen -- then divide once by w_r; a row with no selected incidence gives exactly 0.  Arithmetic kept as written (fp
// contract off).
struct Incidence {
  std::vector<int> rows, start, idx;
  int nb() const { return (int)rows.size(); }
};

inline Incidence build_incidence(const Facets& F) {
  const size_t m = (size_t)F.nf * F.q;
  std::vector<std::pair<int, int>> pairs(m);      // (row, facet node)
  for (size_t t = 0; t < m; ++t) pairs[t] = {F.nodes[t], (int)t};
  std::sort(pairs.begin(), pairs.end());
  Incidence I;
  I.idx.resize(m);
  for (size_t t = 0; t < m; ++t) {
    if (t == 0 || pairs[t].first != pairs[t - 1].first) {
      I.rows.push_back(pairs[t].first);
      I.start.push_back((int)t);
    }
    I.idx[t] = pairs[t].second;
  }
  I.start.push_back((int)m);
  return I;
}

struct LoadArgs {
  const int* rows = nullptr;               // nb
  const int* start = nullptr;              // nb + 1
  const int* idx = nullptr;                // nf x q facet nodes, grouped by row
  const double* weights = nullptr;         // nf x q
  const unsigned char* mask = nullptr;     // nf bytes or null: 0 leaves the facet out
  const double* w = nullptr;               // n nodal weights
  int nb = 0, nf = 0, q = 0;
};

// the load of boundary row r for one field h (nf x q)
MGB_HD double load_row(const LoadArgs& A, const double* h, int r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double s = 0.0;
  bool any = false;
  const int t1 = A.start[r + 1];
  for (int t = A.start[r]; t < t1; ++t) {
    const int fj = A.idx[t];
    if (A.mask && !A.mask[fj / A.q]) continue;
    s += A.weights[fj] * h[fj];
    any = true;
  }
  return any ? s / A.w[A.rows[r]] : 0.0;
}

// host restatement: out is B x nb, h is B x nf x q
inline void boundary_load_host(const LoadArgs& A, int B, const double* h, double* out) {
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < A.nb; ++r) out[(size_t)b * A.nb + r] = load_row(A, h + (size_t)b * A.nf * A.q, r);
}

#if defined(__HIPCC__)
// boundary.hip: boundary_load_kernel on grid (ceil(nb / 256), B), one thread per distinct row, compact output B x nb; all
// pointers of A, h and out are device pointers
void launch_boundary_load(hipStream_t stream, const LoadArgs& A, int B, const double* h, double* out);
// y[rows[j] * stride + offset] += alpha * load[j], one thread per j < nb (rows are distinct: no conflicts)
void launch_boundary_load_add(hipStream_t stream, int nb, const int* rows, const double* load, double alpha, long long stride,
                              long long offset, double* y);
// boundary.hip: two launches on `stream` -- partials on grid (workgroups, B), one thread per (facet, facet node), then the
// finish of reduce.hpp, one workgroup per field; all pointers of A are device pointers (A.E.z a device table of B device
// pointers); the B x kCols results are at scratch + results_offset; facet_flux
// (nullable): B x nf device doubles
void launch_boundary_flux(hipStream_t stream, int dim, int k, const Args& A, double* scratch, double* facet_flux);
#endif

}  // namespace boundary
}  // namespace mgb
