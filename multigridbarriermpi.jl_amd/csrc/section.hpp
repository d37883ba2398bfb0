// Plane sections of nodal fields: what ONE item contributes to the cut of a field by a plane
// n . x = c, written ONCE.  The gfx950 kernels (section.hip) and the host restatement (mgb_geo_sections_host) both run item()
// below.  The marching rule is the level sets' and the isosurfaces', applied to the side function d(x) = n . x - c instead of
// a nodal field: levelset::crossing, isosurface::pick / triangle / kKuhn; value and gradient at a point of a known element
// are flowline::value_grad (interp::ElemBasis, no locator); the flux follows the case distinctions of energy::Node::flux;
// combine, block_reduce and the identity NoItems are reduce.hpp's and levelset.hpp's.  The full rule is the comment of
// mgb_geo_sections in include/mgb_hip.h; in short:
//   2-D (block 7): one item per element, corners = local rows 0, 1, 2; the cut is the segment between the crossings on the
//     two edges at the lone corner, the above side (d > 0) on its left; 4-point Gauss-Legendre on it (u is a cubic there).
//   3-D (block (k+1)^3): item = e 6 + t, the box of the eight corner nodes cut into the six Kuhn tetrahedra; one triangle
//     (one or three corners above) or two (two above), (P1 - P0) x (P2 - P0) towards the below side; the collapsed tensor
//     Gauss-Legendre rule with n_K x n_K points, n_K = 3, 4, 6 for k = 1, 2, 3 (exact for degree 2 n_K - 2 >= 3 k).
//   Five contributions: sum w | sum w v | sum w (sigma . nu) | max v | max (-v), sigma = |g|^(p-2) g, nu = n / |n|.
//   An item the plane does not cut reads no field value and contributes the identity (0, 0, 0, -inf, -inf).
// The arithmetic is kept as written by ONE mechanism: section.hip, which holds the kernels AND the host restatement and is
// the only file that may instantiate item(), is compiled with -ffp-contract=off (build.sh).
#pragma once
#include <cstdint>
#include <string>

#include "flowline.hpp"
#include "isosurface.hpp"

namespace mgb {
namespace section {

using levelset::kCols;
using levelset::kThreads;
using levelset::kWaves;
using levelset::nanmax;
using levelset::no_items;
using levelset::NoItems;
using levelset::workgroups;

// what all rows of one call share; every pointer is a host pointer or every pointer is a device pointer
struct Args {
  interp::BinsView own;                 // the geometry: x and block (its bins are not used)
  const double* const* z = nullptr;     // B pointers to n x S fields
  const double* planes = nullptr;       // nc rows (n_0 .. n_{dim-1}, c)
  double p = 2.0;                       // the exponent of sigma = |g|^(p-2) g
  long long items = 0;                  // items per (field, plane)
  int nel = 0, S = 0, u = 0, B = 0, nc = 0;
};

// items of one (field, plane) row: nel in 2-D, 6 nel in 3-D
inline long long items_per_row(int dim, int nel) { return dim == 2 ? (long long)nel : 6LL * nel; }
// doubles of a piece row: x0 y0 x1 y1 | u0 u1, or the nine coordinates of a triangle | u0 u1 u2
constexpr int piece_width(int dim) { return dim == 2 ? 6 : 12; }
// Gauss points per direction: 4 on a segment; 3, 4, 6 on a triangle of an element of degree 1, 2, 3
constexpr int gauss_points(int dim, int k) { return dim == 2 ? 4 : (k == 1 ? 3 : (k == 2 ? 4 : 6)); }

// Gauss-Legendre nodes and weights on [0, 1], rounded from 40 digits
template <int N>
struct Gauss;
template <>
struct Gauss<3> {
  static constexpr double x[3] = {0.11270166537925831, 0.5, 0.88729833462074169};
  static constexpr double w[3] = {0.27777777777777778, 0.44444444444444444, 0.27777777777777778};
};
template <>
struct Gauss<4> {
  static constexpr double x[4] = {0.069431844202973712, 0.33000947820757187, 0.66999052179242813, 0.93056815579702629};
  static constexpr double w[4] = {0.17392742256872693, 0.32607257743127307, 0.32607257743127307, 0.17392742256872693};
};
template <>
struct Gauss<6> {
  static constexpr double x[6] = {0.033765242898423986, 0.16939530676686774, 0.38069040695840155,
                                  0.61930959304159845,  0.83060469323313226, 0.96623475710157601};
  static constexpr double w[6] = {0.085662246189585173, 0.1803807865240693,  0.23395696728634552,
                                  0.23395696728634552,  0.1803807865240693,  0.085662246189585173};
};

// what one item gives: the five contributions and its `emit` = 0, 1 or 2 pieces, oriented, in the order of the rule
template <int DIM>
struct Term {
  double c[kCols];
  double piece[2][piece_width(DIM)];
  int emit;
};

template <int DIM>
MGB_HD void poison(Term<DIM>& T) {
  T.c[0] = T.c[1] = T.c[2] = T.c[3] = T.c[4] = std::numeric_limits<double>::quiet_NaN();
  T.emit = 0;
}

// sigma = a^(p-2) g for a finite p >= 1, by the case distinctions of energy::Node::flux: g itself at p = 2, g / a at p = 1,
// exactly 0 where a = 0
template <int DIM>
MGB_HD void sigma(const double* g, double p, double* s) {
  if (p == 2.0) {
#pragma unroll
    for (int k = 0; k < DIM; ++k) s[k] = g[k];
    return;
  }
  double gs = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) gs += g[k] * g[k];
  const double a = sqrt(gs);
  const bool one = p == 1.0;
  const double m = one ? 1.0 : pow(a, p - 2.0);
#pragma unroll
  for (int k = 0; k < DIM; ++k) s[k] = a == 0.0 ? 0.0 : (one ? g[k] / a : m * g[k]);
}

// d(x) = (n_0 x_0 + n_1 x_1 [+ n_2 x_2]) - c, summed in that order
template <int DIM>
MGB_HD double side(const double* plane, const double* x) {
  double s = plane[0] * x[0];
#pragma unroll
  for (int k = 1; k < DIM; ++k) s += plane[k] * x[k];
  return s - plane[DIM];
}

// nu = n / |n|
template <int DIM>
MGB_HD void unit_normal(const double* plane, double* nu) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < DIM; ++k) s += plane[k] * plane[k];
  const double a = sqrt(s);
#pragma unroll
  for (int k = 0; k < DIM; ++k) nu[k] = plane[k] / a;
}

// One quadrature point xq of element e with weight om: added to the three sums of the piece (pc) and to the two maxima of the
// item (c[3], c[4]); false where the value or the gradient is not finite.
template <int DIM, int K>
MGB_HD bool point(const Args& A, const double* z, int e, const double* nu, const double* xq, double om, double* pc, double* c) {
  double v, g[DIM], s[DIM];
  flowline::value_grad<DIM, K>(A.own, z, A.S, A.u, e, xq, v, g);
  bool good = interp::finite(v);
  good = good & flowline::all_finite<DIM>(g);
  sigma<DIM>(g, A.p, s);
  double sn = s[0] * nu[0];
#pragma unroll
  for (int k = 1; k < DIM; ++k) sn += s[k] * nu[k];
  pc[0] += om;
  pc[1] += om * v;
  pc[2] += om * sn;
  c[3] = nanmax(c[3], v);
  c[4] = nanmax(c[4], -v);
  return good;
}

// the value of element e's polynomial at q, a vertex of a piece
template <int DIM, int K>
MGB_HD double value_at(const Args& A, const double* z, int e, const double* q) {
  double v, g[DIM];
  flowline::value_grad<DIM, K>(A.own, z, A.S, A.u, e, q, v, g);
  return v;
}

// corner j of three by a select chain
struct Corner2 {
  double p[2], v;
};
MGB_HD Corner2 pick2(const Corner2* R, int j) {
  Corner2 o = R[0];
#pragma unroll
  for (int m = 1; m < 3; ++m) {
    const bool is = j == m;
    o.p[0] = is ? R[m].p[0] : o.p[0];
    o.p[1] = is ? R[m].p[1] : o.p[1];
    o.v = is ? R[m].v : o.v;
  }
  return o;
}

// 2-D: element `it` against the line `plane` = (n_0, n_1, c)
MGB_HD void item2d(const Args& A, const double* z, const double* plane, long long it, Term<2>& T) {
  const int e = (int)it;
  const double* xe = A.own.x + (size_t)e * 14;
  Corner2 R[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    R[m].p[0] = xe[2 * m];
    R[m].p[1] = xe[2 * m + 1];
    R[m].v = side<2>(plane, R[m].p);
  }
  no_items(T.c);
  T.emit = 0;
  const bool up[3] = {R[0].v > 0.0, R[1].v > 0.0, R[2].v > 0.0};
  const int k_above = (int)up[0] + (int)up[1] + (int)up[2];
  if (k_above == 0 || k_above == 3) return;
  // the lone corner: the one above (k_above = 1) or the one not above (k_above = 2)
  const bool one = k_above == 1;
  const int L = up[0] == one ? 0 : (up[1] == one ? 1 : 2), o1 = L == 2 ? 0 : L + 1, o2 = o1 == 2 ? 0 : o1 + 1;
  const Corner2 CL = pick2(R, L), C1 = pick2(R, o1), C2 = pick2(R, o2);
  double Q0[2], Q1[2];
  if (one) {
    levelset::crossing<2>(C1.p, C1.v, CL.p, CL.v, 0.0, Q0);
    levelset::crossing<2>(C2.p, C2.v, CL.p, CL.v, 0.0, Q1);
  } else {
    levelset::crossing<2>(CL.p, CL.v, C1.p, C1.v, 0.0, Q0);
    levelset::crossing<2>(CL.p, CL.v, C2.p, C2.v, 0.0, Q1);
  }
  if ((Q0[0] == Q1[0]) & (Q0[1] == Q1[1])) return;      // both end points are the same point: nothing is cut
  const double* above = one ? CL.p : C1.p;
  const bool swap = levelset::cross2(Q1[0] - Q0[0], Q1[1] - Q0[1], above[0] - Q0[0], above[1] - Q0[1]) < 0.0;
  const double S0[2] = {swap ? Q1[0] : Q0[0], swap ? Q1[1] : Q0[1]}, S1[2] = {swap ? Q0[0] : Q1[0], swap ? Q0[1] : Q1[1]};
  const double dx = S1[0] - S0[0], dy = S1[1] - S0[1];
  const double len = sqrt(dx * dx + dy * dy);
  double nu[2], pc[3] = {0.0, 0.0, 0.0};
  unit_normal<2>(plane, nu);
  bool good = true;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const double s = Gauss<4>::x[q];
    const double xq[2] = {S0[0] + s * dx, S0[1] + s * dy};
    good = good & point<2, 0>(A, z, e, nu, xq, Gauss<4>::w[q] * len, pc, T.c);
  }
  if (!good) {
    poison(T);
    return;
  }
  T.c[0] += pc[0];
  T.c[1] += pc[1];
  T.c[2] += pc[2];
  T.piece[0][0] = S0[0];
  T.piece[0][1] = S0[1];
  T.piece[0][2] = S1[0];
  T.piece[0][3] = S1[1];
  T.piece[0][4] = value_at<2, 0>(A, z, e, S0);
  T.piece[0][5] = value_at<2, 0>(A, z, e, S1);
  T.emit = 1;
}

// 3-D: Kuhn tetrahedron t of the box of element e, item = e 6 + t, against `plane` = (n_0, n_1, n_2, c)
template <int K>
MGB_HD void item3d(const Args& A, const double* z, const double* plane, long long it, Term<3>& T) {
  constexpr int M1 = K + 1, BLOCK = M1 * M1 * M1, NG = gauss_points(3, K);
  using isosurface::Corner;
  using isosurface::pick;
  const int t = (int)(it % 6), e = (int)(it / 6);
  const int code = (int)((isosurface::kKuhn >> (6 * t)) & 63ull);
  const int off[4] = {0, code & 7, code >> 3, 7};
  const double* xe = A.own.x + (size_t)e * BLOCK * 3;
  Corner R[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const size_t node = (size_t)(K * (off[m] & 1) + M1 * (K * ((off[m] >> 1) & 1) + M1 * (K * (off[m] >> 2))));
    R[m].p[0] = xe[3 * node];
    R[m].p[1] = xe[3 * node + 1];
    R[m].p[2] = xe[3 * node + 2];
    R[m].v = side<3>(plane, R[m].p);
  }
  no_items(T.c);
  T.emit = 0;
  const bool up[4] = {R[0].v > 0.0, R[1].v > 0.0, R[2].v > 0.0, R[3].v > 0.0};
  const int k_above = (int)up[0] + (int)up[1] + (int)up[2] + (int)up[3];
  if (k_above == 0 || k_above == 4) return;
  double tri[2][isosurface::kTriWidth] = {}, area[2] = {0.0, 0.0};
  int ntri;
  if (k_above != 2) {
    // the lone corner L: the one above (k_above = 1) or the one not above (k_above = 3); the others in ascending order
    const bool one = k_above == 1;
    const int L = up[0] == one ? 0 : (up[1] == one ? 1 : (up[2] == one ? 2 : 3));
    const Corner CL = pick(R, L), C1 = pick(R, L == 0 ? 1 : 0), C2 = pick(R, L <= 1 ? 2 : 1), C3 = pick(R, L == 3 ? 2 : 3);
    double Q1[3], Q2[3], Q3[3];
    if (one) {
      levelset::crossing<3>(C1.p, C1.v, CL.p, CL.v, 0.0, Q1);
      levelset::crossing<3>(C2.p, C2.v, CL.p, CL.v, 0.0, Q2);
      levelset::crossing<3>(C3.p, C3.v, CL.p, CL.v, 0.0, Q3);
    } else {
      levelset::crossing<3>(CL.p, CL.v, C1.p, C1.v, 0.0, Q1);
      levelset::crossing<3>(CL.p, CL.v, C2.p, C2.v, 0.0, Q2);
      levelset::crossing<3>(CL.p, CL.v, C3.p, C3.v, 0.0, Q3);
    }
    ntri = (int)isosurface::triangle(Q1, Q2, Q3, CL.p, one, tri[0], area[0]);
  } else {
    // two above: A0 < A1 the corners above, B0 < B1 the corners not above
    const int a0 = up[0] ? 0 : (up[1] ? 1 : 2), a1 = up[3] ? 3 : (up[2] ? 2 : 1);
    const int b0 = !up[0] ? 0 : (!up[1] ? 1 : 2), b1 = !up[3] ? 3 : (!up[2] ? 2 : 1);
    const Corner A0 = pick(R, a0), A1 = pick(R, a1), B0 = pick(R, b0), B1 = pick(R, b1);
    double Q00[3], Q01[3], Q10[3], Q11[3];      // Q_ij: from B_j to A_i
    levelset::crossing<3>(B0.p, B0.v, A0.p, A0.v, 0.0, Q00);
    levelset::crossing<3>(B1.p, B1.v, A0.p, A0.v, 0.0, Q01);
    levelset::crossing<3>(B0.p, B0.v, A1.p, A1.v, 0.0, Q10);
    levelset::crossing<3>(B1.p, B1.v, A1.p, A1.v, 0.0, Q11);
    // the quadrilateral Q00 Q01 Q11 Q10 along its diagonal Q01 - Q10
    const bool first = isosurface::triangle(Q00, Q01, Q10, A0.p, true, tri[0], area[0]);
    const bool second = isosurface::triangle(Q01, Q11, Q10, A0.p, true, tri[1], area[1]);
    if (second & !first) {
#pragma unroll
      for (int d = 0; d < isosurface::kTriWidth; ++d) tri[0][d] = tri[1][d];
      area[0] = area[1];
    }
    ntri = (int)first + (int)second;
  }
  if (ntri == 0) return;
  double nu[3];
  unit_normal<3>(plane, nu);
  bool good = true;
  double uv[2][3] = {};
#pragma unroll 1
  for (int q = 0; q < ntri; ++q) {
    // the vertices of piece q by selects, never by a run-time index into registers
    double V[isosurface::kTriWidth];
#pragma unroll
    for (int d = 0; d < isosurface::kTriWidth; ++d) V[d] = q == 0 ? tri[0][d] : tri[1][d];
    const double two_area = 2.0 * (q == 0 ? area[0] : area[1]);
    double pc[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
    for (int i = 0; i < NG; ++i) {
      const double s = Gauss<NG>::x[i], wi = Gauss<NG>::w[i];
#pragma unroll 1
      for (int j = 0; j < NG; ++j) {
        const double tt = Gauss<NG>::x[j];
        const double b0 = 1.0 - s, b1 = s * (1.0 - tt), b2 = s * tt;
        double xq[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) xq[d] = (b0 * V[d] + b1 * V[3 + d]) + b2 * V[6 + d];
        good = good & point<3, K>(A, z, e, nu, xq, ((wi * Gauss<NG>::w[j]) * s) * two_area, pc, T.c);
      }
    }
    T.c[0] += pc[0];
    T.c[1] += pc[1];
    T.c[2] += pc[2];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double val = value_at<3, K>(A, z, e, V + 3 * m);
      uv[0][m] = q == 0 ? val : uv[0][m];
      uv[1][m] = q == 0 ? uv[1][m] : val;
    }
  }
  if (!good) {
    poison(T);
    return;
  }
#pragma unroll
  for (int d = 0; d < isosurface::kTriWidth; ++d) {
    T.piece[0][d] = tri[0][d];
    T.piece[1][d] = tri[1][d];
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    T.piece[0][isosurface::kTriWidth + m] = uv[0][m];
    T.piece[1][isosurface::kTriWidth + m] = uv[1][m];
  }
  T.emit = ntri;
}

template <int DIM, int K>
MGB_HD void item(const Args& A, const double* z, const double* plane, long long it, Term<DIM>& T) {
  if constexpr (DIM == 2) item2d(A, z, plane, it, T);
  else item3d<K>(A, z, plane, it, T);
}

// The ONE place where the arguments of a call are checked, the planes apart (check_planes): the C entry points call it with
// their name as `who` before anything is allocated, launched or written; the launches and the host restatement call it again.
void check(const std::string& who, const Args& A, int dim, int k);

// a zero or non-finite normal and a non-finite offset are argument errors
inline void check_planes(const std::string& who, int dim, int nc, const double* planes) {
  for (int r = 0; r < nc; ++r) {
    const double* P = planes + (size_t)r * (dim + 1);
    bool fin = true, zero = true;
    for (int d = 0; d < dim; ++d) {
      fin = fin && interp::finite(P[d]);
      zero = zero && P[d] == 0.0;
    }
    if (!fin || zero) throw ArgError(who + ": the normal of every plane must be finite and not zero");
    if (!interp::finite(P[dim])) throw ArgError(who + ": the offset c of every plane must be finite");
    double s = 0.0;
    for (int d = 0; d < dim; ++d) s += P[d] * P[d];
    if (!(interp::finite(s) && s > 0.0)) throw ArgError(who + ": the normal of every plane must have a finite, positive length");
  }
}

// section.hip, host: the same per-item routine, serially, row after row (row = field * nc + plane) in ascending item order.
// out: B nc x kCols; counts: B nc; row_offsets (nullable): B nc + 1; piece, item (both or neither; `capacity` rows of
// piece_width(dim) doubles): the emitted pieces and their items.  Throws ArgError where the rows do not fit into capacity.
void sections_host(int dim, int k, const Args& A, double* out, long long* counts, long long* row_offsets, double* piece,
                   int32_t* item_out, long long capacity);

#if defined(__HIPCC__)
// section.hip: the two launches of levelset.hpp's launch_measure on the same buffers (scratch_words, count_words): the
// measure on grid (workgroups(items), nc, B), then levelset::launch_finish; all pointers of A are device pointers
void launch_measure(hipStream_t stream, int dim, int k, const Args& A, double* scratch, long long* counts);
// one launch on the measure's grid: the first piece of an item goes to slot row_base[r] + offsets[r (nwg + 1) + g] + its rank
// in the workgroup, its second one to the next slot; slots beyond `total` are not written; piece: total x piece_width(dim),
// item_out: total
void launch_emit(hipStream_t stream, int dim, int k, const Args& A, const long long* offsets, const long long* row_base,
                 long long total, double* piece, int32_t* item_out);
#endif

}  // namespace section
}  // namespace mgb
