// Isosurfaces of 3-D nodal fields: what ONE item contributes, written ONCE.  The gfx950 kernels
// (isosurface.hip) and the host restatement (mgb_geo_isosurfaces_host) both run item() below; lagrange is interp.hpp's, the
// crossing rule, the identity of the rows and the layout of the launch buffers are levelset.hpp's, combine and block_reduce
// are reduce.hpp's.  The full rule is the comment of mgb_geo_isosurfaces in include/mgb_hip.h; in short:
//   block (k+1)^3, k = 1..3, equispaced tensor nodes (x fastest) on the axis-aligned box of the first and the last node.
//   With N = 2^refine and M = k N an element has M^3 cells of the lattice (a, b, c), 0 <= a, b, c <= M; every cell is cut into
//   the six Kuhn tetrahedra around its diagonal (0,0,0)-(1,1,1): tetrahedron t belongs to the t-th permutation (p0, p1, p2) of
//   the axes in lexicographic order and has the corners O, O + e_p0, O + e_p0 + e_p1, O + (1,1,1).
//   item = (e M^3 + cell) 6 + t, cell = a + M (b + M c).
//   Lattice values: at refine = 0 the nodal values and the node coordinates, loaded; at refine > 0 the tensor Lagrange function
//   at (a, b, c) / M and the position A + (a, b, c) / M (B - A) from the box corners A, B: functions of the lattice index alone.
//   A corner is above when v > c; a crossing runs from the below corner to the above corner (levelset::crossing).
// The arithmetic is kept as written by ONE mechanism: isosurface.hip, which holds the kernels AND the host restatement and is
// the only file that may instantiate item(), is compiled with -ffp-contract=off (build.sh).
#pragma once
#include <cstdint>

#include "levelset.hpp"

namespace mgb {
namespace isosurface {

using levelset::Args;
using levelset::kCols;
using levelset::kThreads;
using levelset::kWaves;
using levelset::nanmax;
using levelset::no_items;
using levelset::NoItems;
using levelset::workgroups;

constexpr int kMaxRefine = 2;
constexpr int kTriWidth = 9;      // doubles of a triangle row: x0 y0 z0 x1 y1 z1 x2 y2 z2

// items of one (field, level) row: 6 (k 2^refine)^3 nel
inline long long items_per_row(int k, int nel, int refine) {
  const long long M = (long long)k << refine;
  return 6LL * M * M * M * nel;
}

// corners 1 and 2 of the six Kuhn tetrahedra as lattice offsets (bit 0: a, bit 1: b, bit 2: c), six bits per tetrahedron,
// corner 1 in the low three; corner 0 is offset 0 and corner 3 is offset 7.  Permutations of the axes in lexicographic order:
//   t = 0 (a,b,c): 1, 3    t = 1 (a,c,b): 1, 5    t = 2 (b,a,c): 2, 3    t = 3 (b,c,a): 2, 6    t = 4 (c,a,b): 4, 5    t = 5 (c,b,a): 4, 6
constexpr unsigned long long kKuhn = (1ull | 3ull << 3) | (1ull | 5ull << 3) << 6 | (2ull | 3ull << 3) << 12 | (2ull | 6ull << 3) << 18 |
                                     (4ull | 5ull << 3) << 24 | (4ull | 6ull << 3) << 30;

// what one item gives: the five contributions and its `emit` = 0, 1 or 2 triangles, oriented, in the order of the rule
struct Term {
  double c[kCols];
  double tri[2][kTriWidth];
  int emit;
};

MGB_HD void poison(Term& T) {
  T.c[0] = T.c[1] = T.c[2] = T.c[3] = T.c[4] = std::numeric_limits<double>::quiet_NaN();
  T.emit = 0;
}

// a point with its value; corner j of four by a select chain, never by a run-time index into registers
struct Corner {
  double p[3], v;
};
MGB_HD Corner pick(const Corner* R, int j) {
  Corner o = R[0];
#pragma unroll
  for (int m = 1; m < 4; ++m) {
    const bool is = j == m;
    o.p[0] = is ? R[m].p[0] : o.p[0];
    o.p[1] = is ? R[m].p[1] : o.p[1];
    o.p[2] = is ? R[m].p[2] : o.p[2];
    o.v = is ? R[m].v : o.v;
  }
  return o;
}

// a . (b x c)
MGB_HD double det3(const double* a, const double* b, const double* c) {
  return a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// |det [p1 - p0, p2 - p0, p3 - p0]| / 6
MGB_HD double tet_volume(const double* p0, const double* p1, const double* p2, const double* p3) {
  double a[3], b[3], c[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a[d] = p1[d] - p0[d];
    b[d] = p2[d] - p0[d];
    c[d] = p3[d] - p0[d];
  }
  return fabs(det3(a, b, c)) / 6.0;
}

MGB_HD bool same_point(const double* a, const double* b) {
  return (a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2]);
}

// The triangle (q0, q1, q2) of the level: false, and nothing written, where two of its vertices are the same point.  Else
// out = the triangle with n = (P1 - P0) x (P2 - P0) pointing to the below side -- q1 and q2 are exchanged when n . (ref - q0)
// > 0 for a reference point on the above side, < 0 for one on the below side -- and area = |n| / 2.
MGB_HD bool triangle(const double* q0, const double* q1, const double* q2, const double* ref, bool ref_above, double* out,
                     double& area) {
  area = 0.0;
  if (same_point(q0, q1) || same_point(q0, q2) || same_point(q1, q2)) return false;
  double a[3], b[3], r[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    a[d] = q1[d] - q0[d];
    b[d] = q2[d] - q0[d];
    r[d] = ref[d] - q0[d];
  }
  const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  area = 0.5 * sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const double s = n[0] * r[0] + n[1] * r[1] + n[2] * r[2];
  const bool swap = ref_above ? s > 0.0 : s < 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    out[d] = q0[d];
    out[3 + d] = swap ? q2[d] : q1[d];
    out[6 + d] = swap ? q1[d] : q2[d];
  }
  return true;
}

// the four lattice points of an item and their values
template <int K>
MGB_HD void lattice(const Args& A, const double* z, long long item, Corner* R) {
  constexpr int M1 = K + 1, BLOCK = M1 * M1 * M1;
  const int M = K << A.refine;
  const long long M3 = (long long)M * M * M;
  const int t = (int)(item % 6);
  const long long ec = item / 6;
  const int cell = (int)(ec % M3);
  const size_t e = (size_t)(ec / M3);
  const int ca = cell % M, cb = (cell / M) % M, cc = cell / (M * M);
  const int code = (int)((kKuhn >> (6 * t)) & 63ull);
  const int off[4] = {0, code & 7, code >> 3, 7};
  const double* xe = A.x + e * BLOCK * 3;
  const double* ze = z + e * BLOCK * A.S + A.u;
  if (A.refine == 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const size_t node = (size_t)((ca + (off[m] & 1)) + M1 * ((cb + ((off[m] >> 1) & 1)) + M1 * (cc + (off[m] >> 2))));
      R[m].p[0] = xe[3 * node];
      R[m].p[1] = xe[3 * node + 1];
      R[m].p[2] = xe[3 * node + 2];
      R[m].v = ze[node * A.S];
    }
    return;
  }
  // The four corners take their index along every axis from the two of the cell, so the one-dimensional bases, the
  // positions and the x-lines are formed once per index s = 0, 1 and picked per corner; what a corner gets is still
  //   sum_kk sum_j (sum_i l_a[i] z[i, j, kk]) (l_b[j] l_c[kk]),   each sum in ascending order from 0,
  // with l_d the basis at (double)index_d / (double)M: the same operations for the same lattice index in every item.
  const double* xa = xe;
  const double* xb = xe + (size_t)(BLOCK - 1) * 3;
  const int cell3[3] = {ca, cb, cc};
  double bas[3][2][M1], pos[3][2], der[M1];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double f = (double)(cell3[d] + s) / (double)M;
      pos[d][s] = xa[d] + f * (xb[d] - xa[d]);
      interp::lagrange<K>(f, bas[d][s], der);
    }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < M1; ++kk)
#pragma unroll
    for (int j = 0; j < M1; ++j) {
      double line[2] = {0.0, 0.0};      // the x-line of nodes (., j, kk) for both indices along a
#pragma unroll
      for (int i = 0; i < M1; ++i) {
        const double zz = ze[(size_t)(i + M1 * (j + M1 * kk)) * A.S];
        line[0] += bas[0][0][i] * zz;
        line[1] += bas[0][1][i] * zz;
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const bool sa = off[m] & 1, sb = (off[m] >> 1) & 1, sc = off[m] >> 2;
        acc[m] += (sa ? line[1] : line[0]) * ((sb ? bas[1][1][j] : bas[1][0][j]) * (sc ? bas[2][1][kk] : bas[2][0][kk]));
      }
    }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const bool sa = off[m] & 1, sb = (off[m] >> 1) & 1, sc = off[m] >> 2;
    R[m].p[0] = sa ? pos[0][1] : pos[0][0];
    R[m].p[1] = sb ? pos[1][1] : pos[1][0];
    R[m].p[2] = sc ? pos[2][1] : pos[2][0];
    R[m].v = acc[m];
  }
}

template <int K>
MGB_HD void item(const Args& A, const double* z, double c, long long it, Term& T) {
  Corner R[4];
  lattice<K>(A, z, it, R);
  bool good = interp::finite(R[0].v);
  good = good & interp::finite(R[1].v);
  good = good & interp::finite(R[2].v);
  good = good & interp::finite(R[3].v);
  if (!good) {
    poison(T);
    return;
  }
  T.emit = 0;
  T.c[0] = T.c[1] = T.c[2] = 0.0;
  T.c[3] = nanmax(nanmax(nanmax(R[0].v - c, R[1].v - c), R[2].v - c), R[3].v - c);
  T.c[4] = nanmax(nanmax(nanmax(c - R[0].v, c - R[1].v), c - R[2].v), c - R[3].v);
  const bool up[4] = {R[0].v > c, R[1].v > c, R[2].v > c, R[3].v > c};
  const int k_above = (int)up[0] + (int)up[1] + (int)up[2] + (int)up[3];
  if (k_above == 0) return;
  const double vol = tet_volume(R[0].p, R[1].p, R[2].p, R[3].p);
  const double mean_excess = (R[0].v + R[1].v + R[2].v + R[3].v) / 4.0 - c;
  if (k_above == 4) {
    T.c[0] = vol;
    T.c[2] = vol * mean_excess;
    return;
  }
  double area;
  if (k_above != 2) {
    // the lone corner L: the one above (k_above = 1) or the one not above (k_above = 3); the others in ascending order
    const bool one = k_above == 1;
    const int L = up[0] == one ? 0 : (up[1] == one ? 1 : (up[2] == one ? 2 : 3));
    const Corner CL = pick(R, L), C1 = pick(R, L == 0 ? 1 : 0), C2 = pick(R, L <= 1 ? 2 : 1), C3 = pick(R, L == 3 ? 2 : 3);
    double Q1[3], Q2[3], Q3[3];
    if (one) {
      levelset::crossing<3>(C1.p, C1.v, CL.p, CL.v, c, Q1);
      levelset::crossing<3>(C2.p, C2.v, CL.p, CL.v, c, Q2);
      levelset::crossing<3>(C3.p, C3.v, CL.p, CL.v, c, Q3);
    } else {
      levelset::crossing<3>(CL.p, CL.v, C1.p, C1.v, c, Q1);
      levelset::crossing<3>(CL.p, CL.v, C2.p, C2.v, c, Q2);
      levelset::crossing<3>(CL.p, CL.v, C3.p, C3.v, c, Q3);
    }
    const double v_s = tet_volume(CL.p, Q1, Q2, Q3), x_s = v_s * ((CL.v - c) / 4.0);
    T.c[0] = one ? v_s : vol - v_s;
    T.c[2] = one ? x_s : vol * mean_excess - x_s;
    T.emit = (int)triangle(Q1, Q2, Q3, CL.p, one, T.tri[0], area);
    T.c[1] = area;
    return;
  }
  // two above: A0 < A1 the corners above, B0 < B1 the corners not above
  const int a0 = up[0] ? 0 : (up[1] ? 1 : 2), a1 = up[3] ? 3 : (up[2] ? 2 : 1);
  const int b0 = !up[0] ? 0 : (!up[1] ? 1 : 2), b1 = !up[3] ? 3 : (!up[2] ? 2 : 1);
  const Corner A0 = pick(R, a0), A1 = pick(R, a1), B0 = pick(R, b0), B1 = pick(R, b1);
  double Q00[3], Q01[3], Q10[3], Q11[3];      // Q_ij: from B_j to A_i
  levelset::crossing<3>(B0.p, B0.v, A0.p, A0.v, c, Q00);
  levelset::crossing<3>(B1.p, B1.v, A0.p, A0.v, c, Q01);
  levelset::crossing<3>(B0.p, B0.v, A1.p, A1.v, c, Q10);
  levelset::crossing<3>(B1.p, B1.v, A1.p, A1.v, c, Q11);
  // the wedge (A0, Q00, Q01) - (A1, Q10, Q11) as three tetrahedra
  const double w1 = tet_volume(A0.p, Q00, Q01, A1.p), w2 = tet_volume(Q00, Q01, A1.p, Q10), w3 = tet_volume(Q01, A1.p, Q10, Q11);
  const double e0 = A0.v - c, e1 = A1.v - c;
  T.c[0] = w1 + w2 + w3;
  T.c[2] = w1 * ((e0 + e1) / 4.0) + w2 * (e1 / 4.0) + w3 * (e1 / 4.0);
  // the quadrilateral Q00 Q01 Q11 Q10 along its diagonal Q01 - Q10
  const bool first = triangle(Q00, Q01, Q10, A0.p, true, T.tri[0], area);
  T.c[1] = area;
  const bool second = triangle(Q01, Q11, Q10, A0.p, true, T.tri[1], area);
  T.c[1] += area;
  if (second & !first) {
#pragma unroll
    for (int d = 0; d < kTriWidth; ++d) T.tri[0][d] = T.tri[1][d];
  }
  T.emit = (int)first + (int)second;
}

// isosurface.hip, host: the same per-item routine, serially, row after row (row = field * nl + level) in ascending item order.
// out: B nl x kCols; counts: B nl; row_offsets (nullable): B nl + 1; tri, item (both or neither; `capacity` rows): the
// emitted triangles and their items.  Throws ArgError where the rows do not fit into capacity.
void isosurfaces_host(int k, const Args& A, double* out, long long* counts, long long* row_offsets, double* tri, int32_t* item_out,
                      long long capacity);

#if defined(__HIPCC__)
// isosurface.hip: the two launches of levelset.hpp's launch_measure on the same buffers (scratch_words, count_words): the
// measure on grid (workgroups(items), nl, B), then levelset::launch_finish; all pointers of A are device pointers
void launch_measure(hipStream_t stream, int k, const Args& A, double* scratch, long long* counts);
// one launch on the measure's grid: the first triangle of an item goes to slot row_base[r] + offsets[r (nwg + 1) + g] + its
// rank in the workgroup, its second one to the next slot; slots beyond `total` are not written; tri: total x 9, item_out: total
void launch_emit(hipStream_t stream, int k, const Args& A, const long long* offsets, const long long* row_base, long long total,
                 double* tri, int32_t* item_out);
#endif

}  // namespace isosurface
}  // namespace mgb
