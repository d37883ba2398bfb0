"""Independent numpy restatement, in np.longdouble, of the isosurface rule of include/mgb_hip.h: the
yardstick of test_isosurface_reference.py, test_isosurface_host.py and test_gpu_isosurfaces.py.  Not a test.  It takes x, z,
the degree k, levels and refine and shares no code with the library: the lattice, the tensor Lagrange basis, the Kuhn
tetrahedra, the classification, the below-to-above crossing rule, the pieces and the orientation are all written out again
here, vectorised over the items.

Per level it returns a Level: rows (5,), the sums of the absolute per-item terms behind rows[0..2], the emitted triangles in
ascending item order with their items, and for every emitted vertex the error bar a double-precision evaluation is held to,
the bars of levelset_reference.py:

  r = 0:  8 eps (|P_hi - P_lo|_inf + max|x|)       the roundings of c - v_lo, v_hi - v_lo and the division (three in all, each
                                                    moving Q by at most eps |P_hi - P_lo|), the product and the sum that form Q
                                                    (eps |P_hi - P_lo| and eps max|x|), with room;
  r > 0:  ... + 32 eps (S / |v_hi - v_lo|) |P_hi - P_lo|_inf,   S = the larger sum_j |N_j| |z_j| of the two corners over the
                                                    (k+1)^3 tensor basis: the bar of the 2-D rule, kept.  A computed lattice
                                                    value is off by a modest multiple of eps S (the roundings of the
                                                    one-dimensional bases, their products and the nested sums), and both
                                                    corners move t; the largest ratio measured against this bar is 0.034.
                                                    The lattice positions A + f (B - A) carry 3 eps max|x| of their own,
                                                    inside the 8.

For r > 0 a lattice value is computed, so a value closer to the level than its own rounding could be classified either way;
`margin` = min |v - c| over all lattice values and `value_bar` = 32 eps max S let a test assert that this cannot happen."""
import itertools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
PERMS = list(itertools.permutations(range(3)))      # lexicographic: abc acb bac bca cab cba
OTHERS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])


class Level:
    """rows (5,) longdouble; abs_terms (3,); count; items (m,); tri (m, 9); bar (m, 3) per vertex; vmax = max |v|; margin,
    value_bar (r > 0)."""


def kuhn():
    """(6, 4, 3) lattice offsets (da, db, dc) of the four corners of the six tetrahedra of a cell."""
    out = np.zeros((6, 4, 3), dtype=np.int64)
    for t, p in enumerate(PERMS):
        out[t, 1, p[0]] = 1
        out[t, 2, p[0]] = out[t, 2, p[1]] = 1
        out[t, 3] = 1
    return out


def lagrange(k, f):
    """(len(f), k + 1): the Lagrange basis on the nodes j / k of [0, 1] at the points f."""
    t = k * np.asarray(f, dtype=LD)
    out = np.ones((len(t), k + 1), dtype=LD)
    for j in range(k + 1):
        for i in range(k + 1):
            if i != j:
                out[:, j] *= (t - i) / LD(j - i)
    return out


def lattice(x, z, k, r):
    """P (items, 4, 3), v (items, 4), S = sum |N_j| |z_j| (items, 4) in item order (e M^3 + cell) 6 + t."""
    m1 = k + 1
    nel = x.shape[0] // m1 ** 3
    xe, ze = x.reshape(nel, m1, m1, m1, 3).astype(LD), z.reshape(nel, m1, m1, m1).astype(LD)      # axes e, c, b, a
    M = k * 2 ** r
    if r == 0:
        pts, val = xe, ze
        S = np.abs(ze)
    else:
        f = np.arange(M + 1).astype(LD) / M
        Lb = lagrange(k, f)
        with np.errstate(invalid="ignore"):
            val = np.einsum("ck,bj,ai,ekji->ecba", Lb, Lb, Lb, ze)
            S = np.einsum("ck,bj,ai,ekji->ecba", np.abs(Lb), np.abs(Lb), np.abs(Lb), np.abs(ze))
        A, B = xe[:, 0, 0, 0], xe[:, -1, -1, -1]
        pts = np.empty((nel, M + 1, M + 1, M + 1, 3), dtype=LD)
        shape = ([1, 1, 1, -1], [1, 1, -1, 1], [1, -1, 1, 1])      # axis d runs along a, b, c
        for d in range(3):
            pts[..., d] = A[:, d].reshape(-1, 1, 1, 1) + f.reshape(shape[d]) * (B[:, d] - A[:, d]).reshape(-1, 1, 1, 1)
    off = kuhn()
    cc, cb, ca = np.meshgrid(np.arange(M), np.arange(M), np.arange(M), indexing="ij")
    ia = ca[None, ..., None, None] + off[:, :, 0]      # (1, M, M, M, 6, 4)
    ib = cb[None, ..., None, None] + off[:, :, 1]
    ic = cc[None, ..., None, None] + off[:, :, 2]
    e = np.arange(nel).reshape(-1, 1, 1, 1, 1, 1)
    P = pts[e, ic, ib, ia].reshape(-1, 4, 3)
    v = val[e, ic, ib, ia].reshape(-1, 4)
    S = S[e, ic, ib, ia].reshape(-1, 4)
    return P, v, S


def _det(a, b, c):
    return (a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]) + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2])
            + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))


def _vol(p0, p1, p2, p3):
    return np.abs(_det(p1 - p0, p2 - p0, p3 - p0)) / 6


def _pick(arr, idx):
    return arr[np.arange(arr.shape[0]), idx]


class _Cross:
    """The crossings of the level on the edges lo -> hi, with their bars."""

    def __init__(self, c, xmax, refine):
        self.c, self.xmax, self.refine = c, xmax, refine

    def __call__(self, lo, hi):
        (Plo, vlo, Slo), (Phi, vhi, Shi) = lo, hi
        t = (self.c - vlo) / (vhi - vlo)
        span = np.abs(Phi - Plo).max(axis=1)
        bar = 8 * EPS * (span + self.xmax)
        if self.refine > 0:
            bar = bar + 32 * EPS * (np.maximum(Slo, Shi) / np.abs(vhi - vlo)) * span
        return Plo + t[:, None] * (Phi - Plo), bar


def _triangle(q, bars, ref, ref_above):
    """q: three (n, 3) vertices with their (n,) bars.  Returns the (n, 9) oriented triangles, (n, 3) bars, the (n,) areas and
    which are emitted: no two vertices the same point."""
    q0, q1, q2 = q
    same = lambda a, b: (a == b).all(axis=1)
    emit = ~(same(q0, q1) | same(q0, q2) | same(q1, q2))
    n = np.cross(q1 - q0, q2 - q0)
    area = np.where(emit, np.sqrt((n * n).sum(axis=1)) / 2, LD(0))
    s = (n * (ref - q0)).sum(axis=1)
    swap = np.where(ref_above, s > 0, s < 0)
    tri = np.where(swap[:, None], np.hstack([q0, q2, q1]), np.hstack([q0, q1, q2]))
    bar = np.where(swap[:, None], np.stack([bars[0], bars[2], bars[1]], axis=1), np.stack(bars, axis=1))
    return tri, bar, area, emit


def isosurfaces(x, z, k, levels, refine=0):
    """One Level per level for the nodal column z (n,) on the nodes x (n, 3) of elements of degree k."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] == 3 and k in (1, 2, 3) and refine in (0, 1, 2)
    P, v, S = lattice(x, z, k, refine)
    n = v.shape[0]
    xmax = LD(np.abs(x).max())
    fin = np.isfinite(v).all(axis=1)
    vol = _vol(P[:, 0], P[:, 1], P[:, 2], P[:, 3])
    res = []
    for c in levels:
        c = LD(c)
        out = Level()
        cross = _Cross(c, xmax, refine)
        with np.errstate(invalid="ignore"):
            up = (v > c) & fin[:, None]
            mean_ex = (v[:, 0] + v[:, 1] + v[:, 2] + v[:, 3]) / 4 - c
        kab = up.sum(axis=1)
        terms = np.zeros((n, 3), dtype=LD)
        tri = np.zeros((n, 2, 9), dtype=LD)
        bar = np.zeros((n, 2, 3), dtype=LD)
        emit = np.zeros((n, 2), dtype=bool)
        k4 = fin & (kab == 4)
        terms[k4, 0], terms[k4, 2] = vol[k4], (vol * mean_ex)[k4]
        # one or three above: the corner piece at the lone corner
        cut = np.nonzero(fin & ((kab == 1) | (kab == 3)))[0]
        one = kab[cut] == 1
        L = np.where(one, up[cut].argmax(axis=1), up[cut].argmin(axis=1))
        corner = lambda idx, rows: (_pick(P[rows], idx), _pick(v[rows], idx), _pick(S[rows], idx))
        CL = corner(L, cut)
        Q, bars = [], []
        for j in range(3):
            Co = corner(OTHERS[L, j], cut)
            lo = tuple(np.where(one.reshape((-1,) + (1,) * (a.ndim - 1)), a, b) for a, b in zip(Co, CL))
            hi = tuple(np.where(one.reshape((-1,) + (1,) * (a.ndim - 1)), b, a) for a, b in zip(Co, CL))
            q, b = cross(lo, hi)
            Q.append(q), bars.append(b)
        v_s = _vol(CL[0], Q[0], Q[1], Q[2])
        x_s = v_s * ((CL[1] - c) / 4)
        terms[cut, 0] = np.where(one, v_s, vol[cut] - v_s)
        terms[cut, 2] = np.where(one, x_s, vol[cut] * mean_ex[cut] - x_s)
        tri[cut, 0], bar[cut, 0], terms[cut, 1], emit[cut, 0] = _triangle(Q, bars, CL[0], one)
        # two above: the wedge and the quadrilateral
        cut = np.nonzero(fin & (kab == 2))[0]
        u2 = up[cut]
        A0, A1 = corner(u2.argmax(axis=1), cut), corner(3 - u2[:, ::-1].argmax(axis=1), cut)
        B0, B1 = corner((~u2).argmax(axis=1), cut), corner(3 - (~u2)[:, ::-1].argmax(axis=1), cut)
        (Q00, b00), (Q01, b01), (Q10, b10), (Q11, b11) = cross(B0, A0), cross(B1, A0), cross(B0, A1), cross(B1, A1)
        w1, w2, w3 = _vol(A0[0], Q00, Q01, A1[0]), _vol(Q00, Q01, A1[0], Q10), _vol(Q01, A1[0], Q10, Q11)
        e0, e1 = A0[1] - c, A1[1] - c
        terms[cut, 0] = w1 + w2 + w3
        terms[cut, 2] = w1 * ((e0 + e1) / 4) + w2 * (e1 / 4) + w3 * (e1 / 4)
        above = np.ones(len(cut), dtype=bool)
        tri[cut, 0], bar[cut, 0], ar1, emit[cut, 0] = _triangle((Q00, Q01, Q10), (b00, b01, b10), A0[0], above)
        tri[cut, 1], bar[cut, 1], ar2, emit[cut, 1] = _triangle((Q01, Q11, Q10), (b01, b11, b10), A0[0], above)
        terms[cut, 1] = ar1 + ar2
        flat = emit.reshape(-1)
        out.tri, out.bar = tri.reshape(-1, 9)[flat], bar.reshape(-1, 3)[flat]
        out.items, out.count = np.repeat(np.arange(n), 2)[flat], int(flat.sum())
        out.vmax = np.abs(v[fin]).max() if fin.any() else LD(0)
        if fin.all():
            out.rows = np.array([terms[:, 0].sum(), terms[:, 1].sum(), terms[:, 2].sum(), (v - c).max(), (c - v).max()], dtype=LD)
            out.abs_terms = np.abs(terms).sum(axis=0)
        else:
            out.rows, out.abs_terms = np.full(5, np.nan, dtype=LD), np.full(3, np.nan, dtype=LD)
        out.margin = np.abs(v[fin] - c).min() if fin.any() else LD(np.inf)
        out.value_bar = 32 * EPS * (S[fin].max() if fin.any() else LD(0))
        res.append(out)
    return res
