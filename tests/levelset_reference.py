"""Independent numpy restatement, in np.longdouble, of the level-set rule of include/mgb_hip.h: the
yardstick of test_levelset_reference.py, test_levelset_host.py and test_gpu_level_sets.py.  Not a test.  It takes x, z, levels
and refine and shares no code with the library: the lattice, the P2 + bubble basis, the classification, the below-to-above
crossing rule, the orientation and the per-item terms are all written out again here, vectorised over the items.

Per level it returns a Level: rows (5,), the sums of the absolute per-item terms behind rows[0..2], the emitted segments in
ascending item order with their items, and for every emitted endpoint the error bar a double-precision evaluation is held to:

  r = 0:  8 eps (|P_hi - P_lo|_inf + max|x|)       the roundings of c - v_lo, v_hi - v_lo and the division (three in all, each
                                                    moving Q by at most eps |P_hi - P_lo|), the product and the sum that form Q
                                                    (eps |P_hi - P_lo| and eps max|x|), with room;
  r > 0:  ... + 32 eps (S / |v_hi - v_lo|) |P_hi - P_lo|_inf,   S = the larger sum_j |N_j| |z_j| of the two corners: a
                                                    seven-term basis sum carries at most 16 eps S, and both corners move t.

For r > 0 a lattice value is computed, so a value closer to the level than its own rounding could be classified either way;
`margin` = min |v - c| over all lattice values and `value_bar` = 32 eps max S let a test assert that this cannot happen."""
import math

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
RING = (0, 3, 1, 4, 2, 5)      # v1 m12 v2 m23 v3 m31 of the block v1 v2 v3 m12 m23 m31 centroid
THIRD = LD(1) / LD(3)
REF = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0.5, 0.5], [0, 0.5], [THIRD, THIRD]], dtype=LD)


class Level:
    """rows (5,) longdouble; abs_terms (3,); count; items (m,); seg (m, 4) (1-D: (m, 2)); bar (m, 2) per endpoint (1-D: (m,));
    vmax = max |v|; margin, value_bar (r > 0)."""


def small_triangles(r):
    """(N^2, 3, 2) lattice indices (a, b) of the corners of small triangle j = 0..N^2-1."""
    N, out = 2 ** r, []
    for j in range(N * N):
        i = math.isqrt(j)
        q, b = j - i * i, N - 1 - i
        if q % 2 == 0:
            a = q // 2
            out.append([(a, b), (a + 1, b), (a, b + 1)])
        else:
            a = (q - 1) // 2
            out.append([(a + 1, b), (a + 1, b + 1), (a, b + 1)])
    return np.array(out)


def basis(xi, et):
    """P2 + cubic bubble nodal basis of the block at reference points (..., ) -> (..., 7)."""
    l = [1 - xi - et, xi, et]
    b = l[0] * l[1] * l[2]
    out = [l[i] * (2 * l[i] - 1) + 3 * b for i in range(3)]
    out += [4 * l[i] * l[(i + 1) % 3] - 12 * b for i in range(3)]
    out.append(27 * b)
    return np.stack(out, axis=-1)


def lattice_2d(x, z, r):
    """P (items, 3, 2), v (items, 3), S = sum |N_j| |z_j| (items, 3) in item order (e 6 + k) N^2 + j."""
    nel = x.shape[0] // 7
    xe, ze = x.reshape(nel, 7, 2).astype(LD), z.reshape(nel, 7).astype(LD)
    N = 2 ** r
    lat = small_triangles(r)
    fa, fb = lat[:, :, 0].astype(LD) / N, lat[:, :, 1].astype(LD) / N      # (N^2, 3)
    Ps, vs, Ss = [], [], []
    for k in range(6):
        ia, ib, ic = RING[k], RING[(k + 1) % 6], 6
        A, B, Cc = xe[:, ia], xe[:, ib], xe[:, ic]
        P = (A[:, None, None, :] + fa[None, :, :, None] * (B - A)[:, None, None, :]
             + fb[None, :, :, None] * (Cc - A)[:, None, None, :])
        if r == 0:
            v = ze[:, [ia, ib, ic]][:, None, :]
            S = np.abs(v)
        else:
            R = REF[ia] + fa[:, :, None] * (REF[ib] - REF[ia]) + fb[:, :, None] * (REF[ic] - REF[ia])      # (N^2, 3, 2)
            Nb = basis(R[..., 0], R[..., 1])                                                                # (N^2, 3, 7)
            with np.errstate(invalid="ignore"):
                v = np.einsum("jmn,en->ejm", Nb, ze)
                S = np.einsum("jmn,en->ejm", np.abs(Nb), np.abs(ze))
        Ps.append(P), vs.append(v), Ss.append(S)
    P = np.stack(Ps, axis=1).reshape(-1, 3, 2)
    v = np.stack(vs, axis=1).reshape(-1, 3)
    S = np.stack(Ss, axis=1).reshape(-1, 3)
    return P, v, S


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def _pick(arr, idx):
    return arr[np.arange(arr.shape[0]), idx]


def _rows(out, terms, fin, v, c):
    """rows, abs_terms, vmax of a Level from the (items, 3) per-item terms; NaN rows where an item is not finite."""
    out.vmax = np.abs(v[fin]).max() if fin.any() else LD(0)
    if not fin.all():
        out.rows = np.full(5, np.nan, dtype=LD)
        out.abs_terms = np.full(3, np.nan, dtype=LD)
        return
    out.rows = np.array([terms[:, 0].sum(), terms[:, 1].sum(), terms[:, 2].sum(), (v - c).max(), (c - v).max()], dtype=LD)
    out.abs_terms = np.abs(terms).sum(axis=0)


def level_sets_2d(x, z, levels, refine):
    P, v, S = lattice_2d(np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64), refine)
    xmax = LD(np.abs(x).max())
    fin = np.isfinite(v).all(axis=1)
    area = np.abs(_cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])) / 2
    res = []
    for c in levels:
        c = LD(c)
        out = Level()
        with np.errstate(invalid="ignore"):
            up = (v > c) & fin[:, None]
        kab = up.sum(axis=1)
        terms = np.zeros((v.shape[0], 3), dtype=LD)
        with np.errstate(invalid="ignore"):
            mean_ex = (v[:, 0] + v[:, 1] + v[:, 2]) / 3 - c
        k3 = fin & (kab == 3)
        terms[k3, 0], terms[k3, 2] = area[k3], (area * mean_ex)[k3]
        cut = np.nonzero(fin & ((kab == 1) | (kab == 2)))[0]
        one = kab[cut] == 1
        L = np.where(one, up[cut].argmax(axis=1), up[cut].argmin(axis=1))
        o1, o2 = (L + 1) % 3, (L + 2) % 3
        Pc, vc, Sc = P[cut], v[cut], S[cut]
        PL, vL, SL = _pick(Pc, L), _pick(vc, L), _pick(Sc, L)
        Q, bars = [], []
        for o in (o1, o2):
            Po, vo, So = _pick(Pc, o), _pick(vc, o), _pick(Sc, o)
            Plo, Phi = np.where(one[:, None], Po, PL), np.where(one[:, None], PL, Po)
            vlo, vhi = np.where(one, vo, vL), np.where(one, vL, vo)
            t = (c - vlo) / (vhi - vlo)
            Q.append(Plo + t[:, None] * (Phi - Plo))
            span = np.abs(Phi - Plo).max(axis=1)
            bar = 8 * EPS * (span + xmax)
            if refine > 0:
                bar = bar + 32 * EPS * (np.maximum(SL, So) / np.abs(vhi - vlo)) * span
            bars.append(bar)
        Q0, Q1 = Q
        above = np.where(one[:, None], PL, _pick(Pc, o1))
        a_s = np.abs(_cross(Q0 - PL, Q1 - PL)) / 2
        d = Q1 - Q0
        terms[cut, 1] = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
        terms[cut, 0] = np.where(one, a_s, area[cut] - a_s)
        terms[cut, 2] = np.where(one, a_s * (vL - c) / 3, area[cut] * mean_ex[cut] - a_s * (vL - c) / 3)
        swap = _cross(d, above - Q0) < 0
        emit = ~(~one & (vL == c))
        seg = np.where(swap[:, None], np.hstack([Q1, Q0]), np.hstack([Q0, Q1]))
        bar = np.where(swap[:, None], np.stack([bars[1], bars[0]], axis=1), np.stack(bars, axis=1))
        out.seg, out.bar, out.items, out.count = seg[emit], bar[emit], cut[emit], int(emit.sum())
        _rows(out, terms, fin, v, c)
        out.margin = np.abs(v[fin] - c).min() if fin.any() else LD(np.inf)
        out.value_bar = 32 * EPS * (S[fin].max() if fin.any() else LD(0))
        res.append(out)
    return res


def level_sets_1d(x, z, levels):
    x, z = np.asarray(x, dtype=np.float64).reshape(-1, 2).astype(LD), np.asarray(z, dtype=np.float64).reshape(-1, 2).astype(LD)
    xmax = np.abs(x).max()
    fin = np.isfinite(z).all(axis=1)
    h = np.abs(x[:, 1] - x[:, 0])
    res = []
    for c in levels:
        c = LD(c)
        out = Level()
        with np.errstate(invalid="ignore"):
            up = (z > c) & fin[:, None]
        kab = up.sum(axis=1)
        terms = np.zeros((x.shape[0], 3), dtype=LD)
        both = fin & (kab == 2)
        with np.errstate(invalid="ignore"):
            terms[both, 0], terms[both, 2] = h[both], (h * ((z[:, 0] + z[:, 1]) / 2 - c))[both]
        cut = np.nonzero(fin & (kab == 1))[0]
        right = up[cut, 1]                      # the right node is the one above: u rises in +x
        xlo, xhi = np.where(right, x[cut, 0], x[cut, 1]), np.where(right, x[cut, 1], x[cut, 0])
        vlo, vhi = np.where(right, z[cut, 0], z[cut, 1]), np.where(right, z[cut, 1], z[cut, 0])
        t = (c - vlo) / (vhi - vlo)
        terms[cut, 0], terms[cut, 1], terms[cut, 2] = (1 - t) * h[cut], 1, (1 - t) * h[cut] * (vhi - c) / 2
        out.seg = np.stack([xlo + t * (xhi - xlo), np.where(xhi > xlo, LD(1), LD(-1))], axis=1)
        out.bar = 8 * EPS * (np.abs(xhi - xlo) + xmax)
        out.items, out.count = cut, len(cut)
        _rows(out, terms, fin, z, c)
        out.margin, out.value_bar = LD(np.inf), LD(0)
        res.append(out)
    return res


def level_sets(x, z, levels, refine=0):
    """One Level per level for the nodal column z (n,) on the nodes x (n, dim), dim 1 or 2."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    if x.shape[1] == 1:
        assert refine == 0
        return level_sets_1d(x, z, levels)
    assert x.shape[1] == 2
    return level_sets_2d(x, z, levels, refine)
