"""Independent numpy restatement, in np.longdouble, of the line-integral rule of include/mgb_hip.h: the
yardstick of test_ray_reference.py, test_ray_host.py and test_gpu_line_integrals.py.  Not a test.  It takes x, z, the
dimension, the degree k, the segments and p and shares no code with the library.  It does not walk: every segment is tested
against ALL elements, so a cell the library's walk skips shows as a missing piece.  The Gauss rules, the bases and the flux
are those of the section yardstick (section_reference.py), which is numpy as well.

ONE thing is computed in float64, in the order the rule prescribes: the reference coordinates of a and of b in every element.
Everything behind them -- alpha, beta, the quotients, the midpoints, the containment of the midpoints, the quadrature -- runs
in longdouble.

Bars a double-precision evaluation is held to, all from eps, tau and the terms:

  piece end  t = -(alpha + tau) / beta with alpha, beta formed from the float64 reference coordinates r:
               d_alpha = 2 eps (1 + |r(a)|_1)            (1 - r_0 - r_1: two roundings; the others are exact)
               d_beta  = 4 eps (1 + |r(a)|_1 + |r(b)|_1) (both sides and the difference)
               d_t     = (d_alpha + eps |alpha + tau|) / |beta| + |t| d_beta / |beta| + 2 eps |t|
             an end at 0 or 1 has bar 0.
  decisions  a ray is UNDECIDED, and left out of a comparison, when one of these lies within its bar of its threshold:
               beta == 0     |beta| <= d_beta while |alpha + tau| <= d_alpha + d_beta (otherwise both readings of beta agree:
                             an empty interval for alpha + tau < 0, no constraint for alpha + tau > 0);
               t1 > t0       |t1 - t0| <= d_t0 + d_t1;
               ownership     the containment of the midpoint in an element e' <= e, where no constraint j fails by more than
                             c_bar_j and not all hold by more than c_bar_j,
                             c_bar_j = 16 eps (1 + max|x| / h') + (d_t0 + d_t1) / 2 |beta_j(e')|
                             (the midpoint in float64, its reference coordinates, and the piece ends it is formed from: an
                             end moves the midpoint along the segment, where constraint j changes at the rate beta_j).
  value      section_reference's: 32 eps S + 8 eps (max|x| / h + 1) G + 2 |grad u|_1 dy with dy = d_t l + 4 eps max|x|.
  flux       |d sigma| <= 2 (1 + |p - 2|) a^(p-2) d_g + 4 eps |sigma| (the last term: pow), a = |grad u|,
             d_g = 32 eps (max|x| / h + 1) G / h + the change of grad u over dy (by evaluating it at both displaced points).
  sums       length:   sum l (d_t0 + d_t1) + n eps sum |terms|, n = pieces + 4
             integral: sum om_q vbar_q + sum l (d_t0 + d_t1) max|u| + (n + N) eps sum |terms|; along and across alike.
  extrema    the largest value bar of the row; enter / leave: the largest end bar of the row.

`overlap` (a length): l times [what the owned pieces cover twice in t + tau / |beta_j|, j the active constraint, at every piece
end that no other piece covers, once where several pieces end in the same place] -- what the computed length differs from
the exact chord by, because neighbouring intervals overlap and intervals at the boundary reach out by tau.  A closed form is
met within bar + overlap x max|integrand|; the excess is systematic, so that comparison has no factor to spare, and for the
length the sharper statement holds and is tested: excess = overlap within the rounding bar alone (ratio 0.001), except for
a ray within tau of a face (see test_ray_reference.py)."""
import numpy as np

import section_reference as SR

LD = np.longdouble
EPS = LD(np.finfo(np.float64).eps)
TAU = LD(1e-12)


class Row:
    """rows (8,) longdouble; bars (8,); abs_terms (4,) behind rows[0..3]; count; elements (count,); t0, t1, integral (count,);
    dt0, dt1, ibar (count,): their bars; overlap; peak (4,): the largest |integrand| behind rows[0..3] over the points of the
    row; undecided (bool); poisoned (bool)."""


def ref_coords64(x, dim, block, p):
    """The float64 reference coordinates (nel, dim) of the point p in every element, in the order of interp.hpp."""
    p = np.asarray(p, dtype=np.float64)
    X = np.asarray(x, dtype=np.float64).reshape(-1, block, dim)
    with np.errstate(all="ignore"):
        if dim == 2:
            v = X.reshape(X.shape[0], -1)
            ax, ay, bx, by = v[:, 2] - v[:, 0], v[:, 3] - v[:, 1], v[:, 4] - v[:, 0], v[:, 5] - v[:, 1]
            det = ax * by - ay * bx
            px, py = p[0] - v[:, 0], p[1] - v[:, 1]
            return np.stack([(px * by - py * bx) / det, (ax * py - ay * px) / det], axis=1)
        A, B = X[:, 0], X[:, -1]
        return (p[None, :] - A) / (B - A)


def constraints(r, dim):
    """g_j (..., 3 or 6) longdouble of reference coordinates r (..., dim), and |r|_1."""
    r = np.asarray(r, dtype=LD)
    if dim == 2:
        g = np.stack([1 - r[..., 0] - r[..., 1], r[..., 0], r[..., 1]], axis=-1)
    else:
        g = np.stack([r[..., 0], 1 - r[..., 0], r[..., 1], 1 - r[..., 1], r[..., 2], 1 - r[..., 2]], axis=-1)
    return g, np.abs(r).sum(axis=-1)


def ref_coords_ld(X, dim, P):
    """Longdouble reference coordinates (m, nel, dim) of the points P (m, dim) in the elements X (nel, block, dim)."""
    if dim == 2:
        v0 = X[:, 0]
        ax, ay = (X[:, 1] - v0).T
        bx, by = (X[:, 2] - v0).T
        det = ax * by - ay * bx
        px, py = P[:, None, 0] - v0[None, :, 0], P[:, None, 1] - v0[None, :, 1]
        return np.stack([(px * by - py * bx) / det, (ax * py - ay * px) / det], axis=-1)
    A, B = X[:, 0], X[:, -1]
    return (P[:, None, :] - A[None]) / (B - A)[None]


class Mesh:
    """What the yardstick keeps of a mesh: the elements in longdouble, their smallest extents, max|x|."""

    def __init__(self, x, dim, k):
        self.dim, self.k = dim, k
        self.block = 7 if dim == 2 else (k + 1) ** 3
        self.x64 = np.ascontiguousarray(x, dtype=np.float64)
        self.X = self.x64.astype(LD).reshape(-1, self.block, dim)
        self.nel = self.X.shape[0]
        self.xmax = np.abs(self.X).max()
        if dim == 2:
            v0 = self.X[:, 0]
            ax, ay = (self.X[:, 1] - v0).T
            bx, by = (self.X[:, 2] - v0).T
            edge = np.maximum(np.maximum(np.hypot(ax, ay), np.hypot(bx, by)), np.hypot(bx - ax, by - ay))
            self.h = np.abs(ax * by - ay * bx) / edge
        else:
            self.h = np.abs(self.X[:, -1] - self.X[:, 0]).min(axis=1)


def _geometry(M, a, b):
    """The pieces of one segment, without the field: (elements, t0, t1, dt0, dt1, overlap_t, undecided)."""
    dim = M.dim
    none = (np.zeros(0, dtype=np.int64),) + (np.zeros(0, dtype=LD),) * 4 + (LD(0), False)
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not (np.isfinite(a64).all() and np.isfinite(b64).all()) or (a64 == b64).all():
        return none
    ga, na = constraints(ref_coords64(M.x64, dim, M.block, a64), dim)
    gb, nb = constraints(ref_coords64(M.x64, dim, M.block, b64), dim)
    al, be = ga, gb - ga
    d_al = 2 * EPS * (1 + na)[:, None]
    d_be = 4 * EPS * (1 + na + nb)[:, None]
    s = al + TAU
    undecided = False
    flat = np.abs(be) <= d_be
    flat_out = flat & (s < -(d_al + d_be))
    flat_unsure = flat & ~flat_out & ~(s > d_al + d_be)
    with np.errstate(all="ignore"):
        q = np.where(flat, LD(0), -s / np.where(flat, LD(1), be))
        d_q = np.where(flat, LD(0), (d_al + EPS * np.abs(s)) / np.abs(be) + np.abs(q) * d_be / np.abs(be) + 2 * EPS * np.abs(q))
    up, down = ~flat & (be > 0), ~flat & (be < 0)
    lo = np.where(up, q, -np.inf)
    hi = np.where(down, q, np.inf)
    j0, j1 = lo.argmax(axis=1), hi.argmin(axis=1)
    idx = np.arange(M.nel)
    t0, t1 = lo[idx, j0], hi[idx, j1]
    dt0, dt1 = d_q[idx, j0], d_q[idx, j1]
    ov0, ov1 = TAU / np.abs(np.where(flat, LD(1), be))[idx, j0], TAU / np.abs(np.where(flat, LD(1), be))[idx, j1]
    start, stop = t0 <= 0, t1 >= 1
    # an end within its bar of 0 or 1 is still an end with that bar: the clamp is a comparison like the others
    t0, dt0, ov0 = np.where(start, LD(0), t0), np.where(start & (t0 < -dt0), LD(0), dt0), np.where(start, LD(0), ov0)
    t1, dt1, ov1 = np.where(stop, LD(1), t1), np.where(stop & (t1 > 1 + dt1), LD(0), dt1), np.where(stop, LD(0), ov1)
    alive = ~flat_out.any(axis=1)
    gap = t1 - t0
    sure = alive & (gap > dt0 + dt1) & ~flat_unsure.any(axis=1)
    maybe = alive & (np.abs(gap) <= dt0 + dt1) | (alive & flat_unsure.any(axis=1) & (gap > -(dt0 + dt1)))
    if maybe.any():
        undecided = True
    cand = np.flatnonzero(sure)
    if len(cand) == 0:
        return none[:6] + (undecided,)
    # ownership: the lowest element that holds the midpoint
    d = b64.astype(LD) - a64.astype(LD)
    tm = (t0[cand] + t1[cand]) / 2
    P = a64.astype(LD)[None, :] + tm[:, None] * d[None, :]
    gm, _ = constraints(ref_coords_ld(M.X, dim, P), dim)                       # (ncand, nel, NG)
    c_bar = 16 * EPS * (1 + M.xmax / M.h)[None, :, None] + ((dt0[cand] + dt1[cand]) / 2)[:, None, None] * np.abs(be)[None, :, :]
    inside = gm.min(axis=2) >= -TAU
    # a containment is decided when one constraint fails by more than its bar, or all hold by more than their bars
    near = ~((gm < -TAU - c_bar).any(axis=2) | (gm > -TAU + c_bar).all(axis=2))
    owner = np.where(inside.any(axis=1), inside.argmax(axis=1), -1)
    upto = idx[None, :] <= cand[:, None]
    if (near & upto & (idx[None, :] <= np.where(owner < 0, M.nel, owner)[:, None])).any():
        undecided = True
    own = owner == cand
    e = cand[own]
    order = np.argsort(t0[e], kind="stable")
    e = e[order]
    # the overlap: what the pieces cover twice, plus tau / |beta| at every end that no other piece covers (the reach-out)
    s0, s1 = t0[e], t1[e]
    union, right = LD(0), -np.inf
    for lo_i, hi_i in zip(s0, s1):
        union += max(hi_i, right) - max(lo_i, right) if hi_i > right else LD(0)
        right = max(right, hi_i)
    overlap = (s1 - s0).sum() - union
    for i in range(len(e)):
        o = np.arange(len(e))
        # an end is covered by another piece that contains it; of several pieces with the same end only the first reaches out
        if not ((o != i) & (s0 <= s0[i]) & (s0[i] < s1) & ((s0 < s0[i]) | (o < i))).any():
            overlap += ov0[e[i]]
        if not ((o != i) & (s0 < s1[i]) & (s1[i] <= s1) & ((s1[i] < s1) | (o < i))).any():
            overlap += ov1[e[i]]
    return e, s0, s1, dt0[e], dt1[e], overlap, undecided


_GEOMETRY = {}


def line_integrals(x, z, dim, k, a, b, p=2.0, key=None):
    """One Row per segment of the field z (n,) on the mesh x.  `key`: the geometric part (pieces, ends, bars) is kept under it
    and shared among fields and exponents."""
    with np.errstate(all="ignore"):      # a non-finite node poisons its rows; their bars are not used
        return _line_integrals(x, z, dim, k, a, b, p, key)


def _line_integrals(x, z, dim, k, a, b, p, key):
    a = np.asarray(a, dtype=np.float64).reshape(-1, dim)
    b = np.asarray(b, dtype=np.float64).reshape(-1, dim)
    gkey = None if key is None else (key, dim, k, a.tobytes(), b.tobytes())
    if gkey is not None and gkey in _GEOMETRY:
        M, geo = _GEOMETRY[gkey]
    else:
        M = Mesh(x, dim, k)
        geo = [_geometry(M, a[i], b[i]) for i in range(len(a))]
        if gkey is not None:
            _GEOMETRY[gkey] = (M, geo)
    N = SR.n_gauss(dim, k)
    gx, gw = SR.gauss01(N)
    Z = np.asarray(z, dtype=np.float64).astype(LD).reshape(-1, M.block)
    out = []
    for i, (e, t0, t1, dt0, dt1, overlap, undecided) in enumerate(geo):
        R = Row()
        R.count, R.elements, R.t0, R.t1, R.dt0, R.dt1, R.undecided = len(e), e, t0, t1, dt0, dt1, undecided
        d = b[i].astype(LD) - a[i].astype(LD)
        ell = np.sqrt((d * d).sum())
        R.overlap = overlap * ell
        R.rows = np.array([0, 0, 0, 0, -np.inf, np.inf, np.nan, np.nan], dtype=LD)
        R.bars, R.abs_terms, R.peak = np.zeros(8, dtype=LD), np.zeros(4, dtype=LD), np.zeros(4, dtype=LD)
        R.integral, R.ibar, R.poisoned = np.zeros(0, dtype=LD), np.zeros(0, dtype=LD), False
        out.append(R)
        if R.count == 0:
            continue
        tdir = d / ell
        nu = np.array([-tdir[1], tdir[0]], dtype=LD) if dim == 2 else None
        dt = t1 - t0
        tq = np.concatenate([t0[:, None] + gx[None, :] * dt[:, None], t0[:, None], t1[:, None]], axis=1)      # (m, N + 2)
        pts = a[i].astype(LD)[None, None, :] + tq[:, :, None] * d[None, None, :]
        dy = np.maximum(dt0, dt1)[:, None] * ell + 4 * EPS * M.xmax
        xe, ze = M.X[e], Z[e]
        v, g, S, G, h = SR.evaluate(dim, k, xe, ze, pts)
        R.poisoned = not (np.isfinite(v).all() and np.isfinite(g).all())
        vbar = SR._value_bar(S, G, g, h, M.xmax, dy)
        # the change of the gradient over dy, along the segment (the only direction a piece end moves a point in) and across
        shift = (dy / ell)[:, :, None] * d[None, None, :]
        _, gp, _, _, _ = SR.evaluate(dim, k, xe, ze, pts + shift)
        _, gm, _, _, _ = SR.evaluate(dim, k, xe, ze, pts - shift)
        dg = 32 * EPS * (M.xmax / h[:, None] + 1) * G / h[:, None] + np.sqrt(np.maximum(((gp - g) ** 2).sum(-1), ((gm - g) ** 2).sum(-1)))
        sg = SR.flux(g, p)
        an = np.sqrt((g * g).sum(-1))
        with np.errstate(all="ignore"):
            lip = np.where(an > 0, an ** LD(p - 2.0), LD(0)) if p != 2.0 else np.ones_like(an)
        sbar = 2 * (1 + abs(LD(p) - 2)) * lip * dg + 4 * EPS * np.sqrt((sg * sg).sum(-1))
        st = (sg * tdir).sum(-1)
        sn = (sg * nu).sum(-1) if dim == 2 else np.zeros_like(st)
        om = gw[None, :] * (dt * ell)[:, None]
        inner = slice(0, N)
        lens = dt * ell
        endbar = ell * (dt0 + dt1)
        n = R.count + 4
        R.integral = (om * v[:, inner]).sum(axis=1)
        R.ibar = (om * vbar[:, inner]).sum(axis=1) + endbar * np.abs(v).max(axis=1) + (N + 4) * EPS * (om * np.abs(v[:, inner])).sum(axis=1)
        terms = [lens, om * v[:, inner], om * st[:, inner], om * sn[:, inner]]
        R.abs_terms = np.array([np.abs(t).sum() for t in terms], dtype=LD)
        R.peak = np.array([1, np.abs(v).max(), np.abs(st).max(), np.abs(sn).max()], dtype=LD)
        R.rows[0] = lens.sum()
        R.bars[0] = endbar.sum() + n * EPS * R.abs_terms[0]
        for c, (term, pbar, peak) in enumerate(((terms[1], vbar, np.abs(v)), (terms[2], sbar, np.abs(st)), (terms[3], sbar, np.abs(sn))), start=1):
            R.rows[c] = term.sum()
            R.bars[c] = (om * pbar[:, inner]).sum() + (endbar * peak.max(axis=1)).sum() + (n + N) * EPS * R.abs_terms[c]
        if dim == 3:
            R.bars[3] = 0
        R.rows[4], R.rows[5] = v.max(), v.min()
        R.bars[4] = R.bars[5] = vbar.max()
        R.rows[6], R.rows[7] = t0.min(), t1.max()
        R.bars[6], R.bars[7] = dt0.max(), dt1.max()
        if R.poisoned:
            R.rows[1:6] = np.nan
    return out
