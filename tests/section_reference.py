"""Independent numpy restatement, in np.longdouble, of the plane-section rule of include/mgb_hip.h: the
yardstick of test_section_reference.py, test_section_host.py and test_gpu_sections.py.  Not a test.  It takes x, z, the
dimension, the degree k, planes and p and shares no code with the library: the corners, the side function, the marching
cases, the orientation, the Gauss rules (found here by Newton's method on the Legendre recurrence), the P2 + bubble and the
tensor Lagrange bases and the flux are written out again, vectorised over the cut items.  The Kuhn table, the crossing with
its bar and the oriented triangle are those of the isosurface yardstick (isosurface_reference.py), which is numpy as well.

ONE thing is computed in float64, in the order the rule prescribes: the side function d = (n_0 x_0 + n_1 x_1 [+ n_2 x_2]) - c.
The rule classifies a corner by d > 0 "by comparison only", so the doubles d ARE the rule; everything behind them runs in
longdouble.

Per plane it returns a Cut: rows (5,), the sums of the absolute per-point terms behind rows[0..2], the emitted pieces in
ascending item order with their items, and the bars a double-precision evaluation is held to:

  vertex   8 eps (|P_hi - P_lo|_inf + max|x|): the bar of the level sets and isosurfaces at refine = 0 -- the roundings of
           0 - d_lo, d_hi - d_lo and the division, the product and the sum that form Q.
  value    of the element's polynomial at a point y known up to dy:
             32 eps S + 8 eps (max|x| / h + 1) G + 2 |grad u|_1 dy
           S = sum_j |N_j(y)| |z_j|: the roundings of the basis and of the sum, the bar of the isosurface yardstick;
           G = sum_j sum_a |dN_j / dr_a| |z_j|, h the smallest extent of the element: the reference coordinates
           r = (y - A) / (B - A) carry the cancellation of y - A, eps max|x| / h, and their own roundings;
           the last term moves the point, first order with a factor 2 for the rest.
           At a vertex dy is the vertex bar; at a quadrature point the largest vertex bar of the piece plus 8 eps max|x|
           for the products and sums that form the point.  The bar of both maxima is the largest value bar over the
           quadrature points of the row.
  sums     1e-12 of the sum of the absolute terms (the tests' KTOL), as everywhere in the project."""
import numpy as np

import isosurface_reference as IR

LD = np.longdouble
EPS = IR.EPS


class Cut:
    """rows (5,) longdouble; abs_terms (3,); count; items (m,); piece (m, 6 or 12); bar (m, 2 or 3) per vertex; vbar (m, 2 or
    3) per vertex value; mbar: the bar of both maxima; ncut: the items that run the quadrature."""


def gauss01(n):
    """Gauss-Legendre nodes and weights on [0, 1] in longdouble: Newton on P_n from the double-precision nodes."""
    x = np.polynomial.legendre.leggauss(n)[0].astype(LD)
    for _ in range(4):
        p0, p1 = np.ones_like(x), x.copy()
        for m in range(2, n + 1):
            p0, p1 = p1, ((2 * m - 1) * x * p1 - (m - 1) * p0) / m
        dp = n * (x * p1 - p0) / (x * x - 1)
        x = x - p1 / dp
    p0, p1 = np.ones_like(x), x.copy()
    for m in range(2, n + 1):
        p0, p1 = p1, ((2 * m - 1) * x * p1 - (m - 1) * p0) / m
    dp = n * (x * p1 - p0) / (x * x - 1)
    w = 2 / ((1 - x * x) * dp * dp)
    return (x + 1) / 2, w / 2


def n_gauss(dim, k):
    return 4 if dim == 2 else {1: 3, 2: 4, 3: 6}[k]


def side(planes_row, P):
    """d at the points P (..., dim) float64, in float64 and in the order of the rule."""
    P = np.asarray(P, dtype=np.float64)
    pr = np.asarray(planes_row, dtype=np.float64)
    s = pr[0] * P[..., 0]
    for a in range(1, P.shape[-1]):
        s = s + pr[a] * P[..., a]
    return s - pr[-1]


def _lagrange(k, f):
    """values and derivatives (..., k + 1) of the Lagrange basis on the nodes j / k of [0, 1] at f."""
    t = k * f
    val, der = np.ones(f.shape + (k + 1,), dtype=LD), np.zeros(f.shape + (k + 1,), dtype=LD)
    for j in range(k + 1):
        for i in range(k + 1):
            if i != j:
                val[..., j] *= (t - i) / LD(j - i)
        for m in range(k + 1):
            if m == j:
                continue
            q = np.full(f.shape, 1 / LD(j - m), dtype=LD)
            for i in range(k + 1):
                if i != j and i != m:
                    q = q * (t - i) / LD(j - i)
            der[..., j] += q
    return val, k * der


def evaluate(dim, k, xe, ze, pts):
    """xe (m, block, dim), ze (m, block), pts (m, q, dim), all longdouble: value (m, q), physical gradient (m, q, dim),
    S = sum |N_j| |z_j| (m, q), G = sum_j sum_a |dN_j / dr_a| |z_j| (m, q), h (m,) the smallest extent."""
    az = np.abs(ze)
    with np.errstate(invalid="ignore"):
        if dim == 2:
            v0 = xe[:, 0]
            ax, ay = (xe[:, 1] - v0).T
            bx, by = (xe[:, 2] - v0).T
            det = (ax * by - ay * bx)[:, None]
            ax, ay, bx, by = ax[:, None], ay[:, None], bx[:, None], by[:, None]
            px, py = pts[..., 0] - v0[:, None, 0], pts[..., 1] - v0[:, None, 1]
            xi, et = (px * by - py * bx) / det, (ax * py - ay * px) / det
            lam = [1 - xi - et, xi, et]
            gx, gy = [LD(-1), LD(1), LD(0)], [LD(-1), LD(0), LD(1)]
            b = lam[0] * lam[1] * lam[2]
            bxi = gx[0] * lam[1] * lam[2] + lam[0] * gx[1] * lam[2] + lam[0] * lam[1] * gx[2]
            bet = gy[0] * lam[1] * lam[2] + lam[0] * gy[1] * lam[2] + lam[0] * lam[1] * gy[2]
            N, Nx, Ny = [None] * 7, [None] * 7, [None] * 7
            for i in range(3):
                j = (i + 1) % 3
                N[i] = lam[i] * (2 * lam[i] - 1) + 3 * b
                Nx[i] = (4 * lam[i] - 1) * gx[i] + 3 * bxi
                Ny[i] = (4 * lam[i] - 1) * gy[i] + 3 * bet
                N[3 + i] = 4 * lam[i] * lam[j] - 12 * b
                Nx[3 + i] = 4 * (lam[i] * gx[j] + lam[j] * gx[i]) - 12 * bxi
                Ny[3 + i] = 4 * (lam[i] * gy[j] + lam[j] * gy[i]) - 12 * bet
            N[6], Nx[6], Ny[6] = 27 * b, 27 * bxi, 27 * bet
            N, Nx, Ny = (np.stack(a, axis=-1) for a in (N, Nx, Ny))      # (m, q, 7)
            zz = ze[:, None, :]
            v, g0, g1 = (N * zz).sum(-1), (Nx * zz).sum(-1), (Ny * zz).sum(-1)
            g = np.stack([(g0 * by - g1 * ay) / det, (-g0 * bx + g1 * ax) / det], axis=-1)
            S = (np.abs(N) * az[:, None, :]).sum(-1)
            G = ((np.abs(Nx) + np.abs(Ny)) * az[:, None, :]).sum(-1)
            edge = np.maximum(np.maximum(np.hypot(ax, ay), np.hypot(bx, by)), np.hypot(bx - ax, by - ay))
            h = (np.abs(det) / edge)[:, 0]
            return v, g, S, G, h
        m1 = k + 1
        A, B = xe[:, 0], xe[:, -1]
        r = (pts - A[:, None, :]) / (B - A)[:, None, :]
        val, der = _lagrange(k, r)      # (m, q, 3, m1)
        zc, ac = ze.reshape(-1, m1, m1, m1), az.reshape(-1, m1, m1, m1)      # axes c, b, a
        ein = lambda fa, fb, fc, w: np.einsum("mqa,mqb,mqc,mcba->mq", fa, fb, fc, w)
        v = ein(val[:, :, 0], val[:, :, 1], val[:, :, 2], zc)
        g = np.stack([ein(der[:, :, 0], val[:, :, 1], val[:, :, 2], zc), ein(val[:, :, 0], der[:, :, 1], val[:, :, 2], zc),
                      ein(val[:, :, 0], val[:, :, 1], der[:, :, 2], zc)], axis=-1) / (B - A)[:, None, :]
        av, ad = np.abs(val), np.abs(der)
        S = ein(av[:, :, 0], av[:, :, 1], av[:, :, 2], ac)
        G = (ein(ad[:, :, 0], av[:, :, 1], av[:, :, 2], ac) + ein(av[:, :, 0], ad[:, :, 1], av[:, :, 2], ac)
             + ein(av[:, :, 0], av[:, :, 1], ad[:, :, 2], ac))
        return v, g, S, G, np.abs(B - A).min(axis=1)


def flux(g, p):
    """sigma = |g|^(p-2) g, 0 where g = 0."""
    if p == 2.0:
        return g
    a = np.sqrt((g * g).sum(-1))[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = g / a if p == 1.0 else a ** LD(p - 2.0) * g
    return np.where(a == 0, LD(0), s)


def _value_bar(S, G, g, h, xmax, dy):
    return 32 * EPS * S + 8 * EPS * (xmax / h[:, None] + 1) * G + 2 * np.abs(g).sum(-1) * dy


def _pieces(dim, k, x, plane, xmax):
    """The geometry of one plane: items (m,), vertices (m, nv, dim) longdouble, bars (m, nv), in output order."""
    cross = IR._Cross(LD(0), xmax, 0)
    zero = lambda P: np.zeros(P.shape[0], dtype=LD)
    if dim == 2:
        P64 = x.reshape(-1, 7, 2)[:, :3]
        d = side(plane, P64)
        up = d > 0
        kab = up.sum(axis=1)
        cut = np.nonzero((kab == 1) | (kab == 2))[0]
        one = kab[cut] == 1
        L = np.where(one, up[cut].argmax(axis=1), up[cut].argmin(axis=1))
        o1 = (L + 1) % 3
        o2 = (o1 + 1) % 3
        P, dv = P64[cut].astype(LD), d[cut].astype(LD)
        corner = lambda idx: (IR._pick(P, idx), IR._pick(dv, idx), zero(P))
        CL, Q, bars = corner(L), [], []
        for o in (o1, o2):
            Co = corner(o)
            sel = lambda a, b: np.where(one.reshape((-1,) + (1,) * (a.ndim - 1)), a, b)
            lo, hi = tuple(sel(a, b) for a, b in zip(Co, CL)), tuple(sel(b, a) for a, b in zip(Co, CL))
            q, b = cross(lo, hi)
            Q.append(q), bars.append(b)
        keep = ~(Q[0] == Q[1]).all(axis=1)
        above = np.where(one[:, None], CL[0], corner(o1)[0])
        e, r = Q[1] - Q[0], above - Q[0]
        swap = (e[:, 0] * r[:, 1] - e[:, 1] * r[:, 0]) < 0
        V = np.where(swap[:, None, None], np.stack([Q[1], Q[0]], axis=1), np.stack(Q, axis=1))
        bar = np.where(swap[:, None], np.stack([bars[1], bars[0]], axis=1), np.stack(bars, axis=1))
        return cut[keep], V[keep], bar[keep]
    m1 = k + 1
    nel = x.shape[0] // m1 ** 3
    box = x.reshape(nel, m1, m1, m1, 3)[:, ::k, ::k, ::k]      # (nel, 2, 2, 2, 3), axes c, b, a
    off = IR.kuhn()
    P64 = box[:, off[:, :, 2], off[:, :, 1], off[:, :, 0]].reshape(-1, 4, 3)      # item = e 6 + t
    d = side(plane, P64)
    up = d > 0
    kab = up.sum(axis=1)
    n = P64.shape[0]
    tri, bar, emit = np.zeros((n, 2, 9), dtype=LD), np.zeros((n, 2, 3), dtype=LD), np.zeros((n, 2), dtype=bool)
    cut = np.nonzero((kab == 1) | (kab == 3))[0]
    one = kab[cut] == 1
    P, dv = P64[cut].astype(LD), d[cut].astype(LD)
    corner = lambda idx: (IR._pick(P, idx), IR._pick(dv, idx), zero(P))
    L = np.where(one, up[cut].argmax(axis=1), up[cut].argmin(axis=1))
    CL, Q, bars = corner(L), [], []
    for j in range(3):
        Co = corner(IR.OTHERS[L, j])
        sel = lambda a, b: np.where(one.reshape((-1,) + (1,) * (a.ndim - 1)), a, b)
        lo, hi = tuple(sel(a, b) for a, b in zip(Co, CL)), tuple(sel(b, a) for a, b in zip(Co, CL))
        q, b = cross(lo, hi)
        Q.append(q), bars.append(b)
    tri[cut, 0], bar[cut, 0], _, emit[cut, 0] = IR._triangle(Q, bars, CL[0], one)
    cut = np.nonzero(kab == 2)[0]
    u2 = up[cut]
    P, dv = P64[cut].astype(LD), d[cut].astype(LD)
    A0, A1 = corner(u2.argmax(axis=1)), corner(3 - u2[:, ::-1].argmax(axis=1))
    B0, B1 = corner((~u2).argmax(axis=1)), corner(3 - (~u2)[:, ::-1].argmax(axis=1))
    (Q00, b00), (Q01, b01), (Q10, b10), (Q11, b11) = cross(B0, A0), cross(B1, A0), cross(B0, A1), cross(B1, A1)
    above = np.ones(len(cut), dtype=bool)
    tri[cut, 0], bar[cut, 0], _, emit[cut, 0] = IR._triangle((Q00, Q01, Q10), (b00, b01, b10), A0[0], above)
    tri[cut, 1], bar[cut, 1], _, emit[cut, 1] = IR._triangle((Q01, Q11, Q10), (b01, b11, b10), A0[0], above)
    flat = emit.reshape(-1)
    return np.repeat(np.arange(n), 2)[flat], tri.reshape(-1, 3, 3)[flat], bar.reshape(-1, 3)[flat]


def sections(x, z, dim, k, planes, p=2.0):
    """One Cut per plane for the nodal column z (n,) on the nodes x (n, dim); k: the degree of 3-D elements (ignored in 2-D)."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, dim + 1)
    assert x.ndim == 2 and x.shape[1] == dim and dim in (2, 3) and (dim == 2 or k in (1, 2, 3))
    block = 7 if dim == 2 else (k + 1) ** 3
    per = 1 if dim == 2 else 6
    xe, ze = x.reshape(-1, block, dim), z.reshape(-1, block)
    xmax = LD(np.abs(x).max())
    gx, gw = gauss01(n_gauss(dim, k))
    res = []
    for plane in planes:
        out = Cut()
        items, V, bar = _pieces(dim, k, x, plane, xmax)
        el = items // per
        xl, zl = xe[el].astype(LD), ze[el].astype(LD)
        nrm = plane[:dim].astype(LD)
        nu = nrm / np.sqrt((nrm * nrm).sum())
        if dim == 2:
            pts = V[:, None, 0] + gx[None, :, None] * (V[:, None, 1] - V[:, None, 0])
            e = V[:, 1] - V[:, 0]
            om = gw[None, :] * np.sqrt((e * e).sum(axis=1))[:, None]
        else:
            s, t = np.repeat(gx, len(gx)), np.tile(gx, len(gx))
            pts = ((1 - s)[None, :, None] * V[:, None, 0] + (s * (1 - t))[None, :, None] * V[:, None, 1]
                   + (s * t)[None, :, None] * V[:, None, 2])
            nn = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
            om = (np.repeat(gw, len(gx)) * np.tile(gw, len(gx)) * s)[None, :] * np.sqrt((nn * nn).sum(axis=1))[:, None]
        v, g, S, G, h = evaluate(dim, k, xl, zl, pts)
        vv, gv, Sv, Gv, _ = evaluate(dim, k, xl, zl, V)
        with np.errstate(invalid="ignore"):
            sn = (flux(g, p) * nu).sum(-1)
            fin = np.isfinite(v).all(axis=1) & np.isfinite(g).all(axis=(1, 2)) if len(items) else np.ones(0, dtype=bool)
        out.ncut = len(np.unique(items))
        bad = np.unique(items[~fin])      # a cut item with a non-finite point poisons the row and emits nothing
        ok = ~np.isin(items, bad)
        out.items, out.count = items[ok], int(ok.sum())
        out.piece = np.hstack([V[ok].reshape(out.count, dim * dim), vv[ok]])
        out.bar = bar[ok]
        out.vbar = _value_bar(Sv[ok], Gv[ok], gv[ok], h[ok], xmax, bar[ok])
        if len(bad):
            out.rows, out.abs_terms, out.mbar = np.full(5, np.nan, dtype=LD), np.full(3, np.nan, dtype=LD), LD(np.nan)
        elif out.count == 0:
            out.rows, out.abs_terms, out.mbar = np.array([0, 0, 0, -np.inf, -np.inf], dtype=LD), np.zeros(3, dtype=LD), LD(0)
        else:
            terms = np.stack([om, om * v, om * sn], axis=-1)
            out.rows = np.array([terms[..., 0].sum(), terms[..., 1].sum(), terms[..., 2].sum(), v.max(), (-v).max()], dtype=LD)
            out.abs_terms = np.abs(terms).sum(axis=(0, 1))
            out.mbar = _value_bar(S, G, g, h, xmax, bar.max(axis=1)[:, None] + 8 * EPS * xmax).max()
        res.append(out)
    return res
