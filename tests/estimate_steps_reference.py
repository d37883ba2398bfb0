"""Independent numpy / math.fsum restatement of the error indicators of the steps of a parabolic run, the
yardstick of test_estimate_steps_host.py and test_gpu_estimate_steps.py.  Not a test.  estimate_reference.py and
energy_reference.py are imported unchanged: the facet tables, the jump and Neumann terms and the flux are theirs.

Step k = 1..B of the snapshots u_0 .. u_B at the times ts, h_k = ts[k] - ts[k-1] (the double the library forms):
  Sigma^m = energy_reference.flux of snapshot m;
  d_i = (u^k_i - u^(k-1)_i) / h_k, in doubles as the contract words it (a subtraction, then a division);
  rho_i = the fsum of f_k,i, d_i and the products -lambda entry Sigma^k of the geometry's own dx / dy / dz rows; vol as in
  estimate_reference; jump and neu ARE estimate_reference.indicators on Sigma^k with the step's Neumann data;
  tim_e = fsum_i w_i (sqrt of the fsum of the squares of Sigma^k_i - Sigma^(k-1)_i)^r;  rate = fsum_i w_i |d_i|^r.
Magnitude: next to each value the same expression with every product and summand replaced by its absolute value before the
power: (|f| + |d| + sum |lambda entry Sigma|)^r for a node, (sqrt of the fsum of (|Sigma^k| + |Sigma^(k-1)|)^2)^r for a time
term; the rate has no cancellation behind d and is its own magnitude.
Bars: KTOL = 1e-12 times the magnitude for a sum or a per-element value, KTOL relative for a maximum.  A non-finite u, Sigma, f
or h makes what it feeds NaN; NaN patterns must agree.
One maximum can vanish by cancellation: max_e tim_e where the fluxes of both snapshots agree in every element (p = 1 in 1-D, where
Sigma is the sign of the slope: the library's g / a is exactly +-1 and its difference exactly 0, while flux() here rounds
(1 / a) g and leaves a difference of an ulp).  Where this yardstick's own maximum is no larger than KTOL times the largest tim
magnitude it is rounding noise of the yardstick, a relative bar means nothing, and the library's value is held to that same
KTOL times the magnitude instead -- the rule of the zero-residual closed forms of test_estimate_host.py."""
import math

import numpy as np

import energy_reference as ER
import estimate_reference as XR

KTOL = XR.KTOL
ROW1 = ("sum tim", "sum rate", "zero", "max tim", "max |d|")


def _rows(a, B, shape, what):
    """None, or `a` as B rows: one row for every step, or a row per step."""
    if a is None:
        return None
    a = np.asarray(a, dtype=float)
    if a.shape == shape:
        return [a] * B
    assert a.shape == (B,) + shape, (what, a.shape)
    return list(a)


def step_indicators(ops, w, F, I, fields, ts, p, f=None, r=2.0, scale=1.0, h=None, mask=None):
    """dict(parts (B, nel, 4), parts_mag, totals (B, 2, 5), totals_mag (B, 2, 3), J, J_mag, N, N_mag (B, .), sigma (B + 1, n, dim))
    of the columns `fields` (B + 1, n)."""
    fields = [np.asarray(u, dtype=float) for u in fields]
    ts = np.asarray(ts, dtype=float)
    B, n = len(fields) - 1, len(fields[0])
    assert len(ts) == B + 1 and B >= 1
    hs = ts[1:] - ts[:-1]
    pn = np.broadcast_to(np.asarray(p, dtype=float), (n,))
    lam = float(scale)
    good_p = np.isfinite(pn) & (pn >= 1.0)
    sigma = [ER.flux(ops, u, p) for u in fields]
    dim = sigma[0].shape[1]
    nf, q = F["nodes"].shape
    fr, hr = _rows(f, B, (n,), "f"), _rows(h, B, (nf, q), "h")
    csr = [op.tocsr() for op in ops]
    table = I["element_facets"]
    nel = table.shape[0]
    block = n // nel
    out = dict(parts=np.zeros((B, nel, 4)), parts_mag=np.zeros((B, nel, 4)), totals=np.zeros((B, 2, 5)), totals_mag=np.zeros((B, 2, 3)),
               J=[], J_mag=[], N=[], N_mag=[], sigma=np.stack(sigma), tim_mag_max=np.zeros(B))
    for k in range(1, B + 1):
        sk, so = sigma[k], sigma[k - 1]
        Y = XR.indicators(ops, w, F, I, fields[k], p, f=None, r=r, scale=lam, h=None if hr is None else hr[k - 1], mask=mask, sigma=sk)
        fv = np.zeros(n) if fr is None else fr[k - 1]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            d = (fields[k] - fields[k - 1]) / hs[k - 1]
            d = np.where(np.isfinite(fields[k]) & np.isfinite(fields[k - 1]) & np.isfinite(hs[k - 1]), d, np.nan)
            term, term_mag, tim, tim_mag = np.empty(n), np.empty(n), np.empty(n), np.empty(n)
            for i in range(n):
                prods = []
                for c in range(dim):
                    lo, hi = csr[c].indptr[i], csr[c].indptr[i + 1]
                    prods.extend(csr[c].data[lo:hi] * sk[csr[c].indices[lo:hi], c])
                prods = np.asarray(prods)
                if good_p[i] and np.isfinite(fv[i]) and np.isfinite(prods).all() and not np.isnan(d[i]):
                    term[i] = w[i] * abs(math.fsum([fv[i], d[i]] + list(-lam * prods))) ** r
                    term_mag[i] = w[i] * math.fsum([abs(fv[i]), abs(d[i])] + list(np.abs(lam * prods))) ** r
                else:
                    term[i] = term_mag[i] = np.nan
                if np.isfinite(sk[i]).all() and np.isfinite(so[i]).all():
                    tim[i] = w[i] * math.sqrt(math.fsum((a - b) * (a - b) for a, b in zip(sk[i], so[i]))) ** r
                    tim_mag[i] = w[i] * math.sqrt(math.fsum((abs(a) + abs(b)) ** 2 for a, b in zip(sk[i], so[i]))) ** r
                else:
                    tim[i] = tim_mag[i] = np.nan
            rate = w * np.abs(d) ** r
            P, G = out["parts"][k - 1], out["parts_mag"][k - 1]
            P[:, 1:3], G[:, 1:3] = Y["parts"][:, 1:3], Y["parts_mag"][:, 1:3]
            for e in range(nel):
                sl = slice(e * block, (e + 1) * block)
                he = math.fsum(w[sl]) ** (1.0 / dim)
                P[e, 0], G[e, 0] = he ** r * math.fsum(term[sl]), he ** r * math.fsum(term_mag[sl])
                P[e, 3], G[e, 3] = math.fsum(tim[sl]), math.fsum(tim_mag[sl])
            eta = P[:, :3].sum(axis=1)
            T = out["totals"][k - 1]
            T[0] = (math.fsum(P[:, 0]), math.fsum(P[:, 1]), math.fsum(P[:, 2]), np.nan if np.isnan(eta).any() else eta.max(), Y["totals"][4])
            T[1] = (math.fsum(P[:, 3]), math.fsum(rate), 0.0, np.nan if np.isnan(P[:, 3]).any() else P[:, 3].max(),
                    np.nan if np.isnan(d).any() else np.abs(d).max())
            out["totals_mag"][k - 1, 0] = [math.fsum(G[:, c]) for c in range(3)]
            out["totals_mag"][k - 1, 1] = (math.fsum(G[:, 3]), T[1, 1], 0.0)
            out["tim_mag_max"][k - 1] = np.nanmax(G[:, 3]) if not np.isnan(G[:, 3]).all() else 0.0
        for key in ("J", "J_mag", "N", "N_mag"):
            out[key].append(Y[key])
    for key in ("J", "J_mag", "N", "N_mag"):
        out[key] = np.stack(out[key])
    return out


def check(name, Y, parts=None, totals=None, J=None, N=None, tol=KTOL):
    """Library results against the yardstick Y = step_indicators(...); prints every figure first."""
    B = len(Y["parts"])
    if J is not None:
        XR._within(name, "J", np.asarray(J).reshape(Y["J"].shape), Y["J"], tol * Y["J_mag"])
    if N is not None:
        XR._within(name, "N", np.asarray(N).reshape(Y["N"].shape), Y["N"], tol * Y["N_mag"])
    if parts is not None:
        XR._within(name, "parts", np.asarray(parts).reshape(B, -1, 4), Y["parts"], tol * Y["parts_mag"])
    if totals is not None:
        T = np.asarray(totals).reshape(B, 2, 5)
        XR._within(name, "sums", T[:, :, :3], Y["totals"][:, :, :3], tol * Y["totals_mag"])
        bar = tol * np.abs(Y["totals"][:, :, 3:])
        noise = tol * Y["tim_mag_max"]
        bar[:, 1, 0] = np.where(Y["totals"][:, 1, 3] <= noise, noise, bar[:, 1, 0])      # a maximum of the yardstick that is its own noise
        XR._within(name, "maxima", T[:, :, 3:], Y["totals"][:, :, 3:], bar)


def time_sum(Y, ts):
    """sum_k h_k time_k and its terms h_k time_k, by fsum: total_time^r of the run."""
    hs = np.diff(np.asarray(ts, dtype=float))
    terms = hs * Y["totals"][:, 1, 0]
    return math.fsum(terms), terms


def host_estimate_steps(lib, g, fields, ts, p, f=None, u=0, r=2.0, scale=1.0, h=None, mask=None, rc_only=False, S=None, B=None,
                        f_rows=None, h_rows=None):
    """mgb_geo_estimate_steps_host on an XR.Mesh: `fields` a list of (n, S) arrays, p a scalar or an (n,) array, f None, (n,) or
    (B, n), h None, (nf, q) or (B, nf, q).  Returns dict(parts, J, N, sigma, totals); outputs prefilled so that an unwritten
    word shows."""
    import ctypes as C
    from mgb_amd import _lib
    zs = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    B = len(zs) - 1 if B is None else B
    nb = max(len(zs) - 1, 1)
    S = zs[0].shape[1] if S is None else S
    table = (_lib.c_dbl_p * len(zs))(*[_lib.dptr(z) for z in zs])
    tv = _lib.f64(ts)
    pn = None if np.isscalar(p) else _lib.f64(p)
    p0 = float(p) if pn is None else float(pn[0])
    fa = None if f is None else _lib.f64(f).reshape(-1, g.n)
    ha = None if h is None else _lib.f64(h).reshape(-1, g.nf, g.q)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    parts, J, N = np.full((nb, g.nel, 4), 7.0), np.full((nb, g.nif), 7.0), np.full((nb, g.nf), 7.0)
    sigma, out = np.full((nb + 1, g.n, g.dim), 7.0), np.full((nb, 2, 5), 7.0)
    rc = lib.mgb_geo_estimate_steps_host(g.handle, B, table, _lib.dptr(tv), S, u, p0, _lib.dptr(pn), _lib.dptr(fa),
                                         (1 if fa is None else fa.shape[0]) if f_rows is None else f_rows, float(r), float(scale),
                                         _lib.dptr(ha), (1 if ha is None else ha.shape[0]) if h_rows is None else h_rows, _lib.u8ptr(m),
                                         _lib.dptr(sigma), _lib.dptr(parts), _lib.dptr(J), _lib.dptr(N), _lib.dptr(out))
    if rc_only:
        return rc, parts, out
    assert rc == 0, lib.mgb_last_error()
    return dict(parts=parts, J=J, N=N, sigma=sigma, totals=out)
