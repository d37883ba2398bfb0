"""Independent numpy / math.fsum restatement of the residual error indicators, the yardstick of
test_estimate_host.py and test_gpu_estimate.py.  Not a test.

Interior facets: found here from geometry.subspaces["full"][-1] by dof SETS (a dict keyed by the sorted corner dofs, not the
library's key sort): a facet whose dofs occur in exactly two elements.  The first side is the smaller (element, local facet);
facets come in ascending order of their first side; the rows of the second side are matched to the first side's by dof; weights,
normal, measure and centre are those of the first side by the formulas of boundary_reference.  The element -> facet table is
rebuilt from the two facet lists.
Indicator: Sigma = energy_reference.flux; the divergence at node i is the fsum over k and over the row of the geometry's own
dx / dy / dz operator of (entry x Sigma_k); rho = f - lambda div; J_Fj = lambda_a (Sigma_a - Sigma_b) . n as one fsum over the 2 dim
products; N_Fj = lambda_i Sigma_i . n + h likewise; every sum above them is an fsum, so the yardstick has no summation error.
Magnitude: next to each value the same expression with every product and every summand replaced by its absolute value before
the power -- (|f_i| + sum |lambda entry Sigma|)^r for a node, (sum_k |lambda Sigma_a,k n_k| + sum_k |lambda Sigma_b,k n_k|)^r for a
jump, (sum_k |lambda Sigma_i,k n_k| + |h|)^r for a Neumann node -- carried through the same weights and sums.
Bars: KTOL = 1e-12 (the project's kernel-parity bar) times the magnitude for a sum or a per-element value, KTOL relative for a
maximum.  A non-finite Sigma, f or h makes what it feeds NaN; NaN patterns must agree."""
import math

import numpy as np

import boundary_reference as BR
import energy_reference as ER

KTOL = ER.KTOL
COLS = ("sum vol", "sum jump", "sum neu", "max eta^r", "max |J|")
R_VALUES = (1.0, 2.0, 1.5)
# name -> (kind, L, k, K, interior facets)
SHAPES = {"fem1d_L1": ("fem1d", 1, None, None, 1), "fem1d_L2": ("fem1d", 2, None, None, 3), "fem1d_L3": ("fem1d", 3, None, None, 7),
          "fem2d_L2": ("fem2d", 2, None, None, 8), "fem2d_L3": ("fem2d", 3, None, None, 40),
          "fem2d_L2_Lshape": ("fem2d", 2, None, BR.L_SHAPE, 28), "fem2d_L1_tri": ("fem2d", 1, None, BR.L_SHAPE[:3], 0),
          "fem2d_L4": ("fem2d", 4, None, None, 176),
          "fem3d_L1_k3": ("fem3d", 1, 3, None, 0), "fem3d_L2_k1": ("fem3d", 2, 1, None, 12), "fem3d_L2_k2": ("fem3d", 2, 2, None, 12),
          "fem3d_L2_k3": ("fem3d", 2, 3, None, 12),
          # every interior face of the cube at L = 2 lies on a coordinate plane, where |x|^2 has no normal flux: the zero-residual
          # closed form needs faces off those planes for its magnitudes to be magnitudes
          "fem3d_L3_k2": ("fem3d", 3, 2, None, 144), "fem3d_L3_k3": ("fem3d", 3, 3, None, 144)}


def _facet_geometry(xe, dim, k, lf, rows):
    nrm = np.zeros(dim)
    if dim == 2:
        a, m, b = (xe[r] for r in rows)
        d = b - a
        length = math.hypot(d[0], d[1])
        nrm[:] = (d[1] / length, -d[0] / length)
        if nrm @ (m - xe[:3].mean(axis=0)) < 0:
            nrm = -nrm
        return [length * c for c in BR.NEWTON_COTES[2]], nrm, length, m
    lo, hi = xe[0], xe[-1]
    axis = 0 if dim == 1 else lf // 2
    mid = 0.5 * (lo + hi)
    nrm[axis] = 1.0 if xe[rows[0], axis] > mid[axis] else -1.0
    centre = mid.copy()
    centre[axis] = xe[rows[0], axis]
    measure = float(np.prod([abs(hi[d] - lo[d]) for d in range(dim) if d != axis]))
    nc = BR.NEWTON_COTES[k]
    w = [1.0] if dim == 1 else [measure * (nc[a] * nc[b]) for b in range(k + 1) for a in range(k + 1)]
    return w, nrm, measure, centre


def interior_facets(geometry, F=None):
    """dict(elements, nodes, weights, normal, measure, centre, element_facets) of a native or a device Geometry."""
    full = geometry.subspaces["full"][-1]
    full = getattr(full, "host", full).tocsr()
    x = geometry.x if isinstance(geometry.x, np.ndarray) else geometry.x.to_numpy()
    n = full.shape[0]
    x = np.asarray(x, dtype=float).reshape(n, -1)
    dof = full.indices
    dim, block = x.shape[1], geometry.discretization["block"]
    k = {1: 1, 2: 0}.get(dim) if dim < 3 else round(block ** (1 / 3)) - 1
    lfs = BR.local_facets(dim, k)
    nel, nlf, q = n // block, len(lfs), len(lfs[0][0])
    groups = {}
    for e in range(nel):
        for lf, (rows, corners) in enumerate(lfs):
            groups.setdefault(frozenset(int(dof[e * block + rows[c]]) for c in corners), set()).add((e, lf))
    assert all(len(v) <= 2 for v in groups.values())
    pairs = sorted(tuple(sorted(v)) for v in groups.values() if len(v) == 2)
    out = dict(elements=[], nodes=[], weights=[], normal=[], measure=[], centre=[])
    table = np.full((nel, nlf), np.iinfo(np.int32).min, dtype=np.int64)
    for f, ((ea, la), (eb, lb)) in enumerate(pairs):
        ra = [ea * block + r for r in lfs[la][0]]
        by_dof = {}
        for r in lfs[lb][0]:
            assert int(dof[eb * block + r]) not in by_dof
            by_dof[int(dof[eb * block + r])] = eb * block + r
        rb = [by_dof[int(dof[i])] for i in ra]
        w, nrm, measure, centre = _facet_geometry(x[ea * block:(ea + 1) * block], dim, k, la, lfs[la][0])
        out["elements"].append((ea, eb))
        out["nodes"].append((ra, rb))
        out["weights"].append(w)
        out["normal"].append(nrm)
        out["measure"].append(measure)
        out["centre"].append(centre)
        table[ea, la] = table[eb, lb] = f
    F = BR.facets(geometry) if F is None else F
    lf_of = {tuple(rows): lf for lf, (rows, _) in enumerate(lfs)}
    for f, (e, nodes) in enumerate(zip(F["element"], F["nodes"])):
        table[e, lf_of[tuple(int(i) - e * block for i in nodes)]] = -1 - f
    shapes = dict(elements=(0, 2), nodes=(0, 2, q), weights=(0, q), normal=(0, dim), measure=(0,), centre=(0, dim))
    res = {key: (np.array(v) if v else np.zeros(shapes[key])) for key, v in out.items()}
    res["element_facets"] = table
    return res


def indicators(ops, w, F, I, uv, p, f=None, r=2.0, scale=None, h=None, mask=None, sigma=None):
    """dict(parts (nel, 3), parts_mag, totals (5,), totals_mag (3,), J, J_mag, N, N_mag, sigma) of the column uv (n,)."""
    n = len(uv)
    sigma = ER.flux(ops, uv, p) if sigma is None else sigma
    dim = sigma.shape[1]
    pn = np.broadcast_to(np.asarray(p, dtype=float), (n,))
    lam = pn if scale is None else np.full(n, float(scale))
    good_p = np.isfinite(pn) & (pn >= 1.0)
    fv = np.zeros(n) if f is None else np.asarray(f, dtype=float)
    table = I["element_facets"]
    nel, nlf = table.shape
    block = n // nel
    csr = [op.tocsr() for op in ops]
    term, term_mag = np.empty(n), np.empty(n)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            prods = []
            for k in range(dim):
                lo, hi = csr[k].indptr[i], csr[k].indptr[i + 1]
                prods.extend(csr[k].data[lo:hi] * sigma[csr[k].indices[lo:hi], k])
            prods = np.asarray(prods)
            if not (good_p[i] and np.isfinite(fv[i]) and np.isfinite(prods).all()):
                term[i] = term_mag[i] = np.nan
                continue
            rho = math.fsum([fv[i]] + list(-lam[i] * prods))
            term[i] = w[i] * abs(rho) ** r
            term_mag[i] = w[i] * math.fsum([abs(fv[i])] + list(np.abs(lam[i] * prods))) ** r

        def facet_node(rows, signs, nrm, extra, lam_row):
            prods = [s * lam[lam_row] * sigma[i, k] * nrm[k] for i, s in zip(rows, signs) for k in range(dim)] + extra
            if not (good_p[lam_row] and np.isfinite(prods).all()):
                return np.nan, np.nan
            return abs(math.fsum(prods)), math.fsum(np.abs(prods))

        nif, q = I["weights"].shape
        J, J_mag, Jabs = np.zeros(nif), np.zeros(nif), np.zeros((nif, q))
        for fi in range(nif):
            vals = [facet_node((I["nodes"][fi, 0, j], I["nodes"][fi, 1, j]), (1.0, -1.0), I["normal"][fi], [], I["nodes"][fi, 0, j])
                    for j in range(q)]
            Jabs[fi] = [v[0] for v in vals]
            J[fi] = math.fsum(I["weights"][fi, j] * vals[j][0] ** r for j in range(q))
            J_mag[fi] = math.fsum(I["weights"][fi, j] * vals[j][1] ** r for j in range(q))
        nf = len(F["element"])
        N, N_mag = np.zeros(nf), np.zeros(nf)
        if h is not None:
            hv = np.asarray(h, dtype=float).reshape(nf, q)
            sel = np.ones(nf, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
            for fb in np.flatnonzero(sel):
                vals = [facet_node((F["nodes"][fb, j],), (1.0,), F["normal"][fb], [hv[fb, j]], F["nodes"][fb, j]) for j in range(q)]
                N[fb] = math.fsum(F["weights"][fb, j] * vals[j][0] ** r for j in range(q))
                N_mag[fb] = math.fsum(F["weights"][fb, j] * vals[j][1] ** r for j in range(q))
        parts, mag = np.zeros((nel, 3)), np.zeros((nel, 3))
        for e in range(nel):
            sl = slice(e * block, (e + 1) * block)
            he = math.fsum(w[sl]) ** (1.0 / dim)
            jf = [t for t in table[e] if t >= 0]
            bf = [-1 - t for t in table[e] if t < 0]
            parts[e] = (he ** r * math.fsum(term[sl]), 0.5 * he * math.fsum(J[jf]), he * math.fsum(N[bf]))
            mag[e] = (he ** r * math.fsum(term_mag[sl]), 0.5 * he * math.fsum(J_mag[jf]), he * math.fsum(N_mag[bf]))
    eta = parts.sum(axis=1)
    totals = np.array([math.fsum(parts[:, 0]), math.fsum(parts[:, 1]), math.fsum(parts[:, 2]), np.max(eta) if nel else 0.0,
                       np.max(Jabs) if nif else 0.0])
    if np.isnan(eta).any():
        totals[3] = np.nan
    if np.isnan(Jabs).any():
        totals[4] = np.nan
    totals_mag = np.array([math.fsum(mag[:, 0]), math.fsum(mag[:, 1]), math.fsum(mag[:, 2])])
    return dict(parts=parts, parts_mag=mag, totals=totals, totals_mag=totals_mag, J=J, J_mag=J_mag, N=N, N_mag=N_mag, sigma=sigma)


def _within(name, what, got, want, bar):
    got, want, bar = (np.asarray(v, dtype=float) for v in (got, want, bar))
    assert got.shape == want.shape, (name, what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: %s NaN pattern differs at %r" % (name, what, np.argwhere(np.isnan(got) != nan)[:5])
    gap = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want)))
    over = gap - np.where(nan, 0.0, bar)
    if gap.size:
        j = np.unravel_index(int(over.argmax()), gap.shape)
        print("%s: %-10s off by %.3e (bar %.3e, value %.17g) at %r" % (name, what, gap[j], np.where(nan, 0.0, bar)[j], want[j], j))
    assert (over <= 0.0).all(), (name, what, np.argwhere(over > 0.0)[:5])


def check(name, Y, parts=None, totals=None, J=None, N=None, tol=KTOL):
    """Library results against the yardstick Y = indicators(...); prints every figure first."""
    if J is not None:
        _within(name, "J", J, Y["J"], tol * Y["J_mag"])
    if N is not None:
        _within(name, "N", N, Y["N"], tol * Y["N_mag"])
    if parts is not None:
        _within(name, "parts", np.asarray(parts).reshape(-1, 3), Y["parts"], tol * Y["parts_mag"])
    if totals is not None:
        _within(name, "sums", np.asarray(totals)[:3], Y["totals"][:3], tol * Y["totals_mag"])
        _within(name, "maxima", np.asarray(totals)[3:], Y["totals"][3:], tol * np.abs(Y["totals"][3:]))


def coarse(parts, dim, L):
    """(eta^r summed per coarse element by fsum, the magnitudes likewise) from parts / parts_mag stacked as (nel, 3)."""
    group = (2 ** dim) ** (L - 1)
    return np.array([math.fsum(g.ravel()) for g in np.asarray(parts).reshape(-1, group, 3)])


class Mesh(BR.HostMesh):
    """BR.HostMesh of one of SHAPES with the yardstick's interior facets."""

    def __init__(self, name):
        kind, L, k, K, nif = SHAPES[name]
        super().__init__(kind=kind, L=L, k=k, K=K)
        self.name = name
        self.I = interior_facets(self.py, self.F)
        self.nif, self.nel = len(self.I["elements"]), self.n // self.block


def host_interior(lib, g):
    """mgb_geo_interior_dims / _get on a HostMesh -> dict like interior_facets()."""
    import ctypes as C
    from mgb_amd import _lib
    nif, q, dim, nel, nlf = (C.c_int() for _ in range(5))
    assert lib.mgb_geo_interior_dims(g.handle, C.byref(nif), C.byref(q), C.byref(dim), C.byref(nel), C.byref(nlf)) == 0, lib.mgb_last_error()
    nif, q, dim, nel, nlf = nif.value, q.value, dim.value, nel.value, nlf.value
    out = dict(elements=np.full((nif, 2), -7, dtype=np.int32), nodes=np.full((nif, 2, q), -7, dtype=np.int32), weights=np.full((nif, q), 7.0),
               normal=np.full((nif, dim), 7.0), measure=np.full(nif, 7.0), centre=np.full((nif, dim), 7.0),
               element_facets=np.full((nel, nlf), 7, dtype=np.int32))
    rc = lib.mgb_geo_interior_get(g.handle, _lib.iptr(out["elements"]), _lib.iptr(out["nodes"]), _lib.dptr(out["weights"]),
                                  _lib.dptr(out["normal"]), _lib.dptr(out["measure"]), _lib.dptr(out["centre"]),
                                  _lib.iptr(out["element_facets"]))
    assert rc == 0, lib.mgb_last_error()
    return out


def host_estimate(lib, g, z, p, f=None, u=0, r=2.0, scale=None, h=None, mask=None, rc_only=False, S=None):
    """mgb_geo_estimate_host on a Mesh: z (n, S), p a scalar or an (n,) array.  Returns dict(parts, J, N, sigma, totals);
    outputs prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    z = _lib.f64(z).reshape(g.n, -1)
    S = z.shape[1] if S is None else S
    pn = None if np.isscalar(p) else _lib.f64(p)
    p0 = float(p) if pn is None else float(pn[0])
    fa = None if f is None else _lib.f64(f)
    ha = None if h is None else _lib.f64(h)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    parts, J, N = np.full((g.nel, 3), 7.0), np.full(g.nif, 7.0), np.full(g.nf, 7.0)
    sigma, out = np.full((g.n, g.dim), 7.0), np.full(5, 7.0)
    rc = lib.mgb_geo_estimate_host(g.handle, _lib.dptr(z), S, u, p0, _lib.dptr(pn), _lib.dptr(fa), float(r), 0 if scale is None else 1,
                                   1.0 if scale is None else float(scale), _lib.dptr(ha), _lib.u8ptr(m), _lib.dptr(parts), _lib.dptr(J),
                                   _lib.dptr(N), _lib.dptr(sigma), _lib.dptr(out))
    if rc_only:
        return rc, parts, out
    assert rc == 0, lib.mgb_last_error()
    return dict(parts=parts, J=J, N=N, sigma=sigma, totals=out)


# ------------------------------------------------------------------------------------------------ triangle lists
def triangles(K):
    return np.asarray(K, dtype=float).reshape(-1, 3, 2)


def orientation(K):
    T = triangles(K)
    a, b = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    return a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]      # twice the signed area


def smallest_angle(K):
    T = triangles(K)
    best = math.pi
    for t in T:
        for i in range(3):
            a, b = t[(i + 1) % 3] - t[i], t[(i + 2) % 3] - t[i]
            best = min(best, math.atan2(abs(a[0] * b[1] - a[1] * b[0]), a @ b))
    return best


def check_conforming(K):
    """Every edge is shared by at most two triangles with identical end points, and no vertex lies inside another triangle's
    edge."""
    T = triangles(K)
    edges = {}
    for t in T:
        for i in range(3):
            key = tuple(sorted((tuple(t[i]), tuple(t[(i + 1) % 3]))))
            edges[key] = edges.get(key, 0) + 1
    assert max(edges.values()) <= 2
    verts = np.array(sorted({tuple(v) for t in T for v in t}))
    for (a, b) in edges:
        a, b = np.array(a), np.array(b)
        d = b - a
        rel = verts - a
        cross = rel[:, 0] * d[1] - rel[:, 1] * d[0]
        s = (rel @ d) / (d @ d)
        hanging = (np.abs(cross) <= 1e-12 * (d @ d)) & (s > 1e-12) & (s < 1 - 1e-12)
        assert not hanging.any(), (a, b, verts[hanging])


def dorfler_ok(values, marked, theta):
    """The marked set reaches theta of the total, and without its last index it does not (sums as mark() takes them)."""
    v = np.asarray(values, dtype=float)
    total = np.cumsum(np.sort(v)[::-1])[-1] if v.size else 0.0
    if len(marked) == 0:
        return not total > 0.0
    cs = np.cumsum(v[np.asarray(marked)])
    return bool(cs[-1] >= theta * total and (len(marked) == 1 or cs[-2] < theta * total))
