"""Independent numpy restatement of the boundary facets of a geometry and of the boundary integrals of a nodal field (DESIGN.md
section 4h), the yardstick of test_boundary_host.py and test_gpu_boundary.py.  Not a test.

Facets: found here, in Python, from geometry.subspaces["full"][-1] (one entry 1 per row: the continuous dof of a row) and x.  A
facet of an element is a boundary facet when the sorted tuple of the dofs of its corner nodes occurs in exactly one element;
facets come in ascending (element, local facet) order.
  1-D  local nodes 0, 1; q = 1; weight 1; normal sign(x - element centre)
  2-D  edge i = local rows (i, 3 + i, (i + 1) % 3); q = 3; Simpson |e| (1/6, 4/6, 1/6); normal perpendicular to the edge with
       n . (midpoint - centroid of the own triangle) > 0
  3-D  x-, x+, y-, y+, z-, z+; the (k+1)^2 nodes of the side in ascending local index; area x tensor closed Newton-Cotes weights
       of degree k; normal +- axis by sign(face coordinate - element centre)
Integrals: sigma = |grad u|^(p-2) grad u from geometry.operators as energy_reference.flux takes it; sn = sigma . n,
t = sigma - sn n; flux = sum omega sn, trace = sum omega u, measure = sum omega (all three by math.fsum: the yardstick has no
summation error), normal_max = max |sn|, tangential_max = max |t|_2.  A selected node with a non-finite u or sigma makes all
five NaN; an empty selection gives five zeros.

Bars: flux sums cancel, so a sum is held to KTOL = 1e-12 (the project's kernel-parity bar) times its ABSOLUTE sum --
sum omega |sn|, sum omega |u|, sum omega -- and a per-facet value to KTOL times that facet's own sum omega |sn|; the maxima to
KTOL relative."""
import ctypes as C
import math

import numpy as np

import energy_reference as ER

KTOL = ER.KTOL
COLS = ("flux", "trace", "measure", "normal_max", "tangential_max")
NEWTON_COTES = {1: (1 / 2, 1 / 2), 2: (1 / 6, 4 / 6, 1 / 6), 3: (1 / 8, 3 / 8, 3 / 8, 1 / 8)}
# the L-shaped domain [-1, 1]^2 without its upper right quarter: a re-entrant corner at the origin
L_SHAPE = np.array([[-1, -1], [0, -1], [0, 0], [-1, -1], [0, 0], [-1, 0], [0, -1], [1, -1], [1, 0],
                    [0, -1], [1, 0], [0, 0], [-1, 0], [0, 0], [0, 1], [-1, 0], [0, 1], [-1, 1]], dtype=float)
# name -> (kind, L, k, K, facet nodes)
SHAPES = {"fem1d_L2": ("fem1d", 2, None, None, 2), "fem2d_L2": ("fem2d", 2, None, None, 24), "fem3d_L1_k3": ("fem3d", 1, 3, None, 96),
          "fem3d_L2_k1": ("fem3d", 2, 1, None, 96), "fem3d_L2_k3": ("fem3d", 2, 3, None, 384),
          "fem2d_L2_Lshape": ("fem2d", 2, None, L_SHAPE, 48)}


def local_facets(dim, k):
    """[(local rows in ascending local index, positions of the corner nodes among them)] per local facet."""
    if dim == 1:
        return [((0,), (0,)), ((1,), (0,))]
    if dim == 2:
        return [((i, 3 + i, (i + 1) % 3), (0, 2)) for i in range(3)]
    m1, out = k + 1, []
    for axis in range(3):
        for fixed in (0, k):
            rows, corners = [], []
            for local in range(m1 ** 3):
                idx = (local % m1, (local // m1) % m1, local // (m1 * m1))
                if idx[axis] != fixed:
                    continue
                if all(idx[d] in (0, k) for d in range(3)):
                    corners.append(len(rows))
                rows.append(local)
            out.append((tuple(rows), tuple(corners)))
    return out


def facets(geometry):
    """dict(element, nodes, weights, normal, measure, centre) of a native or a device Geometry."""
    full = geometry.subspaces["full"][-1]
    full = getattr(full, "host", full).tocsr()
    x = geometry.x if isinstance(geometry.x, np.ndarray) else geometry.x.to_numpy()
    n = full.shape[0]
    x = np.asarray(x, dtype=float).reshape(n, -1)
    assert (np.diff(full.indptr) == 1).all() and (full.data == 1.0).all()
    dof = full.indices
    dim, block = x.shape[1], geometry.discretization["block"]
    k = {1: 1, 2: 0}.get(dim) if dim < 3 else round(block ** (1 / 3)) - 1
    lfs = local_facets(dim, k)
    seen = {}
    for e in range(n // block):
        for lf, (rows, corners) in enumerate(lfs):
            key = tuple(sorted(int(dof[e * block + rows[c]]) for c in corners))
            seen.setdefault(key, []).append((e, lf))
    assert all(len(v) <= 2 for v in seen.values())
    bnd = sorted(v[0] for v in seen.values() if len(v) == 1)
    out = dict(element=[], nodes=[], weights=[], normal=[], measure=[], centre=[])
    for e, lf in bnd:
        xe = x[e * block:(e + 1) * block]
        rows = lfs[lf][0]
        nrm = np.zeros(dim)
        if dim == 2:
            a, m, b = (xe[r] for r in rows)
            d = b - a
            length = math.hypot(d[0], d[1])
            nrm[:] = (d[1] / length, -d[0] / length)
            if nrm @ (m - xe[:3].mean(axis=0)) < 0:
                nrm = -nrm
            w, measure, centre = [length * c for c in NEWTON_COTES[2]], length, m
        else:
            lo, hi = xe[0], xe[-1]
            axis = 0 if dim == 1 else lf // 2
            mid = 0.5 * (lo + hi)
            nrm[axis] = 1.0 if xe[rows[0], axis] > mid[axis] else -1.0
            centre = mid.copy()
            centre[axis] = xe[rows[0], axis]
            measure = float(np.prod([abs(hi[d] - lo[d]) for d in range(dim) if d != axis]))
            nc = NEWTON_COTES[k]
            w = [1.0] if dim == 1 else [measure * (nc[a] * nc[b]) for b in range(k + 1) for a in range(k + 1)]
        out["element"].append(e)
        out["nodes"].append([e * block + r for r in rows])
        out["weights"].append(w)
        out["normal"].append(nrm)
        out["measure"].append(measure)
        out["centre"].append(centre)
    return {key: np.array(v) for key, v in out.items()}


def boundary_flux(ops, F, uv, p, mask=None):
    """((5,) results, (3,) absolute sums behind the three sums, (nf,) per-facet flux, (nf,) per-facet absolute sums) of the
    column uv (n,)."""
    nf = len(F["element"])
    sel = np.ones(nf, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    sigma = ER.flux(ops, uv, p)
    pn = np.broadcast_to(np.asarray(p, dtype=float), uv.shape)
    rows, om, nrm = F["nodes"], F["weights"], F["normal"]
    sig = sigma[rows]                                                     # (nf, q, dim)
    sn = (sig * nrm[:, None, :]).sum(axis=2)
    t = sig - sn[:, :, None] * nrm[:, None, :]
    tn = np.sqrt((t * t).sum(axis=2))
    per_facet = np.array([math.fsum(om[f] * sn[f]) if sel[f] else 0.0 for f in range(nf)])
    per_facet_abs = np.array([math.fsum(om[f] * np.abs(sn[f])) if sel[f] else 0.0 for f in range(nf)])
    if not sel.any():
        return np.zeros(5), np.zeros(3), per_facet, per_facet_abs
    ok = np.isfinite(uv[rows[sel]]).all() and np.isfinite(sig[sel]).all() and np.isfinite(pn[rows[sel]]).all() and (pn[rows[sel]] >= 1).all()
    if not ok:
        return np.full(5, np.nan), np.full(3, np.nan), per_facet, per_facet_abs
    ub = uv[rows]
    vals = np.array([math.fsum((om[sel] * sn[sel]).ravel()), math.fsum((om[sel] * ub[sel]).ravel()), math.fsum(om[sel].ravel()),
                     np.abs(sn[sel]).max(), tn[sel].max()])
    sums = np.array([math.fsum((om[sel] * np.abs(sn[sel])).ravel()), math.fsum((om[sel] * np.abs(ub[sel])).ravel()), vals[2]])
    return vals, sums, per_facet, per_facet_abs


def check(name, got, want, sums, tol=KTOL):
    """Library results ((5,) or (B, 5)) against the yardstick's values and absolute sums; prints every figure first."""
    got, want, sums = np.atleast_2d(got), np.atleast_2d(want), np.atleast_2d(sums)
    gap = np.abs(got - want)
    bar = tol * np.concatenate([sums, np.abs(want[:, 3:])], axis=1)
    for c, col in enumerate(COLS):
        j = (gap[:, c] - bar[:, c]).argmax()
        print("%s: %-14s off by %.3e (bar %.3e, value %.17g)" % (name, col, gap[j, c], bar[j, c], want[j, c]))
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    assert (gap <= bar).all(), np.argwhere(gap > bar)


def check_facets(name, got, want, want_abs, tol=KTOL):
    gap = np.abs(got - want)
    j = (gap - tol * want_abs).argmax()
    print("%s: per facet off by %.3e (bar %.3e, value %.17g)" % (name, gap[j], tol * want_abs[j], want[j]))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (gap <= tol * want_abs).all(), np.argwhere(gap > tol * want_abs)


class HostMesh:
    """A host mgb_geo handle of one of SHAPES (or of kind, L, k, K) with the native Python geometry of the same mesh, its
    operators and the yardstick's facets."""

    def __init__(self, name=None, kind=None, L=None, k=None, K=None):
        import mgb_amd as M
        from mgb_amd import _lib
        if name is not None:
            kind, L, k, K, _ = SHAPES[name]
        self.name, self.kind, self.L, self.k, self.K = name or "%s_L%d" % (kind, L), kind, L, k, K
        h = C.c_void_p()
        if kind == "fem1d":
            _lib.call("mgb_fem1d_native", L, C.byref(h))
            self.py = M.fem1d(L)
        elif kind == "fem2d":
            Kc = None if K is None else _lib.f64(K)
            _lib.call("mgb_fem2d_native", L, _lib.dptr(Kc), 0 if K is None else Kc.shape[0], C.byref(h))
            self.py = M.fem2d(L, K)
        else:
            _lib.call("mgb_fem3d_native", L, k, C.byref(h))
            self.py = M.fem3d(L, k)
        self.handle = h
        self.x, self.w = self.py.x.reshape(len(self.py.w), -1), self.py.w
        self.n, self.dim, self.block = self.x.shape[0], self.x.shape[1], self.py.discretization["block"]
        self.ops = ER.operators(self.py)
        self.F = facets(self.py)
        self.nf, self.q = self.F["nodes"].shape

    def close(self):
        from mgb_amd import _lib
        if self.handle is not None:
            _lib.call("mgb_geo_destroy", self.handle)
            self.handle = None


def host_boundary_flux(lib, g, fields, p, u=0, mask=None, rc_only=False, S=None, B=None):
    """mgb_geo_boundary_flux_host on a HostMesh: `fields` a list of (n, S) arrays, p a scalar or an (n,) array, mask None or
    (nf,) bool.  Returns (B, 5) and the per-facet values (B, nf); outputs prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    fields = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    pn = None if np.isscalar(p) else _lib.f64(p)
    p0 = float(p) if pn is None else float(pn[0])
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    out = np.full((max(B, 1), 5), 7.0)
    fac = np.full((max(B, 1), g.nf), 7.0)
    rc = lib.mgb_geo_boundary_flux_host(g.handle, B, table, S, u, p0, _lib.dptr(pn), _lib.u8ptr(m), _lib.dptr(fac), _lib.dptr(out))
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    return out, fac
