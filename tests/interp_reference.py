"""Independent numpy restatement of point evaluation, the yardstick of test_interp_host.py and
test_gpu_interpolate.py: brute force over ALL elements (no bins), nodal bases from an inverted Vandermonde matrix (the oracle's
monomials, not the library's closed forms), inverse maps by np.linalg.solve.  Same containment rule as the public contract:
reference coordinates, tau = 1e-12, lowest element index wins, NaN / -1 outside.

Also the shared geometries and point sets of those two test files."""
import ctypes as C

import numpy as np

import mgb_oracle as O

TAU = 1e-12

# L-shaped domain [-1,1]^2 minus (0,1]^2 as 6 coarse triangles (3 squares, 2 triangles each)
LSHAPE = np.array([[-1, -1], [0, -1], [-1, 0], [0, -1], [0, 0], [-1, 0],
                   [0, -1], [1, -1], [0, 0], [1, -1], [1, 0], [0, 0],
                   [-1, 0], [0, 0], [-1, 1], [0, 0], [0, 1], [-1, 1]], dtype=np.float64)


def degree(dim, block):
    if dim == 1:
        assert block == 2
        return 1
    if dim == 2:
        assert block == 7
        return 0
    return {8: 1, 27: 2, 64: 3}[block]


_TRI_C = np.linalg.inv(O._tri_basis(O._TRI_NODES)[0])


def _bases(dim, block, r):
    """Nodal basis values (m, block) and reference gradients (m, block, dim) at reference points r (m, dim)."""
    if dim == 2:
        V, Vx, Vy = O._tri_basis(r)
        return V @ _TRI_C, np.stack([Vx @ _TRI_C, Vy @ _TRI_C], axis=2)
    k = degree(dim, block)
    _, basis, dbasis, _ = O._lagrange_1d(k)
    b = [basis(r[:, a]) for a in range(dim)]
    d = [dbasis(r[:, a]) for a in range(dim)]
    if dim == 1:
        return b[0], d[0][:, :, None]
    m = r.shape[0]
    t = lambda fx, fy, fz: np.einsum("pl,pj,pi->plji", fz, fy, fx).reshape(m, -1)      # x fastest
    return t(b[0], b[1], b[2]), np.stack([t(d[0], b[1], b[2]), t(b[0], d[1], b[2]), t(b[0], b[1], d[2])], axis=2)


def _element_map(dim, block, xe):
    """Origin and Jacobian (dim x dim, columns = images of the reference axes) of one element's affine map."""
    if dim == 2:
        return xe[0], np.stack([xe[1] - xe[0], xe[2] - xe[0]], axis=1)
    return xe[0], np.diag(xe[-1] - xe[0])


def interpolate(x, block, z, pts):
    """vals (m, S), grads (m, S, dim), elem (m,) int32 of the broken field z (n, S) on nodes x (n, dim) at pts (m, dim)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    n, dim = x.shape
    z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, dim)
    m, S = pts.shape[0], z.shape[1]
    vals = np.full((m, S), np.nan)
    grads = np.full((m, S, dim), np.nan)
    elem = np.full(m, -1, dtype=np.int32)
    finite = np.all(np.isfinite(pts), axis=1)
    for e in range(n // block):
        todo = np.nonzero((elem < 0) & finite)[0]
        if todo.size == 0:
            break
        xe = x[e * block:(e + 1) * block]
        x0, J = _element_map(dim, block, xe)
        r = np.linalg.solve(J, (pts[todo] - x0).T).T
        if dim == 2:
            inside = np.minimum(1.0 - r[:, 0] - r[:, 1], np.minimum(r[:, 0], r[:, 1])) >= -TAU
        else:
            inside = np.all((r >= -TAU) & (r <= 1.0 + TAU), axis=1)
        hit = todo[inside]
        if hit.size == 0:
            continue
        N, dN = _bases(dim, block, r[inside])
        ze = z[e * block:(e + 1) * block]
        vals[hit] = N @ ze
        gref = np.einsum("pbd,bs->psd", dN, ze)                    # reference gradient, (hits, S, dim)
        grads[hit] = gref @ np.linalg.inv(J)                       # physical = T^-T reference (row vectors: times T^-1)
        elem[hit] = e
    return vals, grads, elem


def h_min(x, block):
    """Smallest element edge."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    xe = x.reshape(-1, block, x.shape[1])
    if x.shape[1] == 2:
        v = xe[:, :3]
        return min(np.linalg.norm(v[:, i] - v[:, (i + 1) % 3], axis=1).min() for i in range(3))
    return np.abs(xe[:, -1] - xe[:, 0]).min()


# ------------------------------------------------------------------------------------------ shared cases of the C-ABI tests
CASES = {      # name -> (kind, L, k or K)
    "fem1d_L1": ("fem1d", 1, None), "fem1d_L4": ("fem1d", 4, None),
    "fem2d_L1": ("fem2d", 1, None),                  # two elements: the bin grid degenerates
    "fem2d_L3": ("fem2d", 3, None), "fem2d_L3_lshape": ("fem2d", 3, LSHAPE),      # 96 elements, non-convex
    "fem3d_L1_k3": ("fem3d", 1, 3),                  # one element
    "fem3d_L2_k1": ("fem3d", 2, 1), "fem3d_L2_k2": ("fem3d", 2, 2), "fem3d_L2_k3": ("fem3d", 2, 3),
}


class NativeGeo:
    """A host mgb_geo handle of one of CASES with its x, dim, block."""

    def __init__(self, name):
        from mgb_amd import _lib
        kind, L, extra = CASES[name]
        h = C.c_void_p()
        if kind == "fem1d":
            _lib.call("mgb_fem1d_native", L, C.byref(h))
        elif kind == "fem2d":
            K = None if extra is None else _lib.f64(extra)
            _lib.call("mgb_fem2d_native", L, _lib.dptr(K), 0 if K is None else K.shape[0], C.byref(h))
        else:
            _lib.call("mgb_fem3d_native", L, extra, C.byref(h))
        self.handle, self.name, self.lshape = h, name, extra is LSHAPE
        n, dim, Lv, block = (C.c_int() for _ in range(4))
        _lib.call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(Lv), C.byref(block))
        self.n, self.dim, self.block = n.value, dim.value, block.value
        self.x = np.empty((self.n, self.dim))
        _lib.call("mgb_geo_get_xw", h, _lib.dptr(self.x), None)

    def close(self):
        from mgb_amd import _lib
        if self.handle is not None:
            _lib.call("mgb_geo_destroy", self.handle)
            self.handle = None


def _ref_points(dim, m, rng, margin=1e-6):
    """Random reference coordinates at least `margin` from every face."""
    if dim == 2:
        lam = rng.dirichlet(np.ones(3), size=m) * (1.0 - 3.0 * margin) + margin
        return lam[:, 1:]
    return margin + (1.0 - 2.0 * margin) * rng.random((m, dim))


def points_interior(g, m, rng):
    """(a) a random element and random reference coordinates >= 1e-6 from every face -> pts (m, dim), the element of each."""
    nel = g.n // g.block
    e = rng.integers(0, nel, size=m)
    r = _ref_points(g.dim, m, rng)
    pts = np.empty((m, g.dim))
    for q in range(m):
        x0, J = _element_map(g.dim, g.block, g.x[e[q] * g.block:(e[q] + 1) * g.block])
        pts[q] = x0 + J @ r[q]
    return pts, e.astype(np.int32)


def points_nodes(g, m):
    """(b) every node of the geometry itself, repeated cyclically to m points."""
    return g.x[np.arange(m) % g.n].copy()


def points_outside(g, m, rng):
    """(c) points at least 1e-6 outside: beyond the bounding box, in the notch of the L-shape, and one NaN coordinate."""
    lo, hi = g.x.min(axis=0), g.x.max(axis=0)
    pts = lo + (hi - lo) * rng.random((m, g.dim))
    side = rng.integers(0, 2, size=m)
    axis = rng.integers(0, g.dim, size=m)
    off = 1e-6 + rng.random(m) * np.where(rng.random(m) < 0.5, 1e-3, 10.0)
    pts[np.arange(m), axis] = np.where(side == 0, lo[axis] - off, hi[axis] + off)
    if g.lshape:
        half = m // 2
        pts[:half] = 1e-6 + (1.0 - 1e-6) * rng.random((half, 2))      # the open notch (0, 1]^2, at least 1e-6 inside it
    pts[m - 1, (m - 1) % g.dim] = np.nan
    if m > 1:
        pts[m - 2, 0] = np.inf
    return pts


def continuous_field(x, S):
    """A smooth function of position, S columns: the same value at coincident nodes of neighbouring elements."""
    x = x.reshape(x.shape[0], -1)
    cols = []
    for s in range(S):
        v = np.cos(0.9 * (s + 1) + x @ (np.arange(1, x.shape[1] + 1) * (0.7 + 0.3 * s)))
        cols.append(v + 0.25 * (s + 1) * (x ** 2).sum(axis=1))
    return np.stack(cols, axis=1)


def tolerances(x, block, z):
    """Issue contract: values 1e-12 max|z|, gradients 1e-12 max|z| / h_min (eps times a small constant for a 7- to 64-term
    sum with O(1) basis values)."""
    zmax = np.abs(z).max()
    return 1e-12 * zmax, 1e-12 * zmax / h_min(x, block)


def host_interpolate(lib, g, pts, z, grad=True, want_elem=True):
    """mgb_geo_interpolate_host on a NativeGeo; outputs prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    pts = _lib.f64(pts).reshape(-1, g.dim)
    z = _lib.f64(z).reshape(g.n, -1)
    m, S = pts.shape[0], z.shape[1]
    vals = np.full((m, S), 7.0)
    grads = np.full((m, S, g.dim), 7.0) if grad else None
    elem = np.full(m, 7, dtype=np.int32) if want_elem else None
    rc = lib.mgb_geo_interpolate_host(g.handle, m, _lib.dptr(pts), S, _lib.dptr(z), _lib.dptr(vals), _lib.dptr(grads),
                                      _lib.iptr(elem))
    assert rc == 0, lib.mgb_last_error()
    return vals, grads, elem


def check_against_helper(g, pts, z, got, exact_elem=None):
    """(vals, grads, elem) of the library, host or device, against the helper to the tolerances above; prints each figure first."""
    vals, grads, elem = got
    rv, rg, re = interpolate(g.x, g.block, z, pts)
    vtol, gtol = tolerances(g.x, g.block, z)
    if exact_elem is not None:
        assert np.array_equal(re, exact_elem)
    if elem is not None:
        assert np.array_equal(elem, re), np.nonzero(elem != re)[0][:10]
    out = re < 0
    assert np.isnan(vals[out]).all() and np.isfinite(vals[~out]).all()
    if (~out).any():
        dv = np.abs(vals[~out] - rv[~out]).max()
        print("%s: values off by %.3e (tolerance %.3e)" % (g.name, dv, vtol))
        assert dv <= vtol
    if grads is not None:
        assert np.isnan(grads[out]).all()
        if (~out).any():
            dg = np.abs(grads[~out] - rg[~out]).max()
            print("%s: gradients off by %.3e (tolerance %.3e)" % (g.name, dg, gtol))
            assert dg <= gtol
    return re
