"""Independent numpy restatement of the norms of a difference field, the yardstick of
test_norms_host.py and test_gpu_norms.py.  Built on tests/interp_reference.py: its Vandermonde bases, element maps and
brute-force point location.  d = a - r and grad d are evaluated per node exactly as the public contract says -- own element,
the nudged point x_i + 2^-20 (c_e - x_i) across meshes -- and summed with math.fsum.

Tolerances are derived, not tuned.  With dv, dg = IR.tolerances(x, block, z) (the per-value and per-gradient contract of the
bases: x the mesh whose polynomials are evaluated -- the other mesh across meshes, else the own one --, z the nodal fields
that go through the bases), W = sum w, D = max |d|, G = max |grad d| and eps = 2^-52:
  sum w |d|^q        q W (D + dv)^(q-1) dv + 8 n eps ref      (mean-value bound of a perturbed term; any summation order of
  sum w |grad d|^q   q W (G + dg)^(q-1) dg + 8 n eps ref       n non-negative terms)
  sum w d            W dv + 8 n eps sum w |d|
  max |d|, max |grad d|    dv, dg
  outside            exact"""
import ctypes as C
import math

import numpy as np

import interp_reference as IR

THETA = 2.0 ** -20
EPS = 2.0 ** -52

# the nested pairs of test_gpu_interpolate.py::test_device_agrees_with_refine: coarse case of IR.CASES -> (kind, fine L, extra)
NESTED = {"fem1d_L4": ("fem1d", 5, None), "fem2d_L3": ("fem2d", 4, None), "fem2d_L3_lshape": ("fem2d", 4, IR.LSHAPE),
          "fem3d_L2_k2": ("fem3d", 3, 2), "fem3d_L2_k3": ("fem3d", 3, 3)}


class Geo(IR.NativeGeo):
    """IR.NativeGeo with the quadrature weights; `spec` = (kind, L, extra) builds a geometry that is not one of IR.CASES."""

    def __init__(self, name, spec=None):
        from mgb_amd import _lib
        if spec is None:
            super().__init__(name)
        else:
            kind, L, extra = spec
            h = C.c_void_p()
            if kind == "fem1d":
                _lib.call("mgb_fem1d_native", L, C.byref(h))
            elif kind == "fem2d":
                K = None if extra is None else _lib.f64(extra)
                _lib.call("mgb_fem2d_native", L, _lib.dptr(K), 0 if K is None else K.shape[0], C.byref(h))
            else:
                _lib.call("mgb_fem3d_native", L, extra, C.byref(h))
            self.handle, self.name, self.lshape = h, name, extra is IR.LSHAPE
            n, dim, Lv, block = (C.c_int() for _ in range(4))
            _lib.call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(Lv), C.byref(block))
            self.n, self.dim, self.block = n.value, dim.value, block.value
            self.x = np.empty((self.n, self.dim))
            _lib.call("mgb_geo_get_xw", h, _lib.dptr(self.x), None)
        self.w = np.empty(self.n)
        _lib.call("mgb_geo_get_xw", self.handle, None, _lib.dptr(self.w))


def python_geometry(spec):
    """The native Python Geometry (operators, refine) of a (kind, L, extra) spec."""
    import mgb_amd as M
    kind, L, extra = spec
    return M.fem1d(L) if kind == "fem1d" else (M.fem2d(L, extra) if kind == "fem2d" else M.fem3d(L, extra))


def eval_in_elements(x, block, z, elem, pts):
    """Values (m, S) and physical gradients (m, S, dim) at pts (m, dim) of the polynomial of element elem[q] -- whether or not
    the point lies inside it."""
    x = x.reshape(x.shape[0], -1)
    dim = x.shape[1]
    z = z.reshape(x.shape[0], -1)
    m, S = pts.shape[0], z.shape[1]
    vals = np.full((m, S), np.nan)
    grads = np.full((m, S, dim), np.nan)
    for e in np.unique(elem[elem >= 0]):
        rows = np.nonzero(elem == e)[0]
        xe = x[e * block:(e + 1) * block]
        x0, J = IR._element_map(dim, block, xe)
        r = np.linalg.solve(J, (pts[rows] - x0).T).T
        N, dN = IR._bases(dim, block, r)
        ze = z[e * block:(e + 1) * block]
        vals[rows] = N @ ze
        grads[rows] = np.einsum("pbd,bs->psd", dN, ze) @ np.linalg.inv(J)
    return vals, grads


def own_gradient(x, block, z):
    """(n, S, dim): at node i the physical gradient of the nodal basis of i's own element i // block."""
    n = x.shape[0]
    return eval_in_elements(x, block, z, np.arange(n) // block, x.reshape(n, -1))[1]


def nudged(x, block):
    x = x.reshape(x.shape[0], -1)
    c = np.repeat(x.reshape(-1, block, x.shape[1]).mean(axis=1), block, axis=0)
    return x + THETA * (c - x)


def difference(x, block, z, ref_vals=None, ref_grads=None, other=None):
    """d (n, S), grad d (n, S, dim), the inside mask (n,), the element of the other mesh (n,) or None, and dv, dg of the
    module docstring.  other = (x_other, block_other, z_other)."""
    x = x.reshape(x.shape[0], -1)
    n = x.shape[0]
    z = z.reshape(n, -1)
    inside = np.ones(n, dtype=bool)
    elem = None
    if other is not None:
        xo, bo, zo = other
        xo = xo.reshape(xo.shape[0], -1)
        zo = zo.reshape(xo.shape[0], -1)
        elem = IR.interpolate(xo, bo, zo[:, :1], nudged(x, block))[2]
        inside = elem >= 0
        vb, gb = eval_in_elements(xo, bo, zo, elem, x)
        d, gd = z - vb, own_gradient(x, block, z) - gb
        d[~inside] = 0.0
        gd[~inside] = 0.0
        dv, dg = IR.tolerances(xo, bo, np.array([np.abs(z).max(), np.abs(zo).max()]))
    elif ref_vals is None:
        d, gd = z.copy(), own_gradient(x, block, z)
        dv, dg = IR.tolerances(x, block, z)
    elif ref_grads is None:
        d = z - ref_vals.reshape(n, -1)
        gd = own_gradient(x, block, d)
        dv, dg = IR.tolerances(x, block, d)
    else:
        d = z - ref_vals.reshape(n, -1)
        gd = own_gradient(x, block, z) - ref_grads.reshape(n, z.shape[1], -1)
        dv, dg = IR.tolerances(x, block, z)
    return d, gd, inside, elem, dv, dg


def _fsum(v):
    return math.fsum(v) if np.isfinite(v).all() else float(np.sum(v))


def sums(w, diff, q):
    """(S, 5) sums / maxima of the contract, sum w |d| (S,), the tolerances (S, 5) and the outside count."""
    d, gd, inside, _, dv, dg = diff
    n, S = d.shape
    W = math.fsum(w)
    ad, gn = np.abs(d), np.sqrt((gd * gd).sum(axis=2))
    out = np.zeros((S, 5))
    tol = np.zeros((S, 5))
    for s in range(S):
        wi, a, g = w[inside], ad[inside, s], gn[inside, s]
        absint = _fsum(wi * a)
        out[s] = [_fsum(wi * d[inside, s]), _fsum(wi * a ** q), _fsum(wi * g ** q), a.max(initial=0.0), g.max(initial=0.0)]
        D, G = out[s, 3], out[s, 4]
        tol[s] = [W * dv + 8 * n * EPS * absint,
                  q * W * (D + dv) ** (q - 1) * dv + 8 * n * EPS * out[s, 1],
                  q * W * (G + dg) ** (q - 1) * dg + 8 * n * EPS * out[s, 2], dv, dg]
    return out, tol, int((~inside).sum())


def check(name, got, got_outside, want, tol, want_outside):
    """Library sums (host or device) against the helper; prints every figure first."""
    gap = np.abs(got - want)
    for k, col in enumerate(("sum w d", "sum w|d|^q", "sum w|grad d|^q", "max|d|", "max|grad d|")):
        print("%s: %-16s off by %.3e (tolerance %.3e, value %.6e)" % (name, col, gap[:, k].max(), tol[gap[:, k].argmax(), k],
                                                                      np.abs(want[:, k]).max()))
    print("%s: outside %d (helper %d)" % (name, got_outside, want_outside))
    assert got_outside == want_outside
    assert np.isfinite(got).all()
    assert (gap <= tol).all(), np.argwhere(gap > tol)


def host_norms(lib, g, z, q, ref_vals=None, ref_grads=None, other=None, z_other=None, rc_only=False):
    """mgb_geo_field_norms_host on Geo handles; outputs prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    z = _lib.f64(z).reshape(g.n, -1)
    S = z.shape[1]
    rv = None if ref_vals is None else _lib.f64(ref_vals)
    rg = None if ref_grads is None else _lib.f64(ref_grads)
    zo = None if z_other is None else _lib.f64(z_other)
    out = np.full((S, 5), 7.0)
    outside = C.c_longlong(7)
    rc = lib.mgb_geo_field_norms_host(g.handle, S, _lib.dptr(z), q, _lib.dptr(rv), _lib.dptr(rg),
                                      None if other is None else other.handle, _lib.dptr(zo), _lib.dptr(out), C.byref(outside))
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    return out, int(outside.value)


def reference_fields(kind, g, S, rng, coarse=None):
    """(ref_vals, ref_grads, other, z_other) keyword values of one of the reference kinds on broken random fields."""
    if kind == "nothing":
        return dict()
    if kind == "vals":
        return dict(ref_vals=rng.standard_normal((g.n, S)))
    if kind == "vals+grads":
        return dict(ref_vals=rng.standard_normal((g.n, S)), ref_grads=rng.standard_normal((g.n, S, g.dim)))
    if kind == "self":
        return dict(other=g, z_other=rng.standard_normal((g.n, S)))
    return dict(other=coarse, z_other=rng.standard_normal((coarse.n, S)))


def helper_difference(g, z, ref_vals=None, ref_grads=None, other=None, z_other=None):
    return difference(g.x, g.block, z, ref_vals, ref_grads, None if other is None else (other.x, other.block, z_other))
