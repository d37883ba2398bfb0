"""Independent numpy restatement of the energy, flux and cone margin of a nodal field, the yardstick of
test_energy_host.py and test_gpu_energy.py.  Not a test.  Built from geometry.operators[...] (gradients are `op @ u`), the
quadrature weights w and plain `**`; the three sums are taken with math.fsum, so the yardstick itself has no summation error.

  gradient energy  sum w a^p / p        load  sum w f u        slack gap  sum w (s - a^p) / p   (term by term)
  flux_max  max a^(p-1) (1 at p = 1 where a > 0, 0 where a = 0)          violation  max (a^p - s)  (margin = -violation)
  flux  a^(p-2) g, exactly 0 where a = 0
A node with a non-finite u, s, f or gradient makes all five results NaN.

Bars: sums and extrema within KTOL = 1e-12 relative to the yardstick's value (the project's kernel-parity bar); a yardstick
value of exactly 0 (no forcing, a constant field) is met exactly.  Flux within KTOL relative to flux_max."""
import ctypes as C
import math

import numpy as np

KTOL = 1e-12
P_VALUES = (1.0, 1.5, 2.0, 3.0, "array")
GEOMETRIES = {"fem1d_L2": ("fem1d", 2, None), "fem2d_L2": ("fem2d", 2, None), "fem3d_L1": ("fem3d", 1, 3),
              "fem2d_L4": ("fem2d", 4, None)}
COLS = ("gradient energy", "load", "slack gap", "flux_max", "max (P - s)")


def exponent(p, x):
    """The scalar, or for "array" an (n,) exponent in [1, 2.5] that is exactly 1 and exactly 2 at a few nodes."""
    if not isinstance(p, str):
        return float(p)
    x = x.reshape(x.shape[0], -1)
    pn = 1.75 + 0.75 * np.sin(3.0 * x[:, 0] + 0.5)
    pn[::5] = 1.0
    pn[1::7] = 2.0
    return pn


def operators(geometry):
    """The host dx [, dy [, dz]] matrices of a native or a device Geometry."""
    ops = [geometry.operators[o] for o in ("dx", "dy", "dz")[:geometry.discretization["dim"]]]
    return [getattr(op, "host", op) for op in ops]


def gradient(ops, u):
    return np.stack([op @ u for op in ops], axis=1)


def flux(ops, u, p):
    g = gradient(ops, u)
    a = np.sqrt((g * g).sum(axis=1))
    p = np.broadcast_to(np.asarray(p, dtype=float), a.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(a == 0.0, 0.0, a ** (p - 2.0))
        return np.where(a[:, None] == 0.0, 0.0, m[:, None] * g)


def energy(ops, w, z, p, f=None, u=0, s=-1):
    """(5,) results of one field z (n, S): gradient energy, load, slack gap, flux_max, max (P - s)."""
    uv, sv = z[:, u], z[:, s]
    fv = np.zeros_like(uv) if f is None else np.asarray(f, dtype=float)
    g = gradient(ops, uv)
    gs = (g * g).sum(axis=1)
    if not all(np.isfinite(v).all() for v in (uv, sv, fv, gs)):
        return np.full(5, np.nan)
    a = np.sqrt(gs)
    p = np.broadcast_to(np.asarray(p, dtype=float), a.shape)
    P = a ** p
    fm = np.where(a > 0.0, a ** (p - 1.0), 0.0)
    return np.array([math.fsum(w * P / p), math.fsum(w * fv * uv), math.fsum(w * (sv - P) / p), fm.max(), (P - sv).max()])


def check(name, got, want, tol=KTOL):
    """Library results (host or device, (5,) or (B, 5)) against the yardstick; prints every figure first."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    gap = np.abs(got - want)
    bar = tol * np.abs(want)
    for k, col in enumerate(COLS):
        j = (gap[:, k] - bar[:, k]).argmax()
        print("%s: %-16s off by %.3e (bar %.3e, value %.17g)" % (name, col, gap[j, k], bar[j, k], want[j, k]))
    assert got.shape == want.shape
    assert np.isfinite(got).all()
    assert (gap <= bar).all(), np.argwhere(gap > bar)


def check_flux(name, got, want, flux_max, tol=KTOL):
    gap = np.abs(got - want).max()
    print("%s: flux off by %.3e (bar %.3e, flux_max %.6e)" % (name, gap, tol * flux_max, flux_max))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert gap <= tol * flux_max


class HostGeo:
    """A host mgb_geo handle of one of GEOMETRIES with n, dim, x, w and the operators of the native Python geometry."""

    def __init__(self, name):
        import mgb_amd as M
        from mgb_amd import _lib
        kind, L, k = GEOMETRIES[name]
        h = C.c_void_p()
        if kind == "fem1d":
            _lib.call("mgb_fem1d_native", L, C.byref(h))
        elif kind == "fem2d":
            _lib.call("mgb_fem2d_native", L, None, 0, C.byref(h))
        else:
            _lib.call("mgb_fem3d_native", L, k, C.byref(h))
        self.handle, self.name = h, name
        n, dim, Lv, block = (C.c_int() for _ in range(4))
        _lib.call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(Lv), C.byref(block))
        self.n, self.dim, self.block = n.value, dim.value, block.value
        self.x, self.w = np.empty((self.n, self.dim)), np.empty(self.n)
        _lib.call("mgb_geo_get_xw", h, _lib.dptr(self.x), _lib.dptr(self.w))
        py = M.fem1d(L) if kind == "fem1d" else (M.fem2d(L) if kind == "fem2d" else M.fem3d(L, k))
        self.ops = operators(py)

    def close(self):
        from mgb_amd import _lib
        if self.handle is not None:
            _lib.call("mgb_geo_destroy", self.handle)
            self.handle = None


def host_energy(lib, g, fields, p, f=None, u=0, s=-1, want_flux=True, rc_only=False, S=None, B=None, f_rows=None):
    """mgb_geo_field_energy_host on a HostGeo: `fields` a list of (n, S) arrays, p a scalar or an (n,) array, f None, (n,) or
    (B, n).  Returns (B, 5) and the flux (B, n, dim); outputs prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    fields = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    s = s + fields[0].shape[1] if s < 0 else s
    pn = None if np.isscalar(p) else _lib.f64(p)
    p0 = float(p) if pn is None else float(pn[0])
    fa = None if f is None else _lib.f64(f).reshape(-1, g.n)
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    out = np.full((max(B, 1), 5), 7.0)
    fl = np.full((max(B, 1), g.n, g.dim), 7.0) if want_flux else None
    rc = lib.mgb_geo_field_energy_host(g.handle, B, table, S, u, s, p0, _lib.dptr(pn), _lib.dptr(fa),
                                       (1 if fa is None else fa.shape[0]) if f_rows is None else f_rows, _lib.dptr(out), _lib.dptr(fl))
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    return out, fl
