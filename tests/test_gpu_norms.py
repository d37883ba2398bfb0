"""GPU tests of mgb_field_norms (csrc/norms.hip) and of the Python surface norms / error / convergence.

The device result is compared with the numpy helper tests/norms_reference.py and with the host restatement
mgb_geo_field_norms_host on the matrix of tests/test_norms_host.py -- every geometry of interp_reference.CASES (less than a
wave: fem1d_L1, fem2d_L1; three workgroups with a partial last one, so that the finish launch sees more than one partial:
fem2d_L3_lshape, 672 nodes; an exact multiple of 256: fem3d_L2_k3; one element: fem3d_L1_k3; up to 16 workgroups: the fine
meshes of the nested pairs), S in {1, 2, 5}, q in {1, 2, 3.5}, the three kinds of reference -- to the tolerances derived in
tests/norms_reference.py; `outside` is exact and two calls are bitwise equal."""
import ctypes as C
import math

import numpy as np
import pytest

import interp_reference as IR
import norms_reference as NR

pytestmark = pytest.mark.gpu

QS = (1.0, 2.0, 3.5)


class DeviceGeo:
    """mgb_locator of a NR.Geo on the default backend, with a direct call of mgb_field_norms."""

    def __init__(self, name, spec=None):
        import mgb_amd as M
        from mgb_amd import _lib
        self.M, self._lib = M, _lib
        self.g = NR.Geo(name, spec)
        self.backend = M.backend_hip()
        self.handle = C.c_void_p()
        _lib.call("mgb_locator_create", self.backend.handle, self.g.handle, C.byref(self.handle))

    def vec(self, a):
        return None if a is None else self.M.HPCVector(self._lib.f64(a).reshape(-1), self.backend)

    def rc(self, S, q, z, ref_vals=None, ref_grads=None, other=None, z_other=None, out=None, outside=None):
        """status of mgb_field_norms on device vectors (or None)"""
        h = lambda v: None if v is None else v.handle
        return self._lib.load().mgb_field_norms(self.handle, S, h(z), q, h(ref_vals), h(ref_grads),
                                                None if other is None else other.handle, h(z_other), self._lib.dptr(out),
                                                None if outside is None else C.byref(outside))

    def __call__(self, z, q, ref_vals=None, ref_grads=None, other=None, z_other=None):
        S = np.asarray(z).reshape(self.g.n, -1).shape[1]
        out = np.full((S, 5), 7.0)
        outside = C.c_longlong(7)
        rc = self.rc(S, q, self.vec(z), self.vec(ref_vals), self.vec(ref_grads), other, self.vec(z_other), out, outside)
        assert rc == 0, self._lib.load().mgb_last_error()
        return out, int(outside.value)

    def close(self):
        if self.handle is not None:
            self._lib.call("mgb_locator_destroy", self.handle)
            self.handle = None
        self.g.close()


@pytest.fixture(scope="module", params=sorted(IR.CASES))
def dev(request, gpu_required):
    d = DeviceGeo(request.param)
    yield d
    d.close()


@pytest.fixture(scope="module", params=sorted(NR.NESTED))
def pair(request, gpu_required):
    coarse, fine = DeviceGeo(request.param), DeviceGeo(request.param + "_fine", NR.NESTED[request.param])
    yield coarse, fine
    coarse.close()
    fine.close()


def _check_all_q(lib, dev, z, ref, other=None):
    """device against the helper and the host restatement for every q; two device calls bitwise equal"""
    g = dev.g
    host_ref = dict(ref)
    dev_ref = dict(ref)
    if other is not None:
        host_ref["other"], dev_ref["other"] = other.g, other
    diff = NR.helper_difference(g, z, **host_ref)
    for q in QS:
        want, tol, outside = NR.sums(g.w, diff, q)
        got, got_outside = dev(z, q, **dev_ref)
        NR.check("%s device q=%g" % (g.name, q), got, got_outside, want, tol, outside)
        host, host_outside = NR.host_norms(lib, g, z, q, **host_ref)
        assert got_outside == host_outside and (np.abs(got - host) <= tol).all()
        again, again_outside = dev(z, q, **dev_ref)
        assert again.tobytes() == got.tobytes() and again_outside == got_outside


@pytest.mark.parametrize("kind", ["nothing", "vals", "vals+grads", "self"])
@pytest.mark.parametrize("S", [1, 2, 5])
def test_device_against_helper_and_host(lib, dev, S, kind):
    rng = np.random.default_rng(200 + S)
    z = rng.standard_normal((dev.g.n, S))
    ref = NR.reference_fields(kind, dev.g, S, rng)
    other = dev if ref.pop("other", None) is not None else None
    _check_all_q(lib, dev, z, ref, other)


@pytest.mark.parametrize("S", [1, 2, 5])
def test_device_against_helper_and_host_across_nested_meshes(lib, pair, S):
    coarse, fine = pair
    rng = np.random.default_rng(210 + S)
    z = rng.standard_normal((fine.g.n, S))
    _check_all_q(lib, fine, z, dict(z_other=rng.standard_normal((coarse.g.n, S))), coarse)


def test_unit_square_against_the_lshape(lib, gpu_required):
    sq, ls = DeviceGeo("fem2d_L3"), DeviceGeo("fem2d_L3_lshape")
    try:
        rng = np.random.default_rng(220)
        z, zo = rng.standard_normal((sq.g.n, 2)), rng.standard_normal((ls.g.n, 2))
        got, outside = sq(z, 2.0, other=ls, z_other=zo)
        assert outside == 7 * (sq.g.n // 7) // 4
        _check_all_q(lib, sq, z, dict(z_other=zo), ls)
    finally:
        sq.close()
        ls.close()


def test_nan_poisons_only_its_column(pair):
    coarse, fine = pair
    rng = np.random.default_rng(230)
    z, zo = rng.standard_normal((fine.g.n, 3)), rng.standard_normal((coarse.g.n, 3))
    clean, _ = fine(z, 3.5, other=coarse, z_other=zo)
    bad = z.copy()
    bad[fine.g.n // 2, 1] = np.nan
    out, outside = fine(bad, 3.5, other=coarse, z_other=zo)
    assert outside == 0 and np.isnan(out[1]).all()
    assert out[0].tobytes() == clean[0].tobytes() and out[2].tobytes() == clean[2].tobytes()
    bad = zo.copy()
    bad[coarse.g.n // 3, 2] = np.inf
    out, _ = fine(z, 3.5, other=coarse, z_other=bad)
    assert not np.isfinite(out[2]).any() and out[:2].tobytes() == clean[:2].tobytes()


def test_argument_errors(dev):
    g = dev.g
    S = 2
    out = np.zeros((S, 5))
    v = lambda k: dev.vec(np.zeros(k))
    z, rv, rg = v(g.n * S), v(g.n * S), v(g.n * S * g.dim)
    assert dev.rc(S, 2.0, z, out=out) == 0
    assert dev.rc(S, 2.0, z, rv, rg, out=out) == 0
    assert dev.rc(S, 2.0, z, other=dev, z_other=rv, out=out) == 0
    assert dev.rc(S, 2.0, None, out=out) == -1 and dev.rc(S, 2.0, z, out=None) == -1 and dev.rc(0, 2.0, z, out=out) == -1
    for q in (0.999, math.nan, math.inf, -1.0):
        assert dev.rc(S, q, z, out=out) == -1
    assert dev.rc(S, 2.0, v(g.n * S + 1), out=out) == -1
    assert dev.rc(S, 2.0, z, v(g.n * S - 1), out=out) == -1
    assert dev.rc(S, 2.0, z, rv, v(g.n * S * g.dim + 1), out=out) == -1
    assert dev.rc(S, 2.0, z, None, rg, out=out) == -1                                 # ref_grads without ref_vals
    assert dev.rc(S, 2.0, z, rv, None, dev, rv, out=out) == -1                        # both kinds of reference
    assert dev.rc(S, 2.0, z, other=dev, out=out) == -1 and dev.rc(S, 2.0, z, z_other=rv, out=out) == -1
    assert dev.rc(S, 2.0, z, other=dev, z_other=v(g.n * S + 1), out=out) == -1
    other = DeviceGeo("fem1d_L1" if g.dim != 1 else "fem2d_L1")
    try:
        assert dev.rc(S, 2.0, z, other=other, z_other=v(other.g.n * S), out=out) == -1      # another dimension
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------ the Python surface
def _exact(x):
    return np.array([math.exp(x[0]) * math.sin(x[1]), 0.0])


def _exact_grad(x):
    return np.array([[math.exp(x[0]) * math.sin(x[1]), math.exp(x[0]) * math.cos(x[1])], [0.0, 0.0]])


_F = lambda x: np.array([0.0, 0.0, 0.0, 1.0])
_G = lambda x: np.array([math.exp(x[0]) * math.sin(x[1]), 100.0])


@pytest.fixture(scope="module")
def sols(gpu_required):
    """the harmonic manufactured problem u* = exp(x) sin(y), p = 2, at L = 2, 3, 4"""
    import mgb_amd as M
    return {L: M.fem2d_mpi_solve(L=L, p=2.0, f=_F, g=_G) for L in (2, 3, 4)}


def _helper_error(x, w, z, q=2.0):
    """the helper applied to nodal values z against the exact solution and its exact gradient"""
    ref = np.array([_exact(xi) for xi in x])
    rg = np.array([_exact_grad(xi) for xi in x])
    return NR.sums(w, NR.difference(x, 7, z, ref, rg), q)


def test_python_norms_and_error_against_the_exact_solution(sols):
    import mgb_amd as M
    import mgb_oracle as O
    sol = sols[3]
    x, w, z = sol.geometry.x.to_numpy(), sol.geometry.w.to_numpy(), sol.z.to_numpy()
    err = M.error(sol, _exact, grad=_exact_grad)
    want, tol, _ = _helper_error(x, w, z)
    NR.check("error(sol, exact)", err.sums, err.outside, want, tol, 0)
    assert err.q == 2.0 and np.array_equal(err.lq, np.sqrt(err.sums[:, 1])) and np.array_equal(err.w1q, np.sqrt(err.sums[:, 2]))
    assert np.array_equal(err.integral, err.sums[:, 0]) and np.array_equal(err.max, err.sums[:, 3])
    nrm = M.norms(sol, q=3.5)
    want, tol, _ = NR.sums(w, NR.difference(x, 7, z), 3.5)
    NR.check("norms(sol)", nrm.sums, nrm.outside, want, tol, 0)
    assert np.array_equal(nrm.lq, nrm.sums[:, 1] ** (1.0 / 3.5)) and np.array_equal(nrm.gradmax, nrm.sums[:, 4])
    same = M.norms(sol.geometry, z=z[:, 0])                                       # (n,) array on a device geometry
    assert same.sums.shape == (1, 5) and same.sums[0].tobytes() == M.norms(sol, q=2.0).sums[0].tobytes()
    arr = M.error((sol.geometry, sol.z), np.array([_exact(xi) for xi in x]), grad=np.array([_exact_grad(xi) for xi in x]))
    assert arr.sums.tobytes() == err.sums.tobytes()                               # arrays instead of callables
    # the looser cross-check: the same numpy formula on the oracle's own solve of the problem.  Margin: the project's stated
    # 1e-10 solve parity, amplified by |u| / |e| ~ 1e2, with 100x headroom.
    so = O.fem2d_solve(L=3, p=2.0, f=_F, g=_G)
    ow, _, _ = _helper_error(np.asarray(so.geometry.x), np.asarray(so.geometry.w), np.asarray(so.z))
    l2, h1 = math.sqrt(ow[0, 1]), math.sqrt(ow[0, 2])
    gap = max(abs(err.lq[0] - l2) / l2, abs(err.w1q[0] - h1) / h1)
    print("L=3: L2 error %.6e (oracle %.6e), H1 error %.6e (oracle %.6e), relative gap %.3e (margin 1e-6)"
          % (err.lq[0], l2, err.w1q[0], h1, gap))
    assert gap <= 1e-6


def test_python_error_across_meshes(sols):
    import mgb_amd as M
    a, b = sols[3], sols[4]
    xa, za = a.geometry.x.to_numpy(), a.z.to_numpy()
    xb, wb, zb = b.geometry.x.to_numpy(), b.geometry.w.to_numpy(), b.z.to_numpy()
    err = M.error(a, b)                                                           # runs on the finer mesh: b
    want, tol, outside = NR.sums(wb, NR.difference(xb, 7, zb, other=(xa, 7, za)), 2.0)
    want[:, 0] = -want[:, 0]                                                      # the signed integral is that of a - b
    NR.check("error(L3, L4)", err.sums, err.outside, want, tol, outside)
    assert err.outside == 0
    assert M.error(b, a).sums[:, 1:].tobytes() == err.sums[:, 1:].tobytes()
    assert np.array_equal(M.error(b, a).integral, -err.integral)
    on_a = M.error(a, b, on="a")                                                  # the quadrature of the coarse mesh
    wa = a.geometry.w.to_numpy()
    want, tol, outside = NR.sums(wa, NR.difference(xa, 7, za, other=(xb, 7, zb)), 2.0)
    NR.check("error(L3, L4, on=a)", on_a.sums, on_a.outside, want, tol, outside)


def test_python_convergence(sols):
    import mgb_amd as M
    order = [sols[2], sols[3], sols[4]]
    conv = M.convergence(order, exact=_exact, grad=_exact_grad)
    errs = [M.error(s, _exact, grad=_exact_grad) for s in order]
    lq = np.array([e.lq for e in errs])
    w1q = np.array([e.w1q for e in errs])
    print("L2 errors %s orders %s; H1 errors %s orders %s" % (lq[:, 0], conv.order_lq[:, 0], w1q[:, 0], conv.order_w1q[:, 0]))
    assert np.array_equal(conv.lq, lq) and np.array_equal(conv.w1q, w1q)
    assert np.array_equal(conv.order_lq[:, 0], np.log2(lq[:-1, 0] / lq[1:, 0]))
    assert np.array_equal(conv.order_w1q[:, 0], np.log2(w1q[:-1, 0] / w1q[1:, 0]))
    rel = M.convergence(order)                                                    # against the finest solution
    assert rel.lq.shape == (2, 2) and rel.order_lq.shape == (1, 2)
    assert rel.lq[1].tobytes() == M.error(sols[3], sols[4]).lq.tobytes()


def test_python_value_errors(sols):
    import mgb_amd as M
    sol = sols[3]
    n = sol.z.shape[0]
    with pytest.raises(ValueError):
        M.error(sol, np.zeros((n, 3)))                                            # mismatched S
    with pytest.raises(ValueError):
        M.error(sol, lambda x: np.zeros(3))
    with pytest.raises(ValueError):
        M.error(sol, (sols[4].geometry, sols[4].z.to_numpy()[:, :1]))
    with pytest.raises(ValueError):
        M.norms(sol, q=0.5)
    ls = M.fem2d_mpi(3, IR.LSHAPE)
    zl = np.zeros((len(ls.w), 2))
    assert M.error(sol, (ls, zl)).outside == 0                                    # runs on the L-shape (more nodes): all inside
    with pytest.raises(ValueError):
        M.error(sol, (ls, zl), on="a")                                            # the square sticks out of the L-shape
    skipped = M.error(sol, (ls, zl), on="a", allow_outside=True)
    assert skipped.outside == 7 * (n // 7) // 4
    line = M.fem1d_mpi(3)
    with pytest.raises(ValueError):
        M.error(sol, (line, np.zeros((len(line.w), 2))))                          # another dimension
