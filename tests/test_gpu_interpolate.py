"""GPU tests of mgb_interpolate (csrc/interp.hip) and of the Python surface interpolate / sample_grid.

The device kernel is compared with the brute-force numpy helper tests/interp_reference.py on the geometries, S values, point
sets and tolerances of tests/test_interp_host.py (values 1e-12 max|z|, gradients 1e-12 max|z| / h_min: eps times a small
constant for a 7- to 64-term sum with O(1) basis values), with m = 4099 points (no multiple of 64: the last wave is partial),
and with the host restatement mgb_geo_interpolate_host: element indices bitwise, values to the same tolerances."""
import ctypes as C

import numpy as np
import pytest

import interp_reference as IR
from interp_reference import check_against_helper, host_interpolate

pytestmark = pytest.mark.gpu

M_POINTS = 4099


class DeviceLocator:
    """mgb_locator of one of IR.CASES on the default backend, with a direct call of mgb_interpolate."""

    def __init__(self, name):
        import mgb_amd as M
        from mgb_amd import _lib
        self.M, self._lib = M, _lib
        self.g = IR.NativeGeo(name)
        self.backend = M.backend_hip()
        self.handle = C.c_void_p()
        _lib.call("mgb_locator_create", self.backend.handle, self.g.handle, C.byref(self.handle))

    def __call__(self, pts, z, grad=True, want_elem=True):
        M, _lib, g = self.M, self._lib, self.g
        pts = _lib.f64(pts).reshape(-1, g.dim)
        z = _lib.f64(z).reshape(g.n, -1)
        m, S = pts.shape[0], z.shape[1]
        pv, zv = M.HPCVector(pts, self.backend), M.HPCVector(z, self.backend)
        vals = M.HPCVector(np.full(m * S, 7.0), self.backend)
        grads = M.HPCVector(np.full(m * S * g.dim, 7.0), self.backend) if grad else None
        elem = np.full(m, 7, dtype=np.int32) if want_elem else None
        _lib.call("mgb_interpolate", self.handle, m, pv.handle, S, zv.handle, vals.handle, grads.handle if grad else None,
                  _lib.iptr(elem))
        return (vals.to_numpy().reshape(m, S), grads.to_numpy().reshape(m, S, g.dim) if grad else None, elem)

    def close(self):
        if self.handle is not None:
            self._lib.call("mgb_locator_destroy", self.handle)
            self.handle = None
        self.g.close()


@pytest.fixture(scope="module", params=sorted(IR.CASES))
def dev(request, gpu_required):
    d = DeviceLocator(request.param)
    yield d
    d.close()


def _check_device(lib, dev, pts, z, exact_elem=None):
    got = dev(pts, z)
    ref_elem = check_against_helper(dev.g, pts, z, got, exact_elem=exact_elem)
    hv, hg, he = host_interpolate(lib, dev.g, pts, z)
    vtol, gtol = IR.tolerances(dev.g.x, dev.g.block, z)
    assert np.array_equal(got[2], he)                                     # bitwise in elem
    inside = he >= 0
    assert np.isnan(got[0][~inside]).all() and np.isnan(got[1][~inside]).all()
    if inside.any():
        assert np.abs(got[0][inside] - hv[inside]).max() <= vtol
        assert np.abs(got[1][inside] - hg[inside]).max() <= gtol
    return ref_elem


@pytest.mark.parametrize("S", [1, 2, 5])
def test_device_against_helper_and_host(lib, dev, S):
    rng = np.random.default_rng(40 + S)
    g = dev.g
    pts, e = IR.points_interior(g, M_POINTS, rng)                         # (a) broken field, exact elements
    _check_device(lib, dev, pts, rng.standard_normal((g.n, S)), exact_elem=e)
    zc = IR.continuous_field(g.x, S)                                      # (b) every node: lowest containing element wins
    re = _check_device(lib, dev, IR.points_nodes(g, M_POINTS), zc)
    assert (re >= 0).all()
    pts = IR.points_outside(g, M_POINTS, rng)                             # (c) NaN rows, element -1
    vals, grads, elem = dev(pts, zc)
    assert (elem == -1).all() and np.isnan(vals).all() and np.isnan(grads).all()
    assert (IR.interpolate(g.x, g.block, zc, pts)[2] == -1).all()


def test_single_point_empty_query_null_outputs_and_reproducibility(lib, dev):
    rng = np.random.default_rng(50)
    g = dev.g
    z = rng.standard_normal((g.n, 2))
    pts, e = IR.points_interior(g, M_POINTS, rng)
    first, second = dev(pts, z), dev(pts, z)
    for a, b in zip(first, second):                                       # two launches, bitwise equal
        assert a.tobytes() == b.tobytes()
    bare = dev(pts, z, grad=False, want_elem=False)                       # grads null and elem null
    assert bare[0].tobytes() == first[0].tobytes() and bare[1] is None and bare[2] is None
    only_elem = dev(pts, z, grad=False)
    assert np.array_equal(only_elem[2], e) and only_elem[0].tobytes() == first[0].tobytes()
    _check_device(lib, dev, pts[:1], z, exact_elem=e[:1])                 # m = 1
    vals, grads, elem = dev(np.zeros((0, g.dim)), z)                      # m = 0: no launch, success
    assert vals.shape == (0, 2) and grads.shape == (0, 2, g.dim) and elem.shape == (0,)


def test_wrong_sizes_are_argument_errors(lib, dev):
    M, _lib, g = dev.M, dev._lib, dev.g
    v = lambda k: M.HPCVector(np.zeros(k), dev.backend)
    m, S = 3, 2
    good = dict(pts=v(m * g.dim), z=v(g.n * S), vals=v(m * S), grads=v(m * S * g.dim))
    call = lambda mm, SS, a: lib.mgb_interpolate(dev.handle, mm, a["pts"].handle, SS, a["z"].handle, a["vals"].handle,
                                                 a["grads"].handle if a["grads"] is not None else None, None)
    assert call(m, S, good) == 0
    for key in good:
        bad = dict(good)
        bad[key] = v(len(good[key]) + 1)
        assert call(m, S, bad) == -1, key
    assert call(m, 0, good) == -1 and call(-1, S, good) == -1
    assert lib.mgb_interpolate(None, m, good["pts"].handle, S, good["z"].handle, good["vals"].handle, None, None) == -1
    assert lib.mgb_interpolate(dev.handle, m, None, S, good["z"].handle, good["vals"].handle, None, None) == -1
    assert lib.mgb_locator_create(dev.backend.handle, None, C.byref(C.c_void_p())) == -1


def test_gradient_agrees_with_the_operators_at_centroids(gpu_required):
    """fem2d L=3: at the centroid nodes (strictly interior, no ties) the interpolated gradient is (dx z, dy z) there."""
    import mgb_amd as M
    dev = DeviceLocator("fem2d_L3")
    try:
        g = dev.g
        native = M.fem2d(3)
        rng = np.random.default_rng(60)
        z = rng.standard_normal((g.n, 2))
        rows = np.arange(6, g.n, 7)
        vals, grads, elem = dev(g.x[rows], z)
        want = np.stack([native.operators["dx"] @ z, native.operators["dy"] @ z], axis=2)[rows]
        vtol, gtol = IR.tolerances(g.x, g.block, z)
        assert np.array_equal(elem, rows // 7)
        assert np.abs(vals - z[rows]).max() <= vtol
        assert np.abs(grads - want).max() <= gtol
    finally:
        dev.close()


@pytest.mark.parametrize("coarse,kind,L,extra", [("fem1d_L4", "fem1d", 5, None), ("fem2d_L3", "fem2d", 4, None),
                                                 ("fem2d_L3_lshape", "fem2d", 4, IR.LSHAPE), ("fem3d_L2_k2", "fem3d", 3, 2),
                                                 ("fem3d_L2_k3", "fem3d", 3, 3)])
def test_device_agrees_with_refine(gpu_required, coarse, kind, L, extra):
    """interpolate(g_{L-1}, z, g_L.x) == g_L.refine[L-2] @ z for z in the continuous coarse space, on every fine row; for a
    broken z at the strictly interior fine centroids of the triangles, with element == parent exactly."""
    import mgb_amd as M
    fine = M.fem1d(L) if kind == "fem1d" else (M.fem2d(L, extra) if kind == "fem2d" else M.fem3d(L, extra))
    crs = M.fem1d(L - 1) if kind == "fem1d" else (M.fem2d(L - 1, extra) if kind == "fem2d" else M.fem3d(L - 1, extra))
    dev = DeviceLocator(coarse)
    try:
        g = dev.g
        assert np.array_equal(crs.x.reshape(g.n, -1), g.x)
        rng = np.random.default_rng(70)
        R = crs.subspaces["full"][-1]
        z = R @ rng.standard_normal((R.shape[1], 2))
        vals, _, elem = dev(fine.x, z)
        assert (elem >= 0).all()
        assert np.abs(vals - fine.refine[L - 2] @ z).max() <= IR.tolerances(g.x, g.block, z)[0]
        if kind == "fem2d":
            zb = rng.standard_normal((g.n, 3))
            rows = np.arange(6, fine.x.shape[0], 7)
            vals, _, elem = dev(fine.x[rows], zb)
            assert np.array_equal(elem, (rows // 7) // 4)
            assert np.abs(vals - (fine.refine[L - 2] @ zb)[rows]).max() <= IR.tolerances(g.x, g.block, zb)[0]
    finally:
        dev.close()


def test_python_surface_on_a_solution(gpu_required):
    import mgb_amd as M
    sol = M.fem2d_mpi_solve(L=3, p=1.5)
    x, z = sol.geometry.x.to_numpy(), sol.z.to_numpy()
    vtol, gtol = IR.tolerances(x, 7, z)
    back = M.interpolate(sol, sol.geometry.x)                             # the nodes themselves: the solution comes back
    assert back.shape == z.shape and np.abs(back - z).max() <= vtol
    assert sol.geometry._locator is not None                              # made once, cached on the geometry
    cached = sol.geometry._locator
    rng = np.random.default_rng(80)
    pts = -1.0 + 2.0 * rng.random((M_POINTS, 2))
    vals, grads, elem = M.interpolate(sol, pts, grad=True, return_element=True)
    assert sol.geometry._locator is cached
    rv, rg, re = IR.interpolate(x, 7, z, pts)
    assert np.array_equal(elem, re) and (elem >= 0).all()
    assert np.abs(vals - rv).max() <= vtol and np.abs(grads - rg).max() <= gtol
    X, img = M.sample_grid(sol, (33, 35))
    assert X.shape == (33, 35, 2) and img.shape == (33, 35, 2)
    assert np.array_equal(X[:, 0, 1], np.linspace(-1.0, 1.0, 33)) and np.array_equal(X[0, :, 0], np.linspace(-1.0, 1.0, 35))
    X, img = M.sample_grid(sol, (33, 33))
    assert not np.isnan(img).any()                                        # the default square: no point is outside
    assert np.abs(img.reshape(-1, 2) - IR.interpolate(x, 7, z, X.reshape(-1, 2))[0]).max() <= vtol
    one = M.interpolate(sol.geometry, pts[:5], z=z[:, 0])                 # (n,) array on a device geometry
    assert one.shape == (5, 1) and np.array_equal(one[:, 0], vals[:5, 0])
    with pytest.raises(ValueError):
        M.interpolate(sol.geometry, pts, z=z[:-1])
    with pytest.raises(ValueError):
        M.interpolate(sol, pts[:, :1])


def test_sample_grid_on_the_lshape_marks_the_notch(gpu_required):
    import mgb_amd as M
    geo = M.fem2d_mpi(3, IR.LSHAPE)
    x = geo.x.to_numpy()
    z = IR.continuous_field(x, 2)
    X, img = M.sample_grid(geo, (33, 33), z=M.HPCMatrix(z, geo.x.backend))
    notch = (X[..., 0] > 0) & (X[..., 1] > 0)                              # the open notch (0, 1]^2
    assert notch.sum() == 16 * 16
    assert np.array_equal(np.isnan(img[..., 0]), notch) and np.array_equal(np.isnan(img[..., 1]), notch)
    rv = IR.interpolate(x, 7, z, X.reshape(-1, 2))[0].reshape(33, 33, 2)
    assert np.abs(img[~notch] - rv[~notch]).max() <= IR.tolerances(x, 7, z)[0]
    vals, elem = M.interpolate(geo, [[0.5, 0.5], [-0.5, -0.5]], z=z, return_element=True)
    assert elem[0] == -1 and elem[1] >= 0 and np.isnan(vals[0]).all()


def test_parabolic_snapshots_in_one_launch(gpu_required):
    import mgb_amd as M
    sol = M.parabolic_solve(M.fem2d_mpi(2), h=0.5, t1=1.0, p=2.0)
    rng = np.random.default_rng(90)
    pts = -1.0 + 2.0 * rng.random((257, 2))
    snaps, grads = M.interpolate(sol, pts, grad=True)
    assert snaps.shape == (3, 257, 3) and grads.shape == (3, 257, 3, 2)
    for t, u in enumerate(sol.u):
        v, gr = M.interpolate(sol.geometry, pts, z=u, grad=True)
        assert np.array_equal(snaps[t], v) and np.array_equal(grads[t], gr)
    X, img = M.sample_grid(sol, (9, 9))
    assert img.shape == (3, 9, 9, 3) and not np.isnan(img).any()
