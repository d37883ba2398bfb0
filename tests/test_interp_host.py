"""CPU tests of the host restatement mgb_geo_interpolate_host (csrc/interp.hpp: the bins, the containment rule and the bases
the gfx950 kernel also runs) against the brute-force numpy helper tests/interp_reference.py.

Tolerances (values 1e-12 max|z|, gradients 1e-12 max|z| / h_min) are eps times a small constant for a 7- to 64-term sum with
O(1) basis values.  No test point lies within rounding of the containment tolerance, so element indices must match exactly."""
import ctypes as C

import numpy as np
import pytest

import interp_reference as IR
from interp_reference import check_against_helper, host_interpolate

M_POINTS = 501      # no multiple of anything


@pytest.fixture(scope="module", params=sorted(IR.CASES))
def geo(request, lib):
    g = IR.NativeGeo(request.param)
    yield g
    g.close()


@pytest.mark.parametrize("S", [1, 2, 5])
def test_interior_points(lib, geo, S):
    rng = np.random.default_rng(10 + S)
    pts, e = IR.points_interior(geo, M_POINTS, rng)
    z = rng.standard_normal((geo.n, S))                       # broken field: a wrong element or stride shows
    check_against_helper(geo, pts, z, host_interpolate(lib, geo, pts, z), exact_elem=e)


@pytest.mark.parametrize("S", [1, 2, 5])
def test_every_node_of_the_geometry(lib, geo, S):
    """Nodes lie on element faces: several elements contain them and the lowest index must win (continuous z)."""
    pts = IR.points_nodes(geo, max(geo.n, 8))
    z = IR.continuous_field(geo.x, S)
    re = check_against_helper(geo, pts, z, host_interpolate(lib, geo, pts, z))
    assert (re >= 0).all()
    vals = host_interpolate(lib, geo, geo.x, z, grad=False, want_elem=False)[0]
    assert np.abs(vals - z).max() <= IR.tolerances(geo.x, geo.block, z)[0]      # nodal basis: the field itself comes back


@pytest.mark.parametrize("S", [1, 5])
def test_outside_points(lib, geo, S):
    rng = np.random.default_rng(20 + S)
    pts = IR.points_outside(geo, 64, rng)
    z = rng.standard_normal((geo.n, S))
    vals, grads, elem = host_interpolate(lib, geo, pts, z)
    assert (elem == -1).all() and np.isnan(vals).all() and np.isnan(grads).all()
    assert (IR.interpolate(geo.x, geo.block, z, pts)[2] == -1).all()


def test_null_outputs_and_empty_query(lib, geo):
    rng = np.random.default_rng(30)
    pts, _ = IR.points_interior(geo, 17, rng)
    z = rng.standard_normal((geo.n, 2))
    full = host_interpolate(lib, geo, pts, z)
    bare = host_interpolate(lib, geo, pts, z, grad=False, want_elem=False)
    assert np.array_equal(full[0], bare[0]) and bare[1] is None and bare[2] is None
    assert lib.mgb_geo_interpolate_host(geo.handle, 0, None, 1, None, None, None, None) == 0      # m = 0 succeeds


def test_argument_errors(lib, geo):
    from mgb_amd import _lib
    z = np.zeros((geo.n, 1)); pts = np.zeros((1, geo.dim)); vals = np.zeros((1, 1))
    a = (_lib.dptr(pts), 1, _lib.dptr(z), _lib.dptr(vals), None, None)
    assert lib.mgb_geo_interpolate_host(None, 1, *a) == -1
    assert lib.mgb_geo_interpolate_host(geo.handle, -1, *a) == -1
    assert lib.mgb_geo_interpolate_host(geo.handle, 1, _lib.dptr(pts), 0, _lib.dptr(z), _lib.dptr(vals), None, None) == -1
    assert lib.mgb_geo_interpolate_host(geo.handle, 1, None, 1, _lib.dptr(z), _lib.dptr(vals), None, None) == -1
    assert lib.mgb_locator_create(None, geo.handle, C.byref(C.c_void_p())) == -1
    assert lib.mgb_locator_destroy(None) == 0
    assert lib.mgb_interpolate(None, 0, None, 1, None, None, None, None) == -1


def _custom_geo(lib, x, block):
    from mgb_amd import _lib
    x = _lib.f64(x)
    w = np.ones(x.shape[0])
    h = C.c_void_p()
    assert lib.mgb_geo_create(x.shape[0], x.shape[1], 1, block, _lib.dptr(x), _lib.dptr(w), C.byref(h)) == 0
    return h


@pytest.mark.parametrize("case,row", [("fem2d_L3", 7 * 5 + 4), ("fem2d_L3", 7 * 9 + 6), ("fem3d_L2_k2", 27 * 3 + 13)])
def test_elements_the_maps_do_not_assume_are_rejected(lib, case, row):
    """A perturbed midpoint / centroid / interior tensor node: MGB_E_ARG with a message; the unperturbed copy is accepted."""
    g = IR.NativeGeo(case)
    try:
        z = np.zeros((g.n, 1)); pts = g.x[:1].copy(); vals = np.zeros((1, 1))
        from mgb_amd import _lib
        for shift, want in ((0.0, 0), (1e-3, -1)):
            x = g.x.copy()
            x[row, 0] += shift
            h = _custom_geo(lib, x, g.block)
            rc = lib.mgb_geo_interpolate_host(h, 1, _lib.dptr(pts), 1, _lib.dptr(z), _lib.dptr(vals), None, None)
            assert rc == want and (want == 0 or b"locator" in lib.mgb_last_error())
            assert lib.mgb_geo_destroy(h) == 0
    finally:
        g.close()


def test_wrong_block_size_is_rejected(lib):
    from mgb_amd import _lib
    x = np.linspace(-1.0, 1.0, 6).reshape(-1, 1)
    h = _custom_geo(lib, x, 3)
    z = np.zeros((6, 1)); vals = np.zeros((1, 1))
    assert lib.mgb_geo_interpolate_host(h, 1, _lib.dptr(x[:1].copy()), 1, _lib.dptr(z), _lib.dptr(vals), None, None) == -1
    assert lib.mgb_geo_destroy(h) == 0


def test_python_surface_rejects_a_native_geometry():
    import mgb_amd as M
    g = M.fem2d(2)
    with pytest.raises(TypeError):
        M.interpolate(g, np.zeros((1, 2)), z=np.zeros(g.x.shape[0]))
    with pytest.raises(TypeError):
        M.sample_grid(g, (3, 3), z=np.zeros(g.x.shape[0]))
    with pytest.raises(TypeError):
        M.interpolate(np.zeros(3), np.zeros((1, 2)))
