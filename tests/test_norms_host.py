"""CPU tests of the host restatement mgb_geo_field_norms_host (csrc/norms.hpp: the per-node routine the gfx950 kernel also
runs) against the numpy helper tests/norms_reference.py, on every geometry of interp_reference.CASES, S in {1, 2, 5},
q in {1, 2, 3.5} and the three kinds of reference (nothing; nodal values with and without gradients; a field on another
mesh: the geometry itself and the nested pairs of test_device_agrees_with_refine), plus known answers.

Tolerances: derived in tests/norms_reference.py from the per-value / per-gradient contract of the bases
(interp_reference.tolerances), the mean-value bound of a perturbed term and 8 n eps for any summation order."""
import numpy as np
import pytest

import interp_reference as IR
import norms_reference as NR

QS = (1.0, 2.0, 3.5)


@pytest.fixture(scope="module", params=sorted(IR.CASES))
def geo(request, lib):
    g = NR.Geo(request.param)
    yield g
    g.close()


@pytest.fixture(scope="module", params=sorted(NR.NESTED))
def pair(request, lib):
    """(coarse, fine, the fine Python geometry with its refine matrices and operators)"""
    spec = NR.NESTED[request.param]
    coarse, fine = NR.Geo(request.param), NR.Geo(request.param + "_fine", spec)
    yield coarse, fine, NR.python_geometry(spec)
    coarse.close()
    fine.close()


def _check_all_q(lib, g, z, ref):
    diff = NR.helper_difference(g, z, **ref)
    for q in QS:
        want, tol, outside = NR.sums(g.w, diff, q)
        got, got_outside = NR.host_norms(lib, g, z, q, **ref)
        NR.check("%s q=%g" % (g.name, q), got, got_outside, want, tol, outside)


@pytest.mark.parametrize("kind", ["nothing", "vals", "vals+grads", "self"])
@pytest.mark.parametrize("S", [1, 2, 5])
def test_host_against_helper(lib, geo, S, kind):
    rng = np.random.default_rng(100 + S)
    z = rng.standard_normal((geo.n, S))                       # broken fields: a wrong element, stride or column shows
    _check_all_q(lib, geo, z, NR.reference_fields(kind, geo, S, rng))


@pytest.mark.parametrize("S", [1, 2, 5])
def test_host_against_helper_across_nested_meshes(lib, pair, S):
    coarse, fine, _ = pair
    rng = np.random.default_rng(110 + S)
    z = rng.standard_normal((fine.n, S))
    ref = NR.reference_fields("cross", fine, S, rng, coarse)
    parent = {1: 2, 2: 4, 3: 8}[fine.dim]
    elem = NR.helper_difference(fine, z, **ref)[3]
    assert np.array_equal(elem, (np.arange(fine.n) // fine.block) // parent)      # every fine node lands in its parent
    _check_all_q(lib, fine, z, ref)


def test_constant_one_integrates_to_the_area(lib, geo):
    want = {1: 2.0, 2: 3.0 if geo.lshape else 4.0, 3: 8.0}[geo.dim]
    one = np.ones((geo.n, 2))
    dv, dg = IR.tolerances(geo.x, geo.block, one)
    for q in QS:
        out, outside = NR.host_norms(lib, geo, one, q)
        assert outside == 0
        assert np.abs(out[:, :2] - want).max() <= 1e-13 * want and np.array_equal(out[:, 3], [1.0, 1.0])
        assert np.abs(out[:, 2]).max() <= q * want * dg ** q and np.abs(out[:, 4]).max() <= dg      # the gradient of a constant


def test_fem2d_z_equals_x(lib):
    g = NR.Geo("fem2d_L3")
    try:
        out, _ = NR.host_norms(lib, g, g.x[:, :1].copy(), 2.0)
        print("z = x: sum w x^2 = %.17g, sum w |grad x|^2 = %.17g" % (out[0, 1], out[0, 2]))
        assert abs(out[0, 1] - 4.0 / 3.0) <= 1e-13 and abs(out[0, 2] - 4.0) <= 1e-13
        assert abs(out[0, 0]) <= 1e-13 and abs(out[0, 3] - 1.0) <= 1e-15 and abs(out[0, 4] - 1.0) <= 1e-13
    finally:
        g.close()


def test_gradient_agrees_with_the_operators_on_every_row(lib, pair):
    """max_i |grad a(x_i) - (dx a, dy a, dz a)_i| through column 4, and the helper's own gradient row by row."""
    _, fine, py = pair
    rng = np.random.default_rng(120)
    z = rng.standard_normal((fine.n, 3))
    ops = np.stack([py.operators[o] @ z for o in ("dx", "dy", "dz")[:fine.dim]], axis=2)
    dv, dg = IR.tolerances(fine.x, fine.block, z)
    gap = np.abs(NR.own_gradient(fine.x, fine.block, z) - ops).max()
    out, _ = NR.host_norms(lib, fine, z, 2.0, ref_vals=np.zeros_like(z), ref_grads=ops)
    print("%s: helper gradient off the operators by %.3e, library by %.3e (tolerance %.3e per component)"
          % (fine.name, gap, out[:, 4].max(), dg))
    assert gap <= dg
    assert out[:, 4].max() <= np.sqrt(fine.dim) * dg


@pytest.mark.parametrize("broken", [False, True])
def test_refined_coarse_field_against_itself_across_meshes(lib, pair, broken):
    """refine @ z on the fine mesh against z on the coarse one is zero in all five columns: for a continuous z, and -- only
    with the nudge, which takes the coarse gradient and value from the parent -- for a broken z."""
    coarse, fine, py = pair
    rng = np.random.default_rng(130)
    if broken:
        z = rng.standard_normal((coarse.n, 2))
    else:
        kind, L, extra = NR.NESTED[coarse.name]
        R = NR.python_geometry((kind, L - 1, extra)).subspaces["full"][-1]      # the continuous coarse space
        z = R @ rng.standard_normal((R.shape[1], 2))
    zf = py.refine[len(py.refine) - 2] @ z
    dv, dg = IR.tolerances(coarse.x, coarse.block, z)
    W = fine.w.sum()
    for q in QS:
        out, outside = NR.host_norms(lib, fine, zf, q, other=coarse, z_other=z)
        tol = np.array([W * dv, q * W * dv ** q, q * W * dg ** q, dv, dg])      # the tolerances around D = G = 0
        print("%s broken=%s q=%g: %s (tolerance %s)" % (fine.name, broken, q, np.abs(out).max(axis=0), tol))
        assert outside == 0
        assert (np.abs(out) <= tol).all()


def test_nan_poisons_only_its_column(lib, pair):
    coarse, fine, _ = pair
    rng = np.random.default_rng(140)
    z = rng.standard_normal((fine.n, 3))
    zo = rng.standard_normal((coarse.n, 3))
    clean, _ = NR.host_norms(lib, fine, z, 3.5, other=coarse, z_other=zo)
    bad = z.copy()
    bad[fine.n // 2, 1] = np.nan
    out, outside = NR.host_norms(lib, fine, bad, 3.5, other=coarse, z_other=zo)
    assert outside == 0 and np.isnan(out[1]).all()
    assert out[0].tobytes() == clean[0].tobytes() and out[2].tobytes() == clean[2].tobytes()
    bad = zo.copy()
    bad[coarse.n // 3, 2] = np.inf                                   # in the other mesh's field
    out, _ = NR.host_norms(lib, fine, z, 2.0, other=coarse, z_other=bad)
    clean, _ = NR.host_norms(lib, fine, z, 2.0, other=coarse, z_other=zo)
    assert not np.isfinite(out[2]).any() and out[:2].tobytes() == clean[:2].tobytes()
    ref = rng.standard_normal((fine.n, 3))
    clean, _ = NR.host_norms(lib, fine, z, 1.0, ref_vals=ref)
    ref[7, 0] = np.nan                                               # in the nodal reference values
    out, _ = NR.host_norms(lib, fine, z, 1.0, ref_vals=ref)
    assert np.isnan(out[0]).all() and out[1:].tobytes() == clean[1:].tobytes()


def test_unit_square_against_the_lshape(lib):
    sq, ls = NR.Geo("fem2d_L3"), NR.Geo("fem2d_L3_lshape")
    try:
        rng = np.random.default_rng(150)
        z, zo = rng.standard_normal((sq.n, 2)), rng.standard_normal((ls.n, 2))
        ref = dict(other=ls, z_other=zo)
        diff = NR.helper_difference(sq, z, **ref)
        want, tol, outside = NR.sums(sq.w, diff, 2.0)
        got, got_outside = NR.host_norms(lib, sq, z, 2.0, **ref)
        assert outside == 7 * (sq.n // 7) // 4                       # the elements of the notch (0, 1]^2: a quarter of the square
        NR.check("square against L-shape", got, got_outside, want, tol, outside)
    finally:
        sq.close()
        ls.close()


def test_argument_errors(lib, geo):
    from mgb_amd import _lib
    import ctypes as C
    z = np.zeros((geo.n, 1))
    rg = np.zeros((geo.n, 1, geo.dim))
    assert NR.host_norms(lib, geo, z, 2.0, rc_only=True) == 0
    for q in (0.5, np.nan, np.inf, -2.0):
        assert NR.host_norms(lib, geo, z, q, rc_only=True) == -1
    assert NR.host_norms(lib, geo, z, 2.0, ref_grads=rg, rc_only=True) == -1                        # ref_grads without ref_vals
    assert NR.host_norms(lib, geo, z, 2.0, ref_vals=z, other=geo, z_other=z, rc_only=True) == -1    # both references
    assert NR.host_norms(lib, geo, z, 2.0, other=geo, rc_only=True) == -1
    assert NR.host_norms(lib, geo, z, 2.0, z_other=z, rc_only=True) == -1
    out = np.zeros((1, 5))
    a = (_lib.dptr(z), 2.0, None, None, None, None)
    assert lib.mgb_geo_field_norms_host(None, 1, *a, _lib.dptr(out), None) == -1
    assert lib.mgb_geo_field_norms_host(geo.handle, 0, *a, _lib.dptr(out), None) == -1
    assert lib.mgb_geo_field_norms_host(geo.handle, 1, None, 2.0, None, None, None, None, _lib.dptr(out), None) == -1
    assert lib.mgb_geo_field_norms_host(geo.handle, 1, *a, None, None) == -1
    assert lib.mgb_geo_field_norms_host(geo.handle, 1, *a, _lib.dptr(out), None) == 0               # outside may be null
    assert lib.mgb_field_norms(None, 1, None, 2.0, None, None, None, None, _lib.dptr(out), None) == -1
    other = NR.Geo("fem1d_L1" if geo.dim != 1 else "fem2d_L1")
    try:
        assert NR.host_norms(lib, geo, z, 2.0, other=other, z_other=np.zeros((other.n, 1)), rc_only=True) == -1      # dimension
        assert b"dimension" in lib.mgb_last_error()
    finally:
        other.close()


def test_python_surface_rejects_what_it_cannot_take():
    import mgb_amd as M
    g = M.fem2d(2)
    with pytest.raises(TypeError):
        M.norms(g, z=np.zeros(g.x.shape[0]))                          # a native geometry has no device locator
    with pytest.raises(TypeError):
        M.norms(np.zeros(3))
    with pytest.raises(TypeError):
        M.error(np.zeros(3), lambda x: 0.0)
