"""CPU tests of the host restatement mgb_geo_field_energy_host (csrc/energy.hpp: the per-node routine the gfx950 kernels also
run) against the numpy yardstick tests/energy_reference.py on the oracle geometries fem1d L=2, fem2d L=2 and fem3d L=1, for
p in {1, 1.5, 2, 3} and an array p(x), plus closed forms on affine fields and the argument errors.

Bars (tests/energy_reference.py): sums and extrema within KTOL = 1e-12 relative, flux within KTOL relative to flux_max."""
import numpy as np
import pytest

import energy_reference as ER

MGB_E_ARG = -1
HOST_GEOMETRIES = ("fem1d_L2", "fem2d_L2", "fem3d_L1")


@pytest.fixture(scope="module", params=HOST_GEOMETRIES)
def geo(request, lib):
    g = ER.HostGeo(request.param)
    yield g
    g.close()


def _fields(g, B, seed):
    """B distinct random (n, 3) fields -- broken across elements, so a wrong element, stride or column shows -- and (B, n) forcing."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((g.n, 3)) for _ in range(B)], rng.standard_normal((B, g.n))


@pytest.mark.parametrize("p", ER.P_VALUES)
def test_host_against_numpy(lib, geo, p):
    pv = ER.exponent(p, geo.x)
    zs, f = _fields(geo, 3, 200)
    for u, s in ((0, -1), (2, 0)):
        out, fl = ER.host_energy(lib, geo, zs, pv, f=f, u=u, s=s)
        want = np.array([ER.energy(geo.ops, geo.w, zs[b], pv, f[b], u, s) for b in range(3)])
        ER.check("%s p=%s u=%d s=%d" % (geo.name, p, u, s), out, want)
        for b in range(3):
            ER.check_flux("%s p=%s field %d" % (geo.name, p, b), fl[b], ER.flux(geo.ops, zs[b][:, u], pv), want[b, 3])
    one, fl1 = ER.host_energy(lib, geo, zs[1:2], pv, f=f[0])            # one field, (n,) forcing: the bits of the batch
    shared, _ = ER.host_energy(lib, geo, zs, pv, f=f[0])                # three fields sharing one forcing row
    assert shared[1].tobytes() == one[0].tobytes()
    none, _ = ER.host_energy(lib, geo, zs, pv)                           # no forcing: the load is exactly 0
    assert np.array_equal(none[:, 1], np.zeros(3)) and np.array_equal(none[:, [0, 2, 3, 4]], shared[:, [0, 2, 3, 4]])


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0, 3.0])
def test_affine_field_closed_form(lib, p):
    """u = a . x + b: gradient energy |a|^p area / p, flux |a|^(p-2) a at every node, flux_max |a|^(p-1)."""
    for name, a, area in (("fem1d_L2", np.array([-1.75]), 2.0), ("fem2d_L2", np.array([0.75, -1.25]), 4.0)):
        g = ER.HostGeo(name)
        try:
            z = np.stack([g.x @ a + 0.3, np.full(g.n, 5.0)], axis=1)
            out, fl = ER.host_energy(lib, g, [z], p)
            na = np.linalg.norm(a)
            want_flux = na ** (p - 2.0) * a
            print("%s p=%g: gradient energy %.17g (closed form %.17g), flux_max %.17g (%.17g), flux off by %.3e"
                  % (name, p, out[0, 0], na ** p * area / p, out[0, 3], na ** (p - 1.0), np.abs(fl[0] - want_flux).max()))
            assert abs(out[0, 0] - na ** p * area / p) <= ER.KTOL * na ** p * area / p
            assert abs(out[0, 3] - na ** (p - 1.0)) <= ER.KTOL * na ** (p - 1.0)
            assert np.abs(fl[0] - want_flux).max() <= ER.KTOL * na ** (p - 1.0)
            assert abs(out[0, 2] - (5.0 - na ** p) * area / p) <= ER.KTOL * abs(5.0 - na ** p) * area / p
            assert abs(out[0, 4] - (na ** p - 5.0)) <= ER.KTOL * abs(na ** p - 5.0) and out[0, 1] == 0.0
        finally:
            g.close()


@pytest.mark.parametrize("p", [1.0, 1.5, 3.0])
def test_zero_gradient_gives_zero_flux(lib, geo, p):
    """u constant on element 0.  The gradient is ElemBasis's sum over the nodal values, so it is exactly 0 where every product
    is: for the constant 0 on every element kind, and in 1-D (derivative weights -1, 1) for any constant.  (A non-zero constant
    on a triangle leaves a rounding-level gradient, about 1e-17, at the centroid node; that is a > 0, not this case.)"""
    for const in (0.0, 0.625) if geo.dim == 1 else (0.0,):
        zs, _ = _fields(geo, 1, 210)
        z = zs[0]
        z[:geo.block, 0] = const
        out, fl = ER.host_energy(lib, geo, [z], p)
        assert np.array_equal(fl[0, :geo.block], np.zeros((geo.block, geo.dim)))
        assert np.isfinite(out).all() and np.isfinite(fl).all()
        w0 = geo.w.copy()
        w0[:geo.block] = 0.0                                             # the yardstick without element 0: it contributes 0
        assert abs(out[0, 0] - ER.energy(geo.ops, w0, z, p)[0]) <= ER.KTOL * out[0, 0]


def test_non_zero_constant_at_p_1_is_zero_or_a_unit_vector(lib):
    """Known limitation, pinned: on a triangle the derivative weights of the basis sum to zero only up to rounding, so a non-zero
    constant leaves a gradient of about 1e-17 at some nodes.  That is a > 0: at p = 1 the flux there is g / a, a unit vector made
    of rounding noise.  Every row is exactly 0 or of length 1, never NaN or Inf, and the energy of the element is below 1e-15."""
    g = ER.HostGeo("fem2d_L2")
    try:
        z = np.zeros((g.n, 2))
        z[:, 0] = 0.625
        out, fl = ER.host_energy(lib, g, [z], 1.0)
        length = np.sqrt((fl[0] ** 2).sum(axis=1))
        print("constant 0.625, p = 1: %d of %d flux rows are unit vectors, gradient energy %.3e" % ((length > 0).sum(), g.n, out[0, 0]))
        assert np.isfinite(fl).all() and np.isfinite(out).all()
        assert ((length == 0.0) | (np.abs(length - 1.0) <= ER.KTOL)).all()
        assert 0.0 <= out[0, 0] <= 1e-15 and out[0, 3] in (0.0, 1.0)
    finally:
        g.close()


def test_large_finite_values_are_finite(lib, geo):
    """Only a non-finite u, s, f or gradient poisons a node: finite values whose sum would overflow do not."""
    zs, f = _fields(geo, 1, 230)
    zs[0][3, 2] = 1.7e308
    f[0, 3] = 1.7e308
    out, _ = ER.host_energy(lib, geo, zs, 1.5, f=f)
    assert np.isfinite(out).all()
    ER.check(geo.name + " large finite s and f", out, ER.energy(geo.ops, geo.w, zs[0], 1.5, f[0]))


def test_non_finite_input_is_never_dropped(lib, geo):
    zs, f = _fields(geo, 3, 220)
    clean, _ = ER.host_energy(lib, geo, zs, 1.5, f=f)
    for col, bad in ((0, np.nan), (0, np.inf), (2, -np.inf), (2, np.nan)):
        broken = [z.copy() for z in zs]
        broken[1][geo.n - 1, col] = bad
        out, _ = ER.host_energy(lib, geo, broken, 1.5, f=f)
        assert np.isnan(out[1]).all()
        assert out[0].tobytes() == clean[0].tobytes() and out[2].tobytes() == clean[2].tobytes()
    fb = f.copy()
    fb[2, 0] = np.nan
    out, _ = ER.host_energy(lib, geo, zs, 1.5, f=fb)
    assert np.isnan(out[2]).all() and out[:2].tobytes() == clean[:2].tobytes()


def test_argument_errors(lib, geo):
    z = np.zeros((geo.n, 2))
    H = lambda **kw: ER.host_energy(lib, geo, [z], kw.pop("p", 2.0), rc_only=True, **kw)
    assert H() == 0
    for p in (0.5, np.nan, np.inf, -2.0):
        assert H(p=p) == MGB_E_ARG
    assert H(p=np.full(geo.n, 0.5)) == MGB_E_ARG and H(p=np.r_[np.full(geo.n - 1, 2.0), np.nan]) == MGB_E_ARG
    assert H(u=2) == MGB_E_ARG and H(u=-1) == MGB_E_ARG and H(s=2) == MGB_E_ARG
    assert H(u=1, s=1) == MGB_E_ARG and b"same column" in lib.mgb_last_error()
    assert H(B=0) == MGB_E_ARG and H(B=-3) == MGB_E_ARG
    assert H(S=0) == MGB_E_ARG
    assert H(f=np.zeros(geo.n), f_rows=2) == MGB_E_ARG                    # one field takes one row of forcing
    assert ER.host_energy(lib, geo, [z, z, z], 2.0, f=np.zeros((2, geo.n)), rc_only=True) == MGB_E_ARG
    from mgb_amd import _lib
    out = np.zeros((1, 5))
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z))
    assert lib.mgb_geo_field_energy_host(None, 1, table, 2, 0, 1, 2.0, None, None, 1, _lib.dptr(out), None) == MGB_E_ARG
    assert lib.mgb_geo_field_energy_host(geo.handle, 1, None, 2, 0, 1, 2.0, None, None, 1, _lib.dptr(out), None) == MGB_E_ARG
    assert lib.mgb_geo_field_energy_host(geo.handle, 1, table, 2, 0, 1, 2.0, None, None, 1, None, None) == MGB_E_ARG
    null = (_lib.c_dbl_p * 1)(None)
    assert lib.mgb_geo_field_energy_host(geo.handle, 1, null, 2, 0, 1, 2.0, None, None, 1, _lib.dptr(out), None) == MGB_E_ARG
    assert lib.mgb_geo_field_energy_host(geo.handle, 1, table, 2, 0, 1, 2.0, None, None, 1, _lib.dptr(out), None) == 0      # flux may be null
    assert lib.mgb_geo_field_energy(None, 1, None, 2, 0, 1, 2.0, None, None, 1, _lib.dptr(out)) == MGB_E_ARG
    assert lib.mgb_geo_field_flux(None, None, 2, 0, 2.0, None, None) == MGB_E_ARG


def test_python_surface_rejects_what_it_cannot_take():
    import mgb_amd as M
    g = M.fem2d(2)
    z = np.zeros((g.x.shape[0], 2))
    with pytest.raises(TypeError, match="geometry"):
        M.energy(g, 2.0, z=z)                                             # a native geometry has no device locator
    with pytest.raises(TypeError, match="geometry"):
        M.flux(g, 2.0, z=z)
    with pytest.raises(TypeError):
        M.energy(np.zeros(3), 2.0)
    with pytest.raises(TypeError):
        M.flux(np.zeros(3), 2.0)
    x = np.linspace(-1.0, 1.0, 4).reshape(4, 1)                           # f(x) or f(t, x): parameters without a default count
    assert np.array_equal(M._energy_forcing(lambda xi, scale=2.0: scale * xi[0], x, None, 1, "energy"), 2.0 * x.T)
    assert M._energy_forcing(lambda t, xi, scale=2.0: scale * t, x, np.arange(3.0), 3, "energy").shape == (3, 4)
    with pytest.raises(TypeError, match="f"):
        M._energy_forcing(lambda a, b, c: 0.0, x, np.arange(3.0), 3, "energy")
    e = M.Energy(1.0, 2.0, 3.0, 0.5, 0.25, 1.5)
    assert M.mpi_to_native(e) is e and e.ts is None                       # host data already: passed through
    assert {"energy", "flux", "Energy"} <= set(M.__all__)
