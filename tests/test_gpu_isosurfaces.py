"""isosurfaces() on the device (csrc/isosurface.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-item routine and against the numpy yardstick tests/isosurface_reference.py.

Shapes, chosen for what can break: fem3d L=1 k=1 r=0 (6 items: one workgroup, 250 idle lanes), L=2 k=3 r=0 (1296 items, 6
workgroups: offsets across workgroups), L=4 k=3 r=0 (82 944 items, 324 workgroups: the finish and the scan fold chunks of 2),
L=2 k=3 r=2 (82 944 items: the tensor Lagrange path), a batch of 3 fields x 4 levels with a level out of range and a NaN node,
and the degenerate r = 0 cases of test_isosurface_host.py.

Bars: against the host restatement counts, offsets and items equal, vertices and maxima BIT FOR BIT (both sides run the same
IEEE + - * / with contraction off), the three sums within 1e-12 of the sum of their absolute terms; against numpy the bars of
tests/isosurface_util.py.  Measured on an MI355X: 0 vertex coordinates differ in every case; largest ratios to the yardstick's
bars vertices 0.050, sums 3.0e-4, maxima 0.044; sums against the host restatement 2.1e-4 of the bar."""
import ctypes as C

import numpy as np
import pytest

import isosurface_util as IU

pytestmark = pytest.mark.gpu
LEVELS = [0.37, 0.91, 1.37]


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_GEO = {}


def mesh(M, L, k):
    """(device geometry, host mesh) of the same nodes."""
    if (L, k) not in _GEO:
        geo, host = M.fem3d_mpi(L, k), IU.host_mesh(L, k)
        assert np.array_equal(geo.x.to_numpy().reshape(host.n, 3), host.x)
        _GEO[(L, k)] = (geo, host)
    return _GEO[(L, k)]


def batch(M, geo, fields, levels, **kw):
    """isosurfaces() of several fields in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(geo, np.arange(float(len(fields))), [M.HPCMatrix(np.asarray(z).reshape(len(z), -1)) for z in fields])
    iso = M.isosurfaces(sol, levels, **kw)
    assert np.array_equal(iso.ts, sol.ts)
    return iso


def tilted(x):
    return x[:, 0] + 0.5 * x[:, 1] + 0.25 * x[:, 2] + 0.05


def smooth(x):
    return np.sin(3.0 * x[:, 0] + 0.5) * np.cos(2.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 2] + 0.2 * x[:, 2]


@pytest.mark.parametrize("L,k,refine", [(1, 1, 0), (2, 3, 0), (4, 3, 0), (2, 3, 2)])
def test_device_against_host_and_numpy(M, lib, L, k, refine):
    geo, h = mesh(M, L, k)
    assert h.items(refine) == {(1, 1, 0): 6, (2, 3, 0): 1296, (4, 3, 0): 82944, (2, 3, 2): 82944}[(L, k, refine)]
    z = np.stack([np.zeros(h.n), IU.paraboloid(h.x) if k > 1 else tilted(h.x)], axis=1)
    levels = LEVELS if k > 1 else [-0.31, 0.23, 0.97]
    name = "fem3d L=%d k=%d r=%d" % (L, k, refine)
    iso = M.isosurfaces(geo, levels, u=1, z=z, refine=refine)
    assert iso.rows.shape == (1, 3, 5) and iso.above.shape == iso.area.shape == iso.excess.shape == (3,) and iso.ts is None
    dev = IU.device_result(iso)
    host = IU.host_isosurfaces(lib, h, [z], levels, refine, u=1)
    keys = ["gpu %s" % name]
    IU.same_as_host(name, dev, host, h, [z], levels, refine, u=1, keys=keys)
    IU.against_reference(name + " device", dev, h, [z], levels, refine, u=1, keys=keys)
    assert (iso.count > 0).all() and iso.reached.all()
    tri = iso.triangles(1)
    assert tri.shape == (iso.count[1], 3, 3) and np.array_equal(tri.reshape(-1, 9), dev.row(0, 1)[0])
    assert np.array_equal(iso.items(1), dev.row(0, 1)[1]) and iso.items(1).dtype == np.int32
    assert np.array_equal(iso.elements(1), dev.row(0, 1)[1] // (6 * (k * 2 ** refine) ** 3)) and iso.elements(1).max() < h.nel
    if refine == 0 and k > 1:      # the closed sphere: every edge twice, in opposite directions
        fwd, rev = IU.edge_pairs(tri)
        assert set(fwd.values()) == {1} and all(rev.get(e, 0) == 1 for e in fwd)


def test_batch_with_a_level_out_of_range_and_a_nan_node(M, lib):
    """3 fields x 4 levels in one call: against the host, and bit for bit the single-field, single-level calls; a repeated call
    and triangles=False return the same bits.  The smooth field has rows with more triangles than emitting items."""
    geo, h = mesh(M, 2, 3)
    rng = np.random.default_rng(7)
    base = IU.paraboloid(h.x)
    fields = [base, smooth(h.x) + 0.8, base + 0.1 * rng.standard_normal(h.n)]
    fields[0][64 * 3 + 21] = np.nan
    levels = [0.37, 0.91, 5.0, 1.37]
    iso = batch(M, geo, fields, levels)
    assert iso.above.shape == iso.area.shape == iso.excess.shape == iso.count.shape == iso.reached.shape == (3, 4)
    dev = IU.device_result(iso)
    host = IU.host_isosurfaces(lib, h, fields, levels)
    IU.same_as_host("batch 3 x 4", dev, host, h, fields, levels, 0)
    IU.against_reference("batch 3 x 4 device", dev, h, fields, levels, 0)
    assert np.isnan(iso.rows[0]).all() and np.isfinite(iso.rows[[1, 2]]).all() and (iso.count[0] > 0).any()
    assert not iso.reached[:, 2].any() and (iso.count[:, 2] == 0).all() and (iso.rows[[1, 2], 2, 3] < 0).all()
    items = iso.items(0, 1)
    assert len(items) > len(np.unique(items)) > 0 and (items[1:] == items[:-1]).any() and (np.diff(items) >= 0).all()
    again = batch(M, geo, fields, levels)
    assert again.rows.tobytes() == iso.rows.tobytes() and again._tri.tobytes() == iso._tri.tobytes()
    assert np.array_equal(again._item, iso._item) and np.array_equal(again._offsets, iso._offsets)
    cheap = batch(M, geo, fields, levels, triangles=False)
    assert cheap.rows.tobytes() == iso.rows.tobytes() and np.array_equal(cheap.count, iso.count)
    with pytest.raises(ValueError, match="triangles=False"):
        cheap.triangles(0, 0)
    for b in range(3):
        for l in range(4):
            one = M.isosurfaces(geo, levels[l], z=fields[b])
            assert isinstance(one.above, float) and isinstance(one.count, int) and isinstance(one.reached, bool)
            assert one.rows[0, 0].tobytes() == iso.rows[b, l].tobytes() and one.count == iso.count[b, l]
            assert one.triangles().tobytes() == iso.triangles(l, b).tobytes()
            assert np.array_equal(one.items(), iso.items(l, b)) and np.array_equal(one.elements(), iso.elements(l, b))


@pytest.mark.parametrize("case", ["u = x", "u = c", "outside", "inf node", "corner on the level", "six items"])
def test_degenerate_cases_at_refine_0(M, lib, case):
    geo, h = mesh(M, 1, 1) if case in ("corner on the level", "six items") else mesh(M, 2, 2)
    if case == "u = x":
        fields, levels = [h.x[:, 0].copy()], [0.0]
    elif case == "u = c":
        fields, levels = [np.full(h.n, 0.3)], [0.3]
    elif case == "outside":
        fields, levels = [IU.paraboloid(h.x)], [3.5, -0.5]
    elif case == "inf node":
        z = IU.paraboloid(h.x)
        zb = z.copy()
        zb[27 * 5 + 13] = np.inf
        fields, levels = [zb, z], [0.37]
    elif case == "corner on the level":
        z = np.ones(8)
        z[0] = 0.25
        fields, levels = [z], [0.25, 0.5]
    else:
        fields, levels = [tilted(h.x)], [0.0]
    iso = batch(M, geo, fields, levels)
    dev = IU.device_result(iso)
    host = IU.host_isosurfaces(lib, h, fields, levels)
    IU.same_as_host(case, dev, host, h, fields, levels, 0)
    IU.against_reference(case + " device", dev, h, fields, levels, 0)
    if case == "u = x":
        assert iso.area[0, 0] == 4.0 and abs(iso.above[0, 0] - 4.0) <= 1e-12 and abs(iso.excess[0, 0] - 2.0) <= 1e-12
    elif case == "u = c":
        assert np.array_equal(iso.rows[0, 0], np.zeros(5)) and iso.count[0, 0] == 0 and not iso.reached[0, 0]
    elif case == "outside":
        assert not iso.reached.any() and iso.above[0, 0] == 0.0 and abs(iso.above[0, 1] - 8.0) <= 1e-12
    elif case == "inf node":
        assert np.isnan(iso.rows[0]).all() and np.isfinite(iso.rows[1]).all()
    elif case == "corner on the level":
        assert iso.count[0, 0] == 0 and iso.area[0, 0] == 0.0 and not iso.reached[0, 0] and iso.count[0, 1] == 6
    else:
        assert iso.count[0, 0] > 6 and set(iso.items(0, 0).tolist()) == set(range(6))


def test_argument_errors(M):
    geo, h = mesh(M, 2, 2)
    z = IU.paraboloid(h.x)
    for kw, err in ((dict(levels=np.nan), ValueError), (dict(levels=[0.1, np.inf]), ValueError), (dict(levels=[]), ValueError),
                    (dict(levels=[[0.1]]), ValueError), (dict(refine=3), ValueError), (dict(refine=-1), ValueError),
                    (dict(refine=1.0), ValueError), (dict(u=1), ValueError), (dict(z=z[:-1]), ValueError)):
        with pytest.raises(err):
            M.isosurfaces(geo, **{**dict(levels=0.37, z=z), **kw})
    g2, g1 = M.fem2d_mpi(2), M.fem1d_mpi(3)
    for flat in (g2, g1):
        with pytest.raises(ValueError, match="level_sets"):
            M.isosurfaces(flat, 0.1, z=np.zeros(len(flat.w)))
    with pytest.raises(TypeError):
        M.isosurfaces(z, 0.1)
    # the C entry point: MGB_E_ARG before anything is launched
    from mgb_amd import _lib
    loc, backend = M._locator_of(geo)
    zv = M.HPCVector(z, backend)
    other = M.HPCVector(z[:-1], backend)
    rows, counts, lv = np.empty(5), np.empty(1, dtype=np.int64), np.array([0.37])
    lib = _lib.load()
    null_field = object()

    def rc(loc=loc, B=1, vec=zv, S=1, u=0, nl=1, lvp=_lib.dptr(lv), refine=0, out=_lib.dptr(rows),
           cnt=counts.ctypes.data_as(_lib.c_ll_p)):
        table = None if vec is None else (C.c_void_p * 1)(None if vec is null_field else vec.handle.value)
        return lib.mgb_geo_isosurfaces(loc, B, table, S, u, nl, lvp, refine, out, cnt, None)

    assert rc() == 0
    foreign = M.HPCVector(z, M.HPCBackend(0))      # the right length, on a second context of the same device
    for kw in (dict(loc=None), dict(vec=None), dict(vec=null_field), dict(lvp=None), dict(out=None), dict(cnt=None), dict(B=0), dict(nl=0),
               dict(B=65536), dict(nl=65536), dict(S=0), dict(u=1), dict(u=-1), dict(refine=3), dict(refine=-1), dict(vec=other),
               dict(vec=foreign), dict(lvp=_lib.dptr(np.array([np.inf])))):
        assert rc(**kw) == IU.MGB_E_ARG, kw
    assert rc(vec=foreign) == IU.MGB_E_ARG and b"another context" in lib.mgb_last_error()
    loc2, backend2 = M._locator_of(g2)
    z2 = M.HPCVector(np.zeros(len(g2.w)), backend2)
    assert rc(loc=loc2, vec=z2) == IU.MGB_E_ARG and b"level_sets" in lib.mgb_last_error()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem3d_mpi(1, 1, backend=be)
    z = M.HPCMatrix(np.ones((8, 2)), be)
    assert M.isosurfaces(g, 0.5, z=z).above == 8.0                        # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.isosurfaces(g, 0.5, z=z)
        rows, counts, lv = np.zeros(5), np.zeros(1, dtype=np.int64), np.array([0.5])
        assert lib.mgb_geo_isosurfaces(loc, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows),
                                       counts.ctypes.data_as(_lib.c_ll_p), None) == IU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)


def test_solutions(M):
    """A fem3d solve and a short 3-D parabolic run: shapes of every field, ts, above decreasing in c, the rows of the C entry
    point, and the snapshots of the run against their single calls."""
    from mgb_amd import _lib
    sol = M.fem3d_mpi_solve(L=2)
    u = sol.z.to_numpy()[:, 0]
    levels = u.min() + (u.max() - u.min()) * np.array([0.2, 0.4, 0.6, 0.8])
    iso = M.isosurfaces(sol, levels, refine=1)
    for v in (iso.above, iso.area, iso.excess, iso.count, iso.reached):
        assert v.shape == (4,)
    print("fem3d L=2 solution: levels %s above %s, area %s, count %s" % (levels, iso.above, iso.area, iso.count))
    assert iso.ts is None and (np.diff(iso.above) <= 0).all() and 0.0 < iso.above[-1] and iso.above[0] <= 8.0 + 1e-12
    assert iso.reached.all() and all(iso.triangles(l).shape == (iso.count[l], 3, 3) for l in range(4))
    loc, backend = M._locator_of(sol.geometry)
    zv, S = M._nodal_values(sol.geometry, sol.z, backend, "test")
    rows, counts = np.empty((4, 5)), np.empty(4, dtype=np.int64)
    _lib.call("mgb_geo_isosurfaces", loc, 1, (C.c_void_p * 1)(zv.handle.value), S, 0, 4, _lib.dptr(levels), 1, _lib.dptr(rows),
              counts.ctypes.data_as(_lib.c_ll_p), None)
    assert rows.tobytes() == iso.rows.tobytes() and np.array_equal(counts, iso.count)
    par = M.parabolic_solve(M.fem3d_mpi(2, 1), h=0.5, p=2.0)
    assert len(par.u) == len(par.ts) == 3
    u0 = par.u[0].to_numpy()[:, 0]
    cs = [u0.min() + 0.3 * (u0.max() - u0.min()), u0.min() + 0.6 * (u0.max() - u0.min())]
    hist = M.isosurfaces(par, cs, triangles=False)
    for v in (hist.above, hist.area, hist.excess, hist.count, hist.reached):
        assert v.shape == (len(par.ts), 2)
    print("3-D parabolic run: above %s, area %s" % (hist.above.tolist(), hist.area.tolist()))
    assert np.array_equal(hist.ts, par.ts) and (hist.above[:, 0] >= hist.above[:, 1]).all()
    one = M.isosurfaces(par, cs[1])
    assert one.above.shape == (3,) and one.rows[:, 0].tobytes() == hist.rows[:, 1].tobytes()
    assert one.triangles(0, 2).shape == (one.count[2], 3, 3)
    single = M.isosurfaces(par.geometry, cs[1], z=par.u[1])
    assert single.rows[0, 0].tobytes() == one.rows[1, 0].tobytes() and single.triangles().tobytes() == one.triangles(0, 1).tobytes()
