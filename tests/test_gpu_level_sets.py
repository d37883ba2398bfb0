"""level_sets() on the device (csrc/levelset.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-item routine and against the numpy yardstick tests/levelset_reference.py.

Shapes, chosen for what can break: fem2d L=2 r=0 (48 items, under one workgroup), L=4 r=0 (768 items, 3 workgroups: offsets
across workgroups), L=3 r=2 (3072 items, 12 workgroups: the basis path), L=5 r=3 (196608 items, 768 workgroups: the finish and
the scan fold chunks of 3), fem1d L=3, a batch of 3 fields x 4 levels with a level out of range and a NaN node, and the
degenerate r = 0 cases of test_levelset_host.py.

Bars: against the host restatement counts, offsets and items equal, endpoints and maxima BIT FOR BIT (both sides run the same
IEEE + - * / with contraction off), the three sums within 1e-12 of the sum of their absolute terms; against numpy the bars of
tests/levelset_util.py.

Argument errors: every MGB_E_ARG condition of the contract is provoked on the device entry point except one, more than INT_MAX
items per row: at refine = 3 that takes 5.6 million triangles (fem2d L = 12, 58 million nodes), far from a quick test; the
check is one comparison in front of the allocation (capi.cpp) and again in front of the launch (levelset.hip)."""
import ctypes as C

import numpy as np
import pytest

import levelset_reference as LR
import levelset_util as LU

pytestmark = pytest.mark.gpu
LEVELS = [0.37, 0.91, 1.37]
NULL_FIELD = object()


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_GEO = {}


def mesh(M, kind, L):
    """(device geometry, host mesh) of the same nodes."""
    if (kind, L) not in _GEO:
        geo, host = getattr(M, kind + "_mpi")(L), LU.host_mesh(kind, L)
        assert np.array_equal(geo.x.to_numpy().reshape(host.n, -1), host.x)
        _GEO[(kind, L)] = (geo, host)
    return _GEO[(kind, L)]


def batch(M, geo, fields, levels, **kw):
    """level_sets() of several fields in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(geo, np.arange(float(len(fields))), [M.HPCMatrix(np.asarray(z).reshape(len(z), -1)) for z in fields])
    ls = M.level_sets(sol, levels, **kw)
    assert np.array_equal(ls.ts, sol.ts)
    return ls


def same_as_host(name, dev, host, x, fields, levels, refine, u=0):
    """Device Result against the host Result: everything discrete equal, endpoints and maxima bit for bit, sums at 1e-12."""
    assert np.array_equal(dev.counts, host.counts), name
    assert np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.item, host.item), name
    differ = int((dev.seg != host.seg).sum())
    print("%s: %d segments, %d endpoint coordinates differ from the host restatement" % (name, len(host.seg), differ))
    assert dev.seg.tobytes() == host.seg.tobytes(), name
    assert dev.rows[:, :, 3:].tobytes() == host.rows[:, :, 3:].tobytes(), name
    worst = 0.0
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(x.shape[0], -1)
        for l, R in enumerate(LR.level_sets(x, z[:, u], np.atleast_1d(levels), refine)):
            if np.isnan(R.rows).any():
                assert np.isnan(dev.rows[b, l]).all() and np.isnan(host.rows[b, l]).all()
                continue
            gap, bar = np.abs(dev.rows[b, l, :3] - host.rows[b, l, :3]), LU.KTOL * R.abs_terms.astype(np.float64)
            worst = max([worst] + [g / s for g, s in zip(gap, bar) if s > 0])
            assert (gap <= bar).all(), (name, b, l, gap, bar)
    print("%s: sums against the host restatement, largest ratio to the bar %.3e" % (name, worst))


@pytest.mark.parametrize("kind,L,refine", [("fem2d", 2, 0), ("fem2d", 4, 0), ("fem2d", 3, 2), ("fem2d", 5, 3), ("fem1d", 3, 0)])
def test_device_against_host_and_numpy(M, lib, kind, L, refine):
    geo, h = mesh(M, kind, L)
    if kind == "fem2d":
        z, levels = np.stack([np.zeros(h.n), LU.paraboloid(h.x)], axis=1), LEVELS
    else:
        z, levels = np.stack([np.ones(h.n), h.x[:, 0] ** 2 - 0.3], axis=1), [-0.2, 0.0, 0.25, 0.7]
    name = "%s L=%d r=%d" % (kind, L, refine)
    ls = M.level_sets(geo, levels, u=1, z=z, refine=refine)
    assert ls.rows.shape == (1, len(levels), 5) and ls.above.shape == (len(levels),) and ls.ts is None
    dev = LU.device_result(ls, 1, len(levels))
    host = LU.host_level_sets(lib, h, [z], levels, refine, u=1)
    same_as_host(name, dev, host, h.x, [z], levels, refine, u=1)
    LU.against_reference(name + " device", dev, h.x, [z], levels, refine, u=1)
    assert (ls.count[:3] > 0).all() and ls.reached[:3].all()
    if kind == "fem2d":
        seg = ls.segments(1)
        assert seg.shape == (ls.count[1], 2, 2) and np.array_equal(seg.reshape(-1, 4), dev.row(0, 1)[0])
        assert np.array_equal(ls.elements(1), dev.row(0, 1)[1] // (6 * 4 ** refine)) and ls.elements(1).max() < h.nel
        with pytest.raises(ValueError):
            ls.points(0)
    else:
        assert np.array_equal(ls.points(1), dev.row(0, 1)[0][:, 0]) and np.array_equal(ls.directions(1), [-1, 1])
        assert ls.length[1] == 2.0 and not ls.reached[3]
        with pytest.raises(ValueError):
            ls.segments(0)


def test_batch_with_a_level_out_of_range_and_a_nan_node(M, lib):
    """3 fields x 4 levels in one call: against the host, and bit for bit the single-field, single-level calls; a repeated call
    and segments=False return the same bits."""
    geo, h = mesh(M, "fem2d", 4)
    rng = np.random.default_rng(7)
    base = LU.paraboloid(h.x)
    fields = [base, np.sin(3.0 * h.x[:, 0] + 0.5) * np.cos(2.0 * h.x[:, 1]) + 0.8, base + 0.1 * rng.standard_normal(h.n)]
    fields[1][7 * 40 + 2] = np.nan
    levels = [0.37, 0.91, 5.0, 1.37]
    ls = batch(M, geo, fields, levels)
    assert ls.above.shape == ls.length.shape == ls.excess.shape == ls.count.shape == ls.reached.shape == (3, 4)
    dev = LU.device_result(ls, 3, 4)
    host = LU.host_level_sets(lib, h, fields, levels)
    same_as_host("batch 3 x 4", dev, host, h.x, fields, levels, 0)
    LU.against_reference("batch 3 x 4 device", dev, h.x, fields, levels, 0)
    assert np.isnan(ls.rows[1]).all() and np.isfinite(ls.rows[[0, 2]]).all() and (ls.count[1] > 0).any()
    assert not ls.reached[:, 2].any() and (ls.count[:, 2] == 0).all() and (ls.rows[[0, 2], 2, 3] < 0).all()
    again = batch(M, geo, fields, levels)
    assert again.rows.tobytes() == ls.rows.tobytes() and again._seg.tobytes() == ls._seg.tobytes()
    assert np.array_equal(again._item, ls._item) and np.array_equal(again._offsets, ls._offsets)
    cheap = batch(M, geo, fields, levels, segments=False)
    assert cheap.rows.tobytes() == ls.rows.tobytes() and np.array_equal(cheap.count, ls.count)
    with pytest.raises(ValueError):
        cheap.segments(0, 0)
    for b in range(3):
        for l in range(4):
            one = M.level_sets(geo, levels[l], z=fields[b])
            assert isinstance(one.above, float) and isinstance(one.count, int) and isinstance(one.reached, bool)
            assert one.rows[0, 0].tobytes() == ls.rows[b, l].tobytes() and one.count == ls.count[b, l]
            assert one.segments().tobytes() == ls.segments(l, b).tobytes()
            assert np.array_equal(one.elements(), ls.elements(l, b))


@pytest.mark.parametrize("case", ["u = x", "u = c", "outside", "inf node"])
def test_degenerate_cases_at_refine_0(M, lib, case):
    for L in (2, 3):
        geo, h = mesh(M, "fem2d", L)
        if case == "u = x":
            fields, levels = [h.x[:, 0].copy()], [0.0]
        elif case == "u = c":
            fields, levels = [np.full(h.n, 0.3)], [0.3]
        elif case == "outside":
            fields, levels = [LU.paraboloid(h.x)], [2.5, -0.5]
        else:
            z = LU.paraboloid(h.x)
            zb = z.copy()
            zb[7 * 5 + 1] = np.inf
            fields, levels = [zb, z], [0.37]
        ls = batch(M, geo, fields, levels)
        dev = LU.device_result(ls, len(fields), len(levels))
        host = LU.host_level_sets(lib, h, fields, levels)
        same_as_host("%s L=%d" % (case, L), dev, host, h.x, fields, levels, 0)
        LU.against_reference("%s L=%d device" % (case, L), dev, h.x, fields, levels, 0)
        if case == "u = x":
            assert abs(ls.length[0, 0] - 2.0) <= 1e-12 and abs(ls.above[0, 0] - 2.0) <= 1e-12
        elif case == "u = c":
            assert np.array_equal(ls.rows[0, 0], np.zeros(5)) and ls.count[0, 0] == 0 and not ls.reached[0, 0]
        elif case == "outside":
            assert not ls.reached.any() and ls.above[0, 0] == 0.0 and abs(ls.above[0, 1] - 4.0) <= 1e-12
        else:
            assert np.isnan(ls.rows[0]).all() and np.isfinite(ls.rows[1]).all()


def test_argument_errors(M):
    geo, h = mesh(M, "fem2d", 2)
    z = LU.paraboloid(h.x)
    for kw, err in ((dict(levels=np.nan), ValueError), (dict(levels=[0.1, np.inf]), ValueError), (dict(levels=[]), ValueError),
                    (dict(levels=[[0.1]]), ValueError), (dict(refine=4), ValueError), (dict(refine=-1), ValueError),
                    (dict(refine=1.0), ValueError), (dict(u=1), ValueError), (dict(z=z[:-1]), ValueError)):
        with pytest.raises(err):
            M.level_sets(geo, **{**dict(levels=0.37, z=z), **kw})
    with pytest.raises(ValueError):
        M.level_sets(mesh(M, "fem1d", 3)[0], 0.1, z=np.zeros(16), refine=1)
    with pytest.raises(NotImplementedError, match="isosurfaces"):
        M.level_sets(M.fem3d_mpi(1, 1), 0.1, z=np.zeros(8))
    with pytest.raises(TypeError):
        M.level_sets(z, 0.1)
    # the C entry point: MGB_E_ARG before anything is launched
    from mgb_amd import _lib
    loc, backend = M._locator_of(geo)
    zv = M.HPCVector(z, backend)
    other = M.HPCVector(z[:-1], backend)
    rows, counts, lv = np.empty(5), np.empty(1, dtype=np.int64), np.array([0.37])
    lib = _lib.load()

    def rc(loc=loc, B=1, vec=zv, S=1, u=0, nl=1, lvp=_lib.dptr(lv), refine=0, out=_lib.dptr(rows),
           cnt=counts.ctypes.data_as(_lib.c_ll_p)):
        table = None if vec is None else (C.c_void_p * 1)(None if vec is NULL_FIELD else vec.handle.value)
        return lib.mgb_geo_level_sets(loc, B, table, S, u, nl, lvp, refine, out, cnt, None)

    assert rc() == 0
    foreign = M.HPCVector(z, M.HPCBackend(0))      # the right length, on a second context of the same device
    for kw in (dict(loc=None), dict(vec=None), dict(vec=NULL_FIELD), dict(lvp=None), dict(out=None), dict(cnt=None), dict(B=0), dict(nl=0),
               dict(B=65536), dict(nl=65536), dict(S=0), dict(u=1), dict(u=-1), dict(refine=4), dict(refine=-1), dict(vec=other),
               dict(vec=foreign), dict(lvp=_lib.dptr(np.array([np.inf])))):
        assert rc(**kw) == LU.MGB_E_ARG, kw
    assert rc(vec=foreign) == LU.MGB_E_ARG and b"another context" in lib.mgb_last_error()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    n = g.x.shape[0]
    z = M.HPCMatrix(np.ones((n, 2)), be)
    assert M.level_sets(g, 0.5, z=z).above == 2.0                        # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.level_sets(g, 0.5, z=z)
        rows, counts, lv = np.zeros(5), np.zeros(1, dtype=np.int64), np.array([0.5])
        assert lib.mgb_geo_level_sets(loc, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows),
                                      counts.ctypes.data_as(_lib.c_ll_p), None) == LU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)


@pytest.mark.parametrize("refine", [0, 1])
def test_orientation_on_elements_of_negative_determinant(M, lib, refine):
    """A mesh half of whose elements have a negative determinant: the device equals the host restatement bit for bit there too,
    and the above side is still on the left -- Green's sum 1/2 sum (x0 y1 - x1 y0) is positive and equals column [0] around a
    disk that is above, negative and equal to column [0] - 4 around a disk that is below."""
    h = LU.host_mesh("fem2d", 3, mixed=True)
    if "mixed" not in _GEO:
        _GEO["mixed"] = M.fem2d_mpi(3, K=LU.K_MIXED)
    geo = _GEO["mixed"]
    assert np.array_equal(geo.x.to_numpy().reshape(h.n, 2), h.x)
    xe = h.x.reshape(-1, 7, 2)
    det = (xe[:, 1, 0] - xe[:, 0, 0]) * (xe[:, 2, 1] - xe[:, 0, 1]) - (xe[:, 1, 1] - xe[:, 0, 1]) * (xe[:, 2, 0] - xe[:, 0, 0])
    assert (det < 0).any() and (det > 0).any()
    z = LU.paraboloid(h.x)
    fields, levels = [-z, z], [-0.37, 0.37]
    ls = batch(M, geo, fields, levels, refine=refine)
    dev = LU.device_result(ls, 2, 2)
    host = LU.host_level_sets(lib, h, fields, levels, refine)
    name = "negative determinants r=%d" % refine
    same_as_host(name, dev, host, h.x, fields, levels, refine)
    LU.against_reference(name + " device", dev, h.x, fields, levels, refine)
    disk, hole = ls.segments(0, 0).reshape(-1, 4), ls.segments(1, 1).reshape(-1, 4)
    print("%s: Green sums %.15f %.15f, columns [0] %.15f %.15f" % (name, LU.green(disk), LU.green(hole), ls.above[0, 0], ls.above[1, 1]))
    assert LU.green(disk) > 0 and abs(LU.green(disk) - ls.above[0, 0]) <= 1e-12 * ls.above[0, 0]
    assert LU.green(hole) < 0 and abs(LU.green(hole) - (ls.above[1, 1] - 4.0)) <= 1e-12 * 4.0
    used = np.unique(ls.elements(0, 0))
    assert (det[used] < 0).any() and (det[used] > 0).any()


def test_solutions(M):
    """An obstacle solve and a parabolic run: shapes of every field, ts, above decreasing in c, and the rows of the C entry point."""
    from mgb_amd import _lib
    sol = M.amgb(M.fem2d_mpi(3), p=1.5, f=lambda x: np.array([5.0, 0, 0, 1.0]), g=lambda x: np.array([1.0, 10.0]),
                 cones=[([1, 2, 3], 1.5), ("linear", [0], [1.0], -0.3)])
    levels = np.array([0.31, 0.5, 0.7, 0.9])
    ls = M.level_sets(sol, levels, refine=1)
    for v in (ls.above, ls.length, ls.excess, ls.count, ls.reached):
        assert v.shape == (4,)
    print("obstacle u > 0.3: above %s, length %s, count %s" % (ls.above, ls.length, ls.count))
    assert ls.ts is None and (np.diff(ls.above) <= 0).all() and 0.0 < ls.above[0] <= 4.0 + 1e-12
    assert all(ls.segments(l).shape == (ls.count[l], 2, 2) for l in range(4))
    loc, backend = M._locator_of(sol.geometry)
    zv, S = M._nodal_values(sol.geometry, sol.z, backend, "test")
    rows, counts = np.empty((4, 5)), np.empty(4, dtype=np.int64)
    _lib.call("mgb_geo_level_sets", loc, 1, (C.c_void_p * 1)(zv.handle.value), S, 0, 4, _lib.dptr(levels), 1, _lib.dptr(rows),
              counts.ctypes.data_as(_lib.c_ll_p), None)
    assert rows.tobytes() == ls.rows.tobytes() and np.array_equal(counts, ls.count)
    par = M.parabolic_solve(M.fem2d_mpi(3), h=0.25, p=2.0)
    assert len(par.u) == 5
    hist = M.level_sets(par, [0.1, 0.3], segments=False)
    for v in (hist.above, hist.length, hist.excess, hist.count, hist.reached):
        assert v.shape == (5, 2)
    print("parabolic run: above %s, length %s" % (hist.above.tolist(), hist.length.tolist()))
    assert np.array_equal(hist.ts, par.ts) and (hist.above[:, 0] >= hist.above[:, 1]).all()
    one = M.level_sets(par, 0.3)
    assert one.above.shape == (5,) and one.rows[:, 0].tobytes() == hist.rows[:, 1].tobytes()
    assert one.segments(0, 4).shape == (one.count[4], 2, 2)
    single = M.level_sets(par.geometry, 0.3, z=par.u[2])
    assert single.rows[0, 0].tobytes() == one.rows[2, 0].tobytes() and single.segments().tobytes() == one.segments(0, 2).tobytes()
