"""flow_lines() on the device (csrc/flowline.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-seed routine and against the longdouble yardstick tests/flowline_reference.py.

Shapes, chosen for what can break: fem2d L = 2, 3 and fem3d L = 1 with k = 1, 3 (every instantiation family, one element and
many); 1, 63, 64, 65 and 300 seeds (one lane, a partial wave, a full wave, a second workgroup at 64, several workgroups at every
workgroup size), each at the workgroup sizes 64, 128 and 256; max_steps <= 256.

Bars: against the host restatement status, count, end element, offsets and elements equal; points, end, length, u_start and
u_end BIT FOR BIT (both sides run the same IEEE + - * / and sqrt with contraction off); time bit for bit for p = 1 and p = 2,
for other p within 4 eps of the sum of its (positive) terms, the device and host pow differing.  Against the yardstick the bars
of tests/flowline_reference.py and the 1 % cap on undecided steps.  Measured on the device: time for p = 1.5 at most 0.70 of its
bar; against the yardstick points 0.015, length and time 0.002 of their bars, no undecided step."""
import ctypes as C

import numpy as np
import pytest

import flowline_reference as FR
import flowline_util as FU

pytestmark = pytest.mark.gpu
MESHES = [("fem2d", 2, None), ("fem2d", 3, None), ("fem3d", 1, 1), ("fem3d", 1, 3)]


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_GEO = {}


def mesh(M, kind, L, k=None):
    """(device geometry, host mesh) of the same nodes."""
    if (kind, L, k) not in _GEO:
        geo = M.fem2d_mpi(L) if kind == "fem2d" else M.fem3d_mpi(L, k=k)
        host = FU.host_mesh(kind, L, k)
        assert np.array_equal(geo.x.to_numpy().reshape(host.n, -1), host.x)
        _GEO[(kind, L, k)] = (geo, host)
    return _GEO[(kind, L, k)]


def smooth(x):
    s = np.sin(1.7 * x[:, 0] + 0.5) * np.cos(1.3 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 1] + 0.9 * x[:, 0]
    return s if x.shape[1] == 2 else s + 0.4 * x[:, 2] * x[:, 0] + 0.6 * x[:, 2]


def seeds_of(h, m):
    return FU.seeds_2d(m) if h.x.shape[1] == 2 else FU.seeds_3d(m)


def batch(M, geo, fields, seeds, **kw):
    """flow_lines() of several fields in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(geo, np.arange(float(len(fields))), [M.HPCMatrix(np.asarray(z).reshape(len(z), -1)) for z in fields])
    fl = M.flow_lines(sol, seeds, **kw)
    assert np.array_equal(fl.ts, sol.ts)
    return fl


@pytest.mark.parametrize("m", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("kind,L,k", MESHES)
def test_device_against_host(M, lib, kind, L, k, m):
    geo, h = mesh(M, kind, L, k)
    z = np.stack([np.zeros(h.n), smooth(h.x)], axis=1)      # column 1 of 2: a wrong stride or column shows
    seeds = seeds_of(h, m)
    for p, direction, steps in ((1.0, 1, 256), (2.0, -1, 40), (1.5, 1, 40)):
        host = FU.host_flow_lines(lib, h, [z], seeds, p=p, direction=direction, max_steps=steps, u=1)
        for wg in (64, 128, 256):
            fl = M.flow_lines(geo, seeds, p=p, u=1, z=z, direction=direction, max_steps=steps, workgroup=wg)
            FU.same_as_host("%s L=%d k=%s m=%d p=%g wg=%d" % (kind, L, k, m, p, wg), FU.device_result(fl), host, p)
        assert fl.status.shape == (m,) and fl.end.shape == (m, h.x.shape[1]) and fl.ts is None
        i = m - 1
        assert fl.path(i).tobytes() == host.path(0, i)[0].tobytes() and np.array_equal(fl.elements(i), host.path(0, i)[1])
        assert fl.path(i).shape == (fl.count[i], h.x.shape[1])
    assert host.count.max() > 2


@pytest.mark.parametrize("kind,L,k", MESHES)
def test_device_against_yardstick(M, lib, kind, L, k):
    """the closed forms (u = x; u = |x|^2 where the element reproduces it) and the one-step replay, on the device's own paths"""
    geo, h = mesh(M, kind, L, k)
    dim = h.x.shape[1]
    seeds = seeds_of(h, 10)
    tol = lambda ds, end=None: ds * 2.0 ** -40 + 2e-12 * (1.0 if end is None else float(np.sqrt((end ** 2).sum()) / np.abs(end).max()))
    z = h.x[:, 0].copy()
    for p in (1.0, 1.5, 2.0):
        fl = M.flow_lines(geo, seeds, p=p, z=z, max_steps=64)
        t = tol(fl.ds)
        assert (fl.status == M.FlowLines.EXIT).all()
        assert np.abs(fl.end[:, 0] - 1).max() <= t and np.abs(fl.end[:, 1:] - seeds[:, 1:]).max() <= t
        assert np.abs(fl.length - (1 - seeds[:, 0])).max() <= t and np.abs(fl.time - (1 - seeds[:, 0])).max() <= t
    name = "device %s L=%d k=%s" % (kind, L, k)
    FU.against_lines(name + " u = x", FU.device_result(fl), h, [z], seeds, 2.0, 1, 64, 1e-12)
    FU.replay(name + " u = x", FU.device_result(fl), h, [z], 2.0, 1, 64, 1e-12)
    if k != 1:
        z = (h.x ** 2).sum(axis=1)
        fl = M.flow_lines(geo, seeds, p=1.0, z=z, max_steps=64, ds=0.125)
        end = seeds / np.abs(seeds).max(axis=1)[:, None]
        assert (fl.status == M.FlowLines.EXIT).all()
        for i in range(len(seeds)):
            t = tol(0.125, end[i])
            want = np.sqrt((end[i] ** 2).sum()) - np.sqrt((seeds[i] ** 2).sum())
            assert np.abs(fl.end[i] - end[i]).max() <= t and abs(fl.length[i] - want) <= t and abs(fl.time[i] - fl.length[i]) <= t
        FU.replay(name + " |x|^2", FU.device_result(fl), h, [z], 1.0, 1, 64, 1e-12)
        down = M.flow_lines(geo, seeds, p=2.0, z=z, direction=-1, ds=0.125, gmin=0.25)
        # 2 r <= gmin = 2 ds where the stall is seen: at x_k or, by step 5 of the rule, at the midpoint ds / 2 ahead of it
        assert (down.status == M.FlowLines.STALLED).all() and (np.sqrt((down.end ** 2).sum(axis=1)) <= 1.5 * 0.125 + 1e-15).all()
    z = smooth(h.x)
    for direction in (1, -1):
        fl = M.flow_lines(geo, seeds, p=1.5, z=z, direction=direction, max_steps=32)
        FU.against_lines(name + " smooth", FU.device_result(fl), h, [z], seeds, 1.5, direction, 32, 1e-12)
        FU.replay(name + " smooth dir %d" % direction, FU.device_result(fl), h, [z], 1.5, direction, 32, 1e-12)


@pytest.mark.parametrize("kind,L,k", [("fem2d", 3, None), ("fem3d", 1, 3)])
def test_batch(M, lib, kind, L, k):
    """3 fields x m seeds in one call, one field with a NaN node: every row equals its single call bit for bit; a repeated call
    equals the first; paths=False gives the same summaries and needs no path buffer."""
    geo, h = mesh(M, kind, L, k)
    m = 70
    seeds = seeds_of(h, m)
    seeds[5] = 7.0      # outside
    z0, z2 = smooth(h.x), h.x[:, 0] - 0.5 * h.x[:, 1]
    z1 = z0.copy()
    z1[h.block * (h.nel // 2) + 1] = np.nan
    fields = [z0, z1, z2]
    kw = dict(p=2.0, max_steps=48)
    fl = batch(M, geo, fields, seeds, **kw)
    assert fl.status.shape == (3, m) and fl.end.shape == (3, m, h.x.shape[1])
    host = FU.host_flow_lines(lib, h, fields, seeds, **kw)
    FU.same_as_host("batch %s" % kind, FU.device_result(fl), host, 2.0)
    assert (fl.status[1] == M.FlowLines.NONFINITE).any() and (fl.status[:, 5] == M.FlowLines.OUTSIDE).all()
    assert not (fl.status[[0, 2]] == M.FlowLines.NONFINITE).any()
    for b, z in enumerate(fields):
        one = M.flow_lines(geo, seeds, z=z, **kw)
        assert one.rows.tobytes() == fl.rows[b].tobytes() and one.end.tobytes() == fl.end[b].tobytes()
        assert np.array_equal(one.status, fl.status[b]) and np.array_equal(one.count, fl.count[b])
        assert np.array_equal(one.end_element, fl.end_element[b])
        for i in (0, 5, 63, 64, m - 1):
            assert one.path(i).tobytes() == fl.path(i, b).tobytes() and np.array_equal(one.elements(i), fl.elements(i, b))
    again = batch(M, geo, fields, seeds, **kw)
    assert again.rows.tobytes() == fl.rows.tobytes() and again._pts.tobytes() == fl._pts.tobytes()
    assert np.array_equal(again._offsets, fl._offsets) and np.array_equal(again._elem, fl._elem)
    bare = batch(M, geo, fields, seeds, paths=False, **kw)
    assert bare.rows.tobytes() == fl.rows.tobytes() and bare.end.tobytes() == fl.end.tobytes()
    assert np.array_equal(bare.status, fl.status) and np.array_equal(bare.count, fl.count) and bare._pts is None
    with pytest.raises(ValueError):
        bare.path(0)
    # no path buffer: a max_steps whose fixed-stride buffer would pass 2^31 - 1 entries is refused with paths and runs without
    big = dict(p=2.0, z=z2, max_steps=2 ** 24)
    with pytest.raises(ValueError):
        M.flow_lines(geo, seeds, **big)
    far = M.flow_lines(geo, seeds, paths=False, **big)
    ref = M.flow_lines(geo, seeds, p=2.0, z=z2, max_steps=256)
    assert far.rows.tobytes() == ref.rows.tobytes() and np.array_equal(far.status, ref.status)
    empty = M.flow_lines(geo, np.empty((0, h.x.shape[1])), z=z2)
    assert empty.status.shape == (0,) and empty.end.shape == (0, h.x.shape[1]) and empty._offsets.tolist() == [0]


def test_real_solve(M, lib):
    """fem2d_mpi_solve(L=3, p=1.5): 64 seeds, both directions, device against host; u rises along +1 and falls along -1 on every
    line that ends EXIT or STALLED, up to one step's worth ds max a of slack."""
    sol = M.fem2d_mpi_solve(L=3, p=1.5)
    h = FU.host_mesh("fem2d", 3)
    assert np.array_equal(sol.geometry.x.to_numpy().reshape(h.n, -1), h.x)
    z = np.ascontiguousarray(M.mpi_to_native(sol).z).reshape(h.n, -1)
    seeds = FU.seeds_2d(64)
    grads = M.interpolate(sol, seeds, grad=True)[1][:, 0, :]
    for direction in (1, -1):
        fl = M.flow_lines(sol, seeds, p=1.5, direction=direction, max_steps=256)
        host = FU.host_flow_lines(lib, h, [z], seeds, p=1.5, direction=direction, max_steps=256)
        FU.same_as_host("solve dir %d" % direction, FU.device_result(fl), host, 1.5)
        ends = np.isin(fl.status, (M.FlowLines.EXIT, M.FlowLines.STALLED))
        print("solve dir %d: status counts %s" % (direction, np.bincount(fl.status, minlength=5).tolist()))
        for i in np.flatnonzero(ends):
            g = M.interpolate(sol, fl.path(i), grad=True)[1][:, 0, :]
            slack = fl.ds * np.sqrt((g ** 2).sum(axis=1)).max()
            assert direction * (fl.end_value[i] - fl.start_value[i]) >= -slack, (direction, i)
        assert np.isfinite(grads).all()


def test_parabolic_run(M, lib):
    """parabolic_solve(fem2d L=3, h=0.25, p=2): 5 snapshots in ONE call; ts carried; every snapshot equals its single call"""
    geo = M.fem2d_mpi(3)
    par = M.parabolic_solve(geo, h=0.25, p=2.0)
    assert len(par.ts) == 5
    seeds = FU.seeds_2d(40)
    fl = M.flow_lines(par, seeds, p=2.0, max_steps=64)
    assert np.array_equal(fl.ts, par.ts) and fl.status.shape == (5, 40) and fl.end.shape == (5, 40, 2)
    for b in range(5):
        one = M.flow_lines(geo, seeds, p=2.0, z=par.u[b], max_steps=64)
        assert one.rows.tobytes() == fl.rows[b].tobytes() and one.end.tobytes() == fl.end[b].tobytes()
        assert np.array_equal(one.status, fl.status[b]) and np.array_equal(one.count, fl.count[b])
        for i in (0, 39):
            assert one.path(i).tobytes() == fl.path(i, b).tobytes() and np.array_equal(one.elements(i), fl.elements(i, b))
    with pytest.raises(ValueError):
        M.flow_lines(par, seeds, z=par.u[0])


def test_argument_errors(M, lib):
    geo, h = mesh(M, "fem2d", 2)
    z, seeds = h.x[:, 0].copy(), FU.seeds_2d(3)
    ok = dict(z=z)
    assert M.flow_lines(geo, seeds, **ok).status.shape == (3,)
    for kw in (dict(ds=0.0), dict(ds=-1.0), dict(ds=np.nan), dict(ds=np.inf), dict(max_steps=0), dict(max_steps=True), dict(gmin=-1.0),
               dict(gmin=np.nan), dict(direction=0), dict(direction=2), dict(p=0.5), dict(p=np.nan), dict(p=np.inf), dict(u=1),
               dict(u=-2), dict(workgroup=32), dict(max_steps=2 ** 30)):
        with pytest.raises((ValueError, IndexError)):
            M.flow_lines(geo, seeds, **{**ok, **kw})
    with pytest.raises(TypeError):
        M.flow_lines(geo, seeds, p=lambda x: 2.0, **ok)
    for bad in (seeds[:, :1], seeds.ravel(), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            M.flow_lines(geo, bad, **ok)
    with pytest.raises(ValueError):
        M.flow_lines(geo, seeds, z=z[:-1])
    with pytest.raises(ValueError):
        M.flow_lines(geo, seeds)      # a Geometry without z=
    with pytest.raises(ValueError):
        M.flow_lines(M.fem1d_mpi(3), np.zeros((2, 1)), z=np.zeros(16))
    with pytest.raises(TypeError):
        M.flow_lines(object(), seeds)
    # the C entry point itself: MGB_E_ARG before anything is launched
    from mgb_amd import _lib
    loc, backend = M._locator_of(geo)
    zv = M.HPCVector(z, backend)
    table = (C.c_void_p * 1)(zv.handle.value)
    rows, end = np.full((3, 4), 7.0), np.full((3, 2), 7.0)
    ints = [np.full(3, -7, dtype=np.int32) for _ in range(3)]
    hp = C.c_void_p()

    def call(B=1, S=1, u=0, m=3, p=2.0, direction=1, ds=None, steps=16, gmin=1e-12, wg=0, tab=table, paths=None, sd=seeds):
        dsv = C.c_double(0.0 if ds is None else ds)
        return lib.mgb_geo_flow_lines(loc, B, tab, S, u, m, _lib.dptr(sd), p, direction, None if ds is None else C.cast(C.byref(dsv), _lib.c_dbl_p),
                                      steps, gmin, wg, _lib.dptr(rows), _lib.dptr(end), *map(_lib.iptr, ints), None, paths)

    assert call() == 0
    first = rows.copy()
    for kw in (dict(B=0), dict(B=65536), dict(S=0), dict(S=2), dict(u=1), dict(u=-1), dict(m=-1), dict(p=0.5), dict(p=np.nan),
               dict(direction=0), dict(ds=0.0), dict(ds=np.inf), dict(steps=0), dict(gmin=-1.0), dict(gmin=np.inf), dict(wg=32),
               dict(tab=None), dict(tab=(C.c_void_p * 1)(None)), dict(sd=None), dict(steps=2 ** 30, paths=C.byref(hp))):
        assert call(**kw) == FU.MGB_E_ARG, kw
        assert b"flow_lines" in lib.mgb_last_error()
    foreign = M.HPCVector(z, M.HPCBackend(0))      # the right length, on a second context of the same device
    assert call(tab=(C.c_void_p * 1)(foreign.handle.value)) == FU.MGB_E_ARG and b"another context" in lib.mgb_last_error()
    short = M.HPCVector(z[:-1], backend)
    assert call(tab=(C.c_void_p * 1)(short.handle.value)) == FU.MGB_E_ARG
    assert rows.tobytes() == first.tobytes() and hp.value is None      # nothing was written
    assert call(m=0) == 0


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem2d_mpi(2, backend=be)
    n = g.x.shape[0]
    z = M.HPCMatrix(g.x.to_numpy().reshape(n, 2), be)
    seeds = FU.seeds_2d(3)
    assert (M.flow_lines(g, seeds, z=z).status == M.FlowLines.EXIT).all()      # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                                  # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.flow_lines(g, seeds, z=z)
        rows, end = np.zeros((3, 4)), np.zeros((3, 2))
        ints = [np.zeros(3, dtype=np.int32) for _ in range(3)]
        assert lib.mgb_geo_flow_lines(loc, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 3, _lib.dptr(seeds), 2.0, 1, None, 16, 1e-12, 0,
                                      _lib.dptr(rows), _lib.dptr(end), *map(_lib.iptr, ints), None, None) == FU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
