"""path_lines() on the device (csrc/pathline.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-seed routine, against flow_lines() in the stationary case and against the longdouble yardstick
tests/pathline_reference.py.

Shapes, chosen for what can break: fem2d L = 2, 3 and fem3d (L, k) = (1, 1), (1, 3), (2, 2) (every instantiation, one element
and many); 1, 63, 64, 65 and 300 seeds (one lane, a partial wave, a full wave, a second workgroup at 64, several workgroups at
every size), each at the workgroup sizes 64, 128 and 256; B in {2, 3, 5} snapshots and 1, 3, 8 substeps, at most 32 steps; the
field in column 1 of 2; release indices mixed within every wave.

Bars: against the host restatement everything discrete equal and points, end and the five row columns BIT FOR BIT for
p = 1, 1.5 and 2 (both sides run the same IEEE + - * / and sqrt with contraction off).  For p = 1.75 (pow) device and host are
each held to the yardstick's one-step replay under the bars of tests/pathline_reference.py with the 1 % cap on undecided steps.
Measured on the device (p = 1.75, the host the same to three digits): points 0.011 of the bar on fem2d L = 3 and 0.008 on
fem3d L = 1, k = 3, length 0.001, no undecided step; the real runs end [DONE, EXIT] = [40, 0] at speed 1, [2, 38] at speed 64
(fem2d L = 3) and [4, 16] at speed 16 (fem3d L = 1, k = 2)."""
import ctypes as C

import numpy as np
import pytest

import flowline_reference as FR
import flowline_util as FU
import pathline_reference as PR
import pathline_util as PU

pytestmark = pytest.mark.gpu
MESHES = [("fem2d", 2, None), ("fem2d", 3, None), ("fem3d", 1, 1), ("fem3d", 1, 3), ("fem3d", 2, 2)]


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


def fields_of(h, B):
    return PU.fields_2d(h.x, B) if h.x.shape[1] == 2 else PU.fields_3d(h.x, B)


def seeds_of(h, m):
    return FU.seeds_2d(m) if h.x.shape[1] == 2 else FU.seeds_3d(m)


def times(B):
    return np.cumsum(np.concatenate([[0.0], 0.0625 + 0.03125 * (np.arange(B - 1) % 3)]))      # unequal slabs


def run(M, geo, fields, ts, seeds, **kw):
    sol = M.ParabolicSOL(geo, np.asarray(ts, dtype=np.float64), [M.HPCMatrix(np.asarray(z).reshape(len(z), -1)) for z in fields])
    return M.path_lines(sol, seeds, **kw)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("kind,L,k", MESHES)
def test_device_against_host(M, lib, kind, L, k, m):
    geo, h = mesh(M, kind, L, k)
    seeds = seeds_of(h, m)
    exits = longest = 0
    for ib, B in enumerate((2, 3, 5)):
        fields = [np.stack([np.zeros(h.n), z], axis=1) for z in fields_of(h, B)]      # column 1 of 2: a wrong stride or column shows
        ts = times(B)
        rel = (np.arange(m) * 7) % (B - 1)      # mixed within every wave
        for i_n, n in enumerate((1, 3, 8)):
            p = (1.0, 1.5, 2.0)[(ib + i_n) % 3]
            speed = 2.0 if (ib + i_n) % 2 else 0.5
            kw = dict(release=rel, substeps=n, p=p, speed=speed, u=1)
            host = PU.host_path_lines(lib, h, fields, ts, seeds, **kw)
            for wg in (64, 128, 256):
                pl = run(M, geo, fields, ts, seeds, workgroup=wg, **kw)
                PU.same_as_host("%s L=%d k=%s m=%d B=%d n=%d p=%g wg=%d" % (kind, L, k, m, B, n, p, wg), PU.device_result(pl), host)
            assert pl.status.shape == (m,) and pl.end.shape == (m, h.x.shape[1]) and np.array_equal(pl.ts, ts)
            assert np.array_equal(pl.release, rel) and pl.stop == B - 1 and pl.substeps == n
            i = m - 1
            assert pl.path(i).tobytes() == host.path(i)[0].tobytes() and np.array_equal(pl.elements(i), host.path(i)[1])
            assert pl.path(i).shape == (pl.count[i], h.x.shape[1]) and len(pl.times(i)) == pl.count[i]
            done = pl.status == M.PathLines.DONE
            assert (pl.count[done] == (B - 1 - rel[done]) * n + 1).all() and (pl.time[done] == ts[-1]).all()
            exits += int((pl.status == M.PathLines.EXIT).sum())
            longest = max(longest, int(pl.count.max()))
    assert longest > 8 and (exits > 0 or m == 1)


@pytest.mark.parametrize("kind,L,k", [("fem2d", 3, None), ("fem3d", 1, 3)])
def test_pow_against_the_yardstick(M, lib, kind, L, k):
    """p = 1.75 goes through pow, which differs between device and host: no bitwise claim, each side under the replay's bars"""
    geo, h = mesh(M, kind, L, k)
    seeds, fields, ts = seeds_of(h, 6), fields_of(h, 3), times(3)
    rel = np.arange(6) % 2
    kw = dict(release=rel, substeps=3, p=1.75, speed=0.5)
    name = "%s L=%d k=%s p=1.75" % (kind, L, k)
    dev = PU.device_result(run(M, geo, fields, ts, seeds, **kw))
    host = PU.host_path_lines(lib, h, fields, ts, seeds, **kw)
    for who, got in (("device", dev), ("host", host)):
        PU.against_lines("%s %s" % (who, name), got, h, fields, ts, seeds, rel, 2, 3, 1.75, -1, 0.5, 1e-12)
        PU.replay("%s %s" % (who, name), got, h, fields, ts, rel, 2, 3, 1.75, -1, 0.5, 1e-12)
    assert np.array_equal(dev.status, host.status) and np.array_equal(dev.count, host.count)


@pytest.mark.parametrize("kind,L,k", [("fem2d", 3, None), ("fem3d", 1, 2)])
def test_stationary_field_gives_the_flow_lines(M, lib, kind, L, k):
    """B equal snapshots, p = 1, speed 1, ts = 2^-3 arange(B), 4 substeps: the points and elements of flow_lines(direction=-1,
    ds=2^-5, max_steps=4 (B - 1)) bit for bit; DONE <-> MAXSTEPS, EXIT <-> EXIT; lengths within 2 count eps length"""
    geo, h = mesh(M, kind, L, k)
    B, seeds, z = 5, seeds_of(h, 70), fields_of(h, 1)[0]
    pl = run(M, geo, [z] * B, 2.0 ** -3 * np.arange(B), seeds, substeps=4, p=1.0, speed=1.0, direction=-1)
    fl = M.flow_lines(geo, seeds, p=1.0, z=z, direction=-1, ds=2.0 ** -5, max_steps=4 * (B - 1))
    F, P = M.FlowLines, M.PathLines
    assert not (fl.status == F.STALLED).any() and not (pl.rested > 0).any()
    assert np.array_equal(pl.status == P.DONE, fl.status == F.MAXSTEPS) and np.array_equal(pl.status == P.EXIT, fl.status == F.EXIT)
    assert (pl.status == P.DONE).any() and (pl.status == P.EXIT).any()
    assert np.array_equal(pl.count, fl.count) and np.array_equal(pl._offsets, fl._offsets)
    assert pl._pts.tobytes() == fl._pts.tobytes() and np.array_equal(pl._elem, fl._elem)
    assert pl.end.tobytes() == fl.end.tobytes() and np.array_equal(pl.end_element, fl.end_element)
    assert pl.start_value.tobytes() == fl.start_value.tobytes()
    assert (np.abs(pl.length - fl.length) <= 2 * pl.count * FR.EPS * fl.length).all()


@pytest.mark.parametrize("kind,L,k", [("fem2d", 3, None), ("fem3d", 2, 2)])
def test_batch_repeat_and_no_paths(M, lib, kind, L, k):
    """a batch with a NaN node, an outside seed and resting particles: every row equals its single-seed call bit for bit; a
    repeated call returns the same bits; paths=False gives the same rows and its path methods raise"""
    geo, h = mesh(M, kind, L, k)
    m = 70
    seeds = seeds_of(h, m)
    seeds[5] = 7.0      # outside
    zero = np.zeros(h.n)
    f = fields_of(h, 2)
    bad = f[1].copy()
    bad[h.block * (h.nel // 2) + 1] = np.nan
    fields, ts = [zero, zero, f[0], bad], np.array([0.0, 0.125, 0.25, 0.5])
    rel = np.arange(m) % 3      # released at 0: rests through the first slab; at 2: never rests
    kw = dict(release=rel, substeps=4, p=2.0, speed=1.0)
    pl = run(M, geo, fields, ts, seeds, **kw)
    PU.same_as_host("batch %s" % kind, PU.device_result(pl), PU.host_path_lines(lib, h, fields, ts, seeds, **kw))
    P = M.PathLines
    assert pl.status[5] == P.OUTSIDE and (pl.status == P.NONFINITE).any() and (pl.status != P.NONFINITE).any()
    inside = pl.status != P.OUTSIDE
    assert (pl.rested[inside & (rel == 0)] >= 4).all() and (pl.rested[inside & (rel == 2)] == 0).all()
    for i in (0, 1, 2, 5, 63, 64, m - 1) + tuple(np.flatnonzero(pl.status == P.NONFINITE)[:2]):
        one = run(M, geo, fields, ts, seeds[i: i + 1], **{**kw, "release": int(rel[i])})
        assert one.rows.tobytes() == pl.rows[i: i + 1].tobytes() and one.end.tobytes() == pl.end[i: i + 1].tobytes()
        assert one.status[0] == pl.status[i] and one.count[0] == pl.count[i] and one.rested[0] == pl.rested[i]
        assert one.path(0).tobytes() == pl.path(int(i)).tobytes() and np.array_equal(one.elements(0), pl.elements(int(i)))
    again = run(M, geo, fields, ts, seeds, **kw)
    assert again.rows.tobytes() == pl.rows.tobytes() and again._pts.tobytes() == pl._pts.tobytes()
    assert np.array_equal(again._offsets, pl._offsets) and np.array_equal(again._elem, pl._elem)
    bare = run(M, geo, fields, ts, seeds, paths=False, **kw)
    assert bare.rows.tobytes() == pl.rows.tobytes() and bare.end.tobytes() == pl.end.tobytes()
    assert np.array_equal(bare.status, pl.status) and np.array_equal(bare.count, pl.count) and bare._pts is None
    assert np.array_equal(bare.rested, pl.rested) and np.array_equal(bare.end_element, pl.end_element)
    for call in (lambda: bare.path(0), lambda: bare.elements(0), lambda: bare.times(0), lambda: bare.positions(1)):
        with pytest.raises(ValueError, match="paths=False"):
            call()
    # no path buffer: substeps whose fixed-stride buffer would pass 2^31 - 1 entries are refused with paths only
    with pytest.raises(ValueError, match="2\\^31"):
        run(M, geo, fields, ts, seeds, substeps=2 ** 23)
    empty = run(M, geo, fields, ts, np.empty((0, h.x.shape[1])))
    assert empty.status.shape == (0,) and empty.end.shape == (0, h.x.shape[1]) and empty._offsets.tolist() == [0]


def check_real_run(M, lib, par, h, seeds, name, speed=1.0):
    """Device against host on the snapshots of a real run; DONE particles end at ts[-1]; positions(j) is the point of path()
    whose times() entry is ts[j]; u at the recorded points is the blend of interpolate() of the two snapshots of the slab."""
    ts, B, n = np.asarray(par.ts), len(par.ts), 4
    rel = np.arange(len(seeds)) % (B - 1)
    pl = M.path_lines(par, seeds, p=2.0, substeps=n, release=rel, speed=speed)
    snaps = [np.ascontiguousarray(u.to_numpy()).reshape(h.n, -1) for u in par.u]
    host = PU.host_path_lines(lib, h, snaps, ts, seeds, release=rel, substeps=n, p=2.0, speed=speed)
    PU.same_as_host(name, PU.device_result(pl), host)
    P = M.PathLines
    print("%s: status counts %s" % (name, np.bincount(pl.status, minlength=4).tolist()))
    done = pl.status == P.DONE
    assert (done.any() or speed > 1.0) and (pl.time[done] == ts[-1]).all() and np.isin(pl.status, (P.DONE, P.EXIT)).all()
    for j in range(B):
        pos = pl.positions(j)
        for i in range(len(seeds)):
            t = pl.times(i)
            k = (j - int(rel[i])) * n      # the accepted steps it takes to be there
            alive = k >= 0 and (pl.status[i] == P.DONE or ts[j] <= pl.time[i])
            if alive:
                assert t[k] == ts[j] and np.array_equal(pos[i], pl.path(i)[k]), (name, j, i)
            else:
                assert np.isnan(pos[i]).all(), (name, j, i)
    vals = [M.interpolate(par.geometry, pl._pts, z=u)[:, 0] for u in par.u]      # every snapshot at every recorded point
    scale = max(float(np.abs(s[:, 0]).max()) for s in snaps)
    for i in range(len(seeds)):
        a, e = int(pl._offsets[i]), int(pl._offsets[i + 1])
        tol = 64 * FR.EPS * h.block * scale      # two evaluations of block-term sums, one with contraction and one without
        assert abs(pl.start_value[i] - vals[rel[i]][a]) <= tol, (name, i)
        if pl.status[i] == P.DONE:
            assert abs(pl.end_value[i] - vals[B - 1][e - 1]) <= tol, (name, i)
        else:
            t = pl.time[i]
            j = min(int(np.searchsorted(ts, t, side="right")) - 1, B - 2)
            th = (t - ts[j]) / (ts[j + 1] - ts[j])
            want = vals[j][e - 1] + th * (vals[j + 1][e - 1] - vals[j][e - 1])
            assert abs(pl.end_value[i] - want) <= tol + 8 * FR.EPS * abs(vals[j + 1][e - 1] - vals[j][e - 1]) * max(t, 1.0) / (ts[j + 1] - ts[j]), (name, i)
    return pl


def test_real_runs(M, lib):
    geo = M.fem2d_mpi(3)
    par = M.parabolic_solve(geo, p=2.0, ts=[0.0, 0.25, 0.5, 0.75, 1.0])
    h = FU.host_mesh("fem2d", 3)
    check_real_run(M, lib, par, h, FU.seeds_2d(40), "parabolic fem2d L=3")
    check_real_run(M, lib, par, h, FU.seeds_2d(40), "parabolic fem2d L=3, 64 times faster", speed=64.0)      # some leave the domain
    geo = M.fem3d_mpi(1, k=2)
    par = M.parabolic_solve(geo, h=0.5, p=2.0)
    check_real_run(M, lib, par, FU.host_mesh("fem3d", 1, 2), FU.seeds_3d(20), "parabolic fem3d L=1 k=2", speed=16.0)


def test_argument_errors(M, lib):
    geo, h = mesh(M, "fem2d", 2)
    seeds, fields, ts = FU.seeds_2d(3), fields_of(h, 3), times(3)
    assert run(M, geo, fields, ts, seeds).status.shape == (3,)
    for kw in (dict(substeps=0), dict(substeps=True), dict(substeps=1.5), dict(gmin=-1.0), dict(gmin=np.nan), dict(direction=0),
               dict(direction=2), dict(p=0.5), dict(p=np.nan), dict(p=np.inf), dict(u=1), dict(u=-2), dict(workgroup=32),
               dict(speed=0.0), dict(speed=-1.0), dict(speed=np.inf), dict(stop=0), dict(stop=3), dict(stop=1.0), dict(release=2),
               dict(release=-1), dict(release=[0, 1]), dict(release=0.5), dict(release=1, stop=1), dict(substeps=2 ** 30)):
        with pytest.raises((ValueError, IndexError)):
            run(M, geo, fields, ts, seeds, **kw)
    with pytest.raises(TypeError):
        run(M, geo, fields, ts, seeds, p=lambda x: 2.0)
    for bad in (seeds[:, :1], seeds.ravel(), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            run(M, geo, fields, ts, bad)
    with pytest.raises(ValueError):
        run(M, geo, fields[:1], ts[:1], seeds)      # one snapshot is no run in time
    with pytest.raises(ValueError):
        run(M, geo, fields, [0.0, 0.25, 0.25], seeds)
    for other in (geo, object()):
        with pytest.raises(TypeError, match="flow_lines"):
            M.path_lines(other, seeds)
    g1 = M.fem1d_mpi(3)
    with pytest.raises(ValueError, match="1-D"):
        run(M, g1, [np.zeros(16)] * 2, [0.0, 1.0], np.zeros((2, 1)))
    # the C entry point itself: MGB_E_ARG before anything is allocated, launched or written
    from mgb_amd import _lib
    loc, backend = M._locator_of(geo)
    vecs = [M.HPCVector(z, backend) for z in fields]
    table = (C.c_void_p * 3)(*[v.handle.value for v in vecs])
    rows, end = np.full((3, 5), 7.0), np.full((3, 2), 7.0)
    ints = [np.full(3, -7, dtype=np.int32) for _ in range(4)]
    rel0 = np.zeros(3, dtype=np.int32)
    hp = C.c_void_p()

    def call(B=3, S=1, u=0, m=3, stop=2, n=4, p=2.0, direction=-1, speed=1.0, gmin=1e-12, wg=0, tab=table, t=ts, paths=None, sd=seeds,
             rel=rel0, r=rows, i3=ints[3], lc=loc):
        ptr = lambda a, f: None if a is None else f(a)
        return lib.mgb_geo_path_lines(lc, B, tab, ptr(t, _lib.dptr), S, u, m, ptr(sd, _lib.dptr), ptr(rel, _lib.iptr), stop, n, p, direction,
                                      speed, gmin, wg, ptr(r, _lib.dptr), _lib.dptr(end), *map(_lib.iptr, ints[:3]), ptr(i3, _lib.iptr),
                                      paths)

    assert call() == 0
    first = rows.copy()
    bad_ts = [np.array(v) for v in ([0.0, 0.1, 0.1], [0.0, 0.2, 0.1], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf])]
    for kw in (dict(B=1), dict(B=65536), dict(S=0), dict(S=2), dict(u=1), dict(u=-1), dict(m=-1), dict(p=0.5), dict(p=np.nan),
               dict(direction=0), dict(speed=0.0), dict(speed=np.inf), dict(n=0), dict(gmin=-1.0), dict(gmin=np.inf), dict(wg=32),
               dict(stop=0), dict(stop=3), dict(rel=np.array([0, 2, 0], dtype=np.int32)), dict(rel=np.array([0, -1, 0], dtype=np.int32)),
               dict(tab=None), dict(tab=(C.c_void_p * 3)(vecs[0].handle.value, None, vecs[2].handle.value)), dict(sd=None),
               dict(t=None), dict(rel=None), dict(r=None), dict(i3=None), dict(lc=None), dict(n=2 ** 29, paths=C.byref(hp))) \
            + tuple(dict(t=v) for v in bad_ts):
        assert call(**kw) == PU.MGB_E_ARG, kw
        assert b"path_lines" in lib.mgb_last_error()
    foreign = M.HPCVector(fields[1], M.HPCBackend(0))      # the right length, on a second context of the same device
    assert call(tab=(C.c_void_p * 3)(vecs[0].handle.value, foreign.handle.value, vecs[2].handle.value)) == PU.MGB_E_ARG
    assert b"another context" in lib.mgb_last_error()
    short = M.HPCVector(fields[1][:-1], backend)
    assert call(tab=(C.c_void_p * 3)(vecs[0].handle.value, short.handle.value, vecs[2].handle.value)) == PU.MGB_E_ARG
    assert rows.tobytes() == first.tobytes() and hp.value is None      # nothing was written
    assert call(m=0) == 0
    loc1, _ = M._locator_of(g1)
    v1 = [M.HPCVector(np.zeros(16), g1.x.backend) for _ in range(3)]
    assert call(lc=loc1, tab=(C.c_void_p * 3)(*[v.handle.value for v in v1])) == PU.MGB_E_ARG and b"2-D or 3-D" in lib.mgb_last_error()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem2d_mpi(2, backend=be)
    n = g.x.shape[0]
    z = M.HPCMatrix(g.x.to_numpy().reshape(n, 2), be)
    seeds, ts = FU.seeds_2d(3), np.array([0.0, 0.125])
    sol = M.ParabolicSOL(g, ts, [z, z])
    assert np.isin(M.path_lines(sol, seeds).status, (0, 1)).all()      # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                          # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.path_lines(sol, seeds)
        rows, end = np.zeros((3, 5)), np.zeros((3, 2))
        ints = [np.zeros(3, dtype=np.int32) for _ in range(5)]
        assert lib.mgb_geo_path_lines(loc, 2, (C.c_void_p * 2)(z._v.handle.value, z._v.handle.value), _lib.dptr(ts), 2, 0, 3,
                                      _lib.dptr(seeds), _lib.iptr(ints[4]), 1, 4, 2.0, -1, 1.0, 1e-12, 0, _lib.dptr(rows), _lib.dptr(end),
                                      *map(_lib.iptr, ints[:4]), None) == PU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
