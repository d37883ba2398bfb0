"""time_stats() on the device (csrc/timestat.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-node routines and against the exact yardstick tests/timestat_reference.py.

Fields are synthetic -- random values and the moving front tanh((t - |x|) / 0.2) -- handed over as a hand-made ParabolicSOL.
Shapes, the smallest at which the kernel can go wrong:
  fem1d L=3, B=2, one level                      16 nodes, one interval
  fem2d L=2, S=2, u=1, B=5, 3 levels             56 nodes, under one workgroup, column stride
  fem2d L=4, B=9, non-uniform ts, 9 levels       896 nodes = 3.5 workgroups; the last level chunk holds one level
  fem2d L=8, B=3, 2 levels                       229 376 nodes = 896 workgroups: the finish folds runs of 4 partials; device
                                                 against the host restatement only
  fem3d L=1                                      nothing depends on the dimension
  the NaN / inf batch                            non-finite values

Device against host restatement: both tables and the maxima of every row BIT FOR BIT (both sides run the same IEEE operations
with contraction off); the three sums within (24 + ceil(nwg / 256)) eps sum |terms|, the depth of the two-stage fold of
reduce.hpp.  Device against the yardstick, up to L=4: the bars of tests/timestat_util.py.
Largest ratios to the bars seen on an MI355X (every run prints them): change 0.50, integral 0.18, variation 0.21, rate 0.22,
arrival 0.14, left 0.09, exposure 0.09, excess 0.07, totals 0.09; sums against the host restatement 0.04; `total` of the
parabolic run against the trapezoid sum of its masses 0.00.

Argument errors: every MGB_E_ARG condition of the contract is provoked on the device entry point except one, `node` and
`level` being the same vector: a vector cannot hold n x 8 and nl x n x 5 values at once, so the length check refuses it first."""
import ctypes as C
import math

import numpy as np
import pytest

import timestat_reference as TR
import timestat_util as TU

pytestmark = pytest.mark.gpu
NAN = float("nan")
NULL_FIELD = object()


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_GEO = {}


def mesh(M, kind, L):
    """(device geometry, host mesh) of the same nodes."""
    if (kind, L) not in _GEO:
        geo = M.fem3d_mpi(L, 1) if kind == "fem3d" else getattr(M, kind + "_mpi")(L)
        host = TU.host_mesh(kind, L)
        assert np.array_equal(geo.x.to_numpy().reshape(host.n, -1), host.x)
        _GEO[(kind, L)] = (geo, host)
    return _GEO[(kind, L)]


def fields_of(Z, S=1, u=0, seed=0):
    """the (B, n) values as B fields of S columns with the values in column u and noise elsewhere"""
    rng = np.random.default_rng(seed)
    out = []
    for row in Z:
        z = rng.standard_normal((len(row), S))
        z[:, u] = row
        out.append(z)
    return out


def run_of(M, geo, fields, ts):
    return M.ParabolicSOL(geo, np.asarray(ts, dtype=np.float64), [M.HPCMatrix(z) for z in fields])


def device_result(st, n):
    nl = 0 if st.level is None else st.level.shape[0] // n
    assert st.node.shape == (n, 8) and (st.level is None or st.level.shape == (nl * n, 5)) and st.rows.shape == (1 + nl, 5)
    level = np.zeros((0, n, 5)) if st.level is None else st.level.to_numpy().reshape(nl, n, 5)
    return TU.Result(st.node.to_numpy(), level, st.rows)


def same_as_host(name, dev, host, w):
    """tables and maxima bit for bit, the three sums within the depth of the two-stage fold"""
    assert dev.node.tobytes() == host.node.tobytes(), name
    assert dev.level.tobytes() == host.level.tobytes(), name
    assert dev.rows[:, 3:].tobytes() == host.rows[:, 3:].tobytes(), name
    n = len(w)
    depth = 24 + math.ceil(math.ceil(n / 256) / 256)
    worst = 0.0
    for r in range(dev.rows.shape[0]):
        if r == 0:
            terms = [w * host.node[:, 0], w * host.node[:, 5], w * host.node[:, 7]]
        else:
            L = host.level[r - 1]
            terms = [np.where(np.isnan(L[:, 4]), np.nan, w * (L[:, 4] > 0)), w * L[:, 2], w * L[:, 3]]
        for k in range(3):
            if np.isnan(terms[k]).any():
                assert np.isnan(dev.rows[r, k]) and np.isnan(host.rows[r, k]), (name, r, k)
                continue
            gap, bar = abs(dev.rows[r, k] - host.rows[r, k]), depth * TR.EPS * math.fsum(np.abs(terms[k]))
            if bar > 0:
                worst = max(worst, gap / bar)
            assert gap <= bar, (name, r, k, gap, bar)
    print("%s: tables and maxima equal the host restatement; sums, largest ratio to the bar %.3e" % (name, worst))


CASES = {
    "fem1d L=3 B=2": ("fem1d", 3, 1, 0, np.array([0.25, 0.75]), [0.1]),
    "fem2d L=2 S=2 u=1 B=5": ("fem2d", 2, 2, 1, np.array([-1.5, -0.75, -0.125, 0.5, 2.0]), [-0.5, 0.0, 0.6]),
    "fem2d L=4 B=9 nl=9": ("fem2d", 4, 1, 0, np.cumsum(np.random.default_rng(5).uniform(0.05, 0.4, 9)) - 0.6, None),
    "fem3d L=1 B=4": ("fem3d", 1, 1, 0, np.array([0.0, 0.5, 1.25, 1.5]), [0.0, 0.4]),
}
_CASE = {}


def case(M, lib, name):
    """geometry, host mesh, values, fields, levels, the host result and the yardstick of a case: computed once and shared"""
    if name not in _CASE:
        kind, L, S, u, ts, levels = CASES[name]
        geo, h = mesh(M, kind, L)
        rng = np.random.default_rng(len(name))
        Z = np.where(rng.random((len(ts), h.n)) < 0.6, TU.front(h.x, ts - ts[0]), rng.standard_normal((len(ts), h.n)))
        if levels is None:      # one above and one below every value, some equal to snapshot values
            Z = np.round(Z, 2)
            levels = [Z.max() + 1.0, Z.min() - 1.0, 0.25, -0.25, 0.0, 0.5, Z[3, 11], Z[0, 0], Z[8, 895]]
        fields = fields_of(Z, S, u)
        host = TU.host_time_stats(lib, h, fields, ts, levels, never=7.5, u=u)
        _CASE[name] = (geo, h, Z, fields, ts, levels, u, host, TR.Reference(Z, ts, levels, h.w))
    return _CASE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_device_against_host_and_reference(M, lib, name):
    geo, h, Z, fields, ts, levels, u, host, R = case(M, lib, name)
    par = run_of(M, geo, fields, ts)
    st = M.time_stats(par, levels, u=u, never=7.5)
    dev = device_result(st, h.n)
    same_as_host(name, dev, host, h.w)
    TU.against_reference(name + " device", dev, R, 7.5)
    again = device_result(M.time_stats(par, levels, u=u, never=7.5), h.n)
    assert again.node.tobytes() == dev.node.tobytes() and again.level.tobytes() == dev.level.tobytes()
    assert again.rows.tobytes() == dev.rows.tobytes()
    # the attributes of the Python result
    nl = len(levels)
    assert np.array_equal(st.ts, ts) and np.array_equal(st.levels, levels)
    for k, key in enumerate(TR.NODE_NAMES):
        assert getattr(st, key).tobytes() == dev.node[:, k].tobytes(), key
    assert st.mean.tobytes() == (dev.node[:, 0] / (ts[-1] - ts[0])).tobytes()
    for k, key in enumerate(TR.LEVEL_NAMES[:4]):
        assert getattr(st, key).shape == (h.n, nl) and getattr(st, key).tobytes() == dev.level[:, :, k].T.tobytes(), key
    assert st.entries.dtype == np.int64 and np.array_equal(st.entries, dev.level[:, :, 4].T) and np.array_equal(st.reached, st.entries > 0)
    assert (st.total, st.total_variation, st.total_change, st.peak, st.trough) == tuple(dev.rows[0, :4]) + (-dev.rows[0, 4],)
    for k, key in enumerate(("reached_measure", "exposure_total", "excess_total", "last_arrival", "longest_exposure")):
        assert getattr(st, key).tobytes() == dev.rows[1:, k].tobytes(), key
    assert st.peak == Z.max() and st.trough == Z.min()


def test_levels_chunks_windows_and_tables(M, lib):
    """On the 9-level case: bitwise, a one-level call equals that level's slice and row of the 9-level call; start=2, stop=5
    equals a run built from those four snapshots; no levels gives the node table alone; st.node and st.level are usable as z=
    of level_sets without a host copy."""
    geo, h, Z, fields, ts, levels, u, host, R = case(M, lib, "fem2d L=4 B=9 nl=9")
    par = run_of(M, geo, fields, ts)
    for l, c in enumerate(levels):
        one = M.time_stats(par, float(c), never=7.5)
        d = device_result(one, h.n)
        assert d.node.tobytes() == host.node.tobytes()
        assert d.level[0].tobytes() == host.level[l].tobytes() and d.rows[1, 3:].tobytes() == host.rows[1 + l, 3:].tobytes(), l
        assert one.arrival.shape == (h.n,) and isinstance(one.reached_measure, float) and one.levels == c
        assert one.arrival.tobytes() == host.level[l, :, 0].tobytes() and np.array_equal(one.entries, host.level[l, :, 4])
    nine = device_result(M.time_stats(par, levels, never=7.5), h.n)
    for l, c in enumerate(levels):      # the sums too: the same workgroups fold the same terms in the same order
        assert device_result(M.time_stats(par, float(c), never=7.5), h.n).rows[1].tobytes() == nine.rows[1 + l].tobytes(), l
    none = M.time_stats(par)
    assert none.level is None and none.levels is None and none.rows.tobytes() == nine.rows[:1].tobytes()
    assert none.node.to_numpy().tobytes() == nine.node.tobytes()
    with pytest.raises(ValueError):
        none.arrival
    with pytest.raises(ValueError):
        none.reached_measure
    win = device_result(M.time_stats(par, levels, start=2, stop=5, never=7.5), h.n)
    built = device_result(M.time_stats(run_of(M, geo, fields[2:6], ts[2:6]), levels, never=7.5), h.n)
    assert win.node.tobytes() == built.node.tobytes() and win.level.tobytes() == built.level.tobytes() and win.rows.tobytes() == built.rows.tobytes()
    TU.against_reference("window 2..5 device", win, TR.Reference(Z[2:6], ts[2:6], levels, h.w), 7.5)
    neg = device_result(M.time_stats(par, levels, start=-7, stop=-4, never=7.5), h.n)
    assert neg.node.tobytes() == win.node.tobytes() and neg.rows.tobytes() == win.rows.tobytes()
    # the tables as fields of level_sets: the HPCMatrix is taken as it is
    st = M.time_stats(par, 0.25, never=float(ts[-1]) + 1.0)
    iso = M.level_sets(geo, [0.0, 0.5], z=st.level, u=0)
    assert iso.rows.tobytes() == M.level_sets(geo, [0.0, 0.5], z=st.arrival).rows.tobytes()
    dose = M.level_sets(geo, 0.1, z=st.node, u=0)
    assert dose.rows.tobytes() == M.level_sets(geo, 0.1, z=st.integral).rows.tobytes()
    assert M._nodal_values(geo, st.node, st.node.backend, "test")[0] is st.node._v


def test_many_workgroups_against_the_host_restatement(M, lib):
    geo, h = mesh(M, "fem2d", 8)
    assert h.n == 229376
    ts = np.array([0.0, 0.3, 1.0])
    rng = np.random.default_rng(8)
    Z = TU.front(h.x, ts) + 0.05 * rng.standard_normal((3, h.n))
    fields, levels = fields_of(Z), [0.0, 0.7]
    host = TU.host_time_stats(lib, h, fields, ts, levels)
    dev = device_result(M.time_stats(run_of(M, geo, fields, ts), levels), h.n)
    same_as_host("fem2d L=8 B=3", dev, host, h.w)
    assert 0.0 < dev.rows[1, 0] < 4.0 and dev.rows[1, 0] > dev.rows[2, 0] > 0.0


@pytest.mark.parametrize("never", [NAN, 7.5, np.inf])
def test_non_finite_values(M, lib, never):
    """A NaN, an inf and a -inf at three nodes, in different snapshots and workgroups: those nodes' columns are all NaN, every sum
    and maximum is NaN, every other node is untouched."""
    geo, h = mesh(M, "fem2d", 4)
    ts = np.array([0.0, 0.5, 1.5, 2.0, 2.25])
    Z = np.random.default_rng(12).standard_normal((5, h.n))
    levels = [0.1, -0.3, 9.0]
    clean = device_result(M.time_stats(run_of(M, geo, fields_of(Z), ts), levels, never=never), h.n)
    assert np.isfinite(clean.rows[:, :3]).all()
    Zb = Z.copy()
    Zb[0, 5], Zb[2, 300], Zb[4, 895] = np.nan, np.inf, -np.inf
    fields = fields_of(Zb)
    dev = device_result(M.time_stats(run_of(M, geo, fields, ts), levels, never=never), h.n)
    host = TU.host_time_stats(lib, h, fields, ts, levels, never=never)
    same_as_host("non-finite batch", dev, host, h.w)
    TU.against_reference("non-finite batch device", dev, TR.Reference(Zb, ts, levels, h.w), never)
    bad = np.zeros(h.n, dtype=bool)
    bad[[5, 300, 895]] = True
    assert np.isnan(dev.node[bad]).all() and np.isnan(dev.level[:, bad]).all() and np.isnan(dev.rows).all()
    assert dev.node[~bad].tobytes() == clean.node[~bad].tobytes() and dev.level[:, ~bad].tobytes() == clean.level[:, ~bad].tobytes()
    top = clean.level[2]
    assert TU._same_never(top[:, 0], never).all() and TU._same_never(top[:, 1], never).all() and (top[:, 2:] == 0.0).all()
    assert clean.rows[3].tolist() == [0.0, 0.0, 0.0, -np.inf, 0.0]


def test_a_real_run(M, lib):
    """parabolic_solve on fem2d L=3: time_stats equals the host restatement on its snapshots, and `total` is the trapezoid sum of
    the masses sum_i w_i u_i(t_m), within the integral bar (B + 2) eps sum |terms| (the numpy side is summed exactly, fsum)."""
    par = M.parabolic_solve(M.fem2d_mpi(3), h=0.25, p=2.0)
    h = TU.host_mesh("fem2d", 3)
    B = len(par.u)
    assert B == 5
    snaps = [zk.to_numpy() for zk in par.u]
    st = M.time_stats(par, [0.1, 0.3])
    dev = device_result(st, h.n)
    host = TU.host_time_stats(lib, h, snaps, par.ts, [0.1, 0.3])
    same_as_host("parabolic run", dev, host, h.w)
    U = np.stack([z[:, 0] for z in snaps])
    ts = np.asarray(par.ts, dtype=np.float64)
    mass = [math.fsum(h.w * U[m]) for m in range(B)]
    trapezoid = math.fsum(0.5 * (ts[m + 1] - ts[m]) * (mass[m] + mass[m + 1]) for m in range(B - 1))
    terms = math.fsum(math.fsum(0.5 * (ts[m + 1] - ts[m]) * h.w * (np.abs(U[m]) + np.abs(U[m + 1]))) for m in range(B - 1))
    bar = (B + 2) * TR.EPS * terms
    print("parabolic run: total %.17g, trapezoid of the masses %.17g, gap / bar %.3f; reached measure %s, last arrival %s"
          % (st.total, trapezoid, abs(st.total - trapezoid) / bar, st.reached_measure, st.last_arrival))
    assert abs(st.total - trapezoid) <= bar
    assert st.arrival.shape == (h.n, 2) and (st.reached_measure[0] >= st.reached_measure[1]).all()
    tail = M.time_stats(par, start=-2)
    assert np.array_equal(tail.ts, ts[-2:]) and tail.change.tobytes() == (U[-1] - U[-2]).tobytes()


def test_argument_errors(M):
    geo, h = mesh(M, "fem2d", 2)
    ts = np.array([0.0, 1.0, 2.0])
    Z = np.random.default_rng(1).standard_normal((3, h.n))
    par = run_of(M, geo, fields_of(Z), ts)
    assert M.time_stats(par, 0.1).entries.shape == (h.n,)
    for kw, err in ((dict(start=1.0), TypeError), (dict(stop="2"), TypeError), (dict(u=0.0), TypeError), (dict(never="x"), TypeError),
                    (dict(never=None), TypeError), (dict(levels="abc"), TypeError), (dict(start=2), ValueError), (dict(start=3), ValueError),
                    (dict(stop=0), ValueError), (dict(start=1, stop=-3), ValueError), (dict(stop=-4), ValueError), (dict(u=1), ValueError),
                    (dict(levels=np.nan), ValueError), (dict(levels=[[0.1]]), ValueError), (dict(levels=[]), ValueError),
                    (dict(levels=np.zeros(4097)), ValueError)):
        with pytest.raises(err):
            M.time_stats(par, **kw)
    with pytest.raises(TypeError):
        M.time_stats(geo, 0.1)
    for bad_ts in ([0.0, 1.0, 1.0], [0.0, np.nan, 2.0], [0.0, 2.0, 1.0]):
        with pytest.raises(ValueError):
            M.time_stats(run_of(M, geo, fields_of(Z), bad_ts))
    assert M.time_stats(run_of(M, geo, fields_of(Z), [0.0, 1.0, 1.0]), stop=1).ts.tolist() == [0.0, 1.0]      # the window alone counts
    with pytest.raises(ValueError):
        M.time_stats(M.ParabolicSOL(geo, ts, [M.HPCMatrix(Z[0][:, None]), M.HPCMatrix(fields_of(Z, 2)[1]), M.HPCMatrix(Z[2][:, None])]))
    # the C entry point: MGB_E_ARG before anything is launched or written
    from mgb_amd import _lib
    lib = _lib.load()
    loc, backend = M._locator_of(geo)
    n = h.n
    vec = lambda a, be=backend: M.HPCVector(np.ascontiguousarray(a, dtype=np.float64).reshape(-1), be)
    z = [vec(Z[m]) for m in range(3)]
    node, level, short = vec(np.full(n * 8, 7.0)), vec(np.full(n * 5, 7.0)), vec(np.full(n * 5 - 1, 7.0))
    other = M.HPCBackend(0)      # a second context of the same device
    rows, lv = np.full((2, 5), 7.0), np.array([0.1])

    def rc(loc=loc, B=3, fields=z, tsp=_lib.dptr(ts), S=1, u=0, nl=1, lvp=_lib.dptr(lv), node=node, level=level, out=_lib.dptr(rows)):
        table = None if fields is None else (C.c_void_p * len(fields))(*[None if f is NULL_FIELD else f.handle.value for f in fields])
        return lib.mgb_geo_time_stats(loc, B, table, tsp, S, u, nl, lvp, 7.5, None if node is None else node.handle,
                                      None if level is None else level.handle, out)

    assert rc() == 0 and not (rows == 7.0).any()
    assert rc(nl=0, lvp=None, level=None) == 0
    rows[:] = 7.0
    node, level = vec(np.full(n * 8, 7.0)), vec(np.full(n * 5, 7.0))
    bad_ts = [np.array(t) for t in ([0.0, np.nan, 2.0], [0.0, np.inf, 2.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0])]
    z8 = [vec(np.zeros(n * 8)) for _ in range(3)]
    z5 = [vec(np.zeros(n * 5)) for _ in range(3)]
    for kw in (dict(loc=None), dict(fields=None), dict(tsp=None), dict(node=None), dict(out=None), dict(lvp=None), dict(level=None),
               dict(fields=[z[0], NULL_FIELD, z[2]]), dict(B=1, fields=z[:1]), dict(B=0), dict(nl=-1), dict(nl=4097), dict(S=0),
               dict(u=1), dict(u=-1), dict(lvp=_lib.dptr(np.array([np.inf]))), dict(lvp=_lib.dptr(np.array([np.nan]))),
               dict(tsp=_lib.dptr(bad_ts[0])), dict(tsp=_lib.dptr(bad_ts[1])), dict(tsp=_lib.dptr(bad_ts[2])), dict(tsp=_lib.dptr(bad_ts[3])),
               dict(fields=[z[0], short, z[2]]), dict(S=2), dict(node=short), dict(level=short), dict(node=level),
               dict(fields=[z[0], vec(Z[1], other), z[2]]), dict(node=vec(np.zeros(n * 8), other)), dict(level=vec(np.zeros(n * 5), other)),
               dict(fields=[z8[0], node, z8[2]], S=8), dict(fields=[z5[0], z5[1], level], S=5)):
        assert rc(**{**dict(node=node, level=level), **kw}) == TU.MGB_E_ARG, kw
    assert rc(fields=[z8[0], node, z8[2]], S=8, node=node, level=level) == TU.MGB_E_ARG and b"also an input" in lib.mgb_last_error()
    assert (rows == 7.0).all() and (node.to_numpy() == 7.0).all() and (level.to_numpy() == 7.0).all()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    n = g.x.shape[0]
    ts = np.array([0.0, 1.0])
    par = M.ParabolicSOL(g, ts, [M.HPCMatrix(np.zeros((n, 1)), be), M.HPCMatrix(np.ones((n, 1)), be)])
    assert abs(M.time_stats(par, 0.5).total - 1.0) <= 1e-14              # fine while the context is one rank
    loc, _ = M._locator_of(g)
    node, rows = M.HPCVector(n * 8, be), np.zeros((1, 5))
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.time_stats(par, 0.5)
        table = (C.c_void_p * 2)(par.u[0]._v.handle.value, par.u[1]._v.handle.value)
        assert lib.mgb_geo_time_stats(loc, 2, table, _lib.dptr(ts), 1, 0, 0, None, 0.0, node.handle, None, _lib.dptr(rows)) == TU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
