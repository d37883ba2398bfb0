"""estimate_steps(), adapt_time() on the device (csrc/estimate.hip; contract in include/mgb_hip.h) against the
host restatement of the same routines and against the numpy / fsum yardstick tests/estimate_steps_reference.py.

Shapes: fem1d L=2 (4 elements), fem2d L=2 (8 elements; block 7 and q = 3 divide nothing), fem2d L=4 (128 elements = 3 workgroups
of 36 + a partly idle one; 176 interior facets at 85 per workgroup: a partly idle third), fem3d L=2 k=1 (block 8, q 4), fem3d L=1
k=3 (block 64; no interior facet: no facet launch without Neumann data).  B = 1 and 3 with unequal steps.

Bars (tests/estimate_steps_reference.py): a sum or a per-element value within KTOL = 1e-12 times its magnitude, a maximum within
KTOL relative; bit for bit where the contract says so (a call repeated, a batch against its steps one by one, the fluxes
against flux(), equal snapshots against estimate())."""
import math

import numpy as np
import pytest

import boundary_reference as BR
import energy_reference as ER
import estimate_reference as XR
import estimate_steps_reference as SR

pytestmark = pytest.mark.gpu
MGB_E_ARG = -1
KTOL = SR.KTOL
GPU_SHAPES = ("fem1d_L2", "fem2d_L2", "fem2d_L4", "fem3d_L2_k1", "fem3d_L1_k3")
TS = np.array([0.0, 0.3, 0.5, 1.0])
P_VALUES = (1.0, 1.5, 2.0, "array")


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


class Mesh:
    """A device geometry of XR.SHAPES with the host handle of the same mesh, the numpy pieces of the yardstick and random data."""

    def __init__(self, M, shape):
        kind, L, k, K, nif = XR.SHAPES[shape]
        self.name, self.L = shape, L
        self.geo = M.fem1d_mpi(L) if kind == "fem1d" else (M.fem2d_mpi(L, K) if kind == "fem2d" else M.fem3d_mpi(L, k))
        self.host = XR.Mesh(shape)
        for a in ("x", "w", "n", "dim", "block", "ops", "F", "I", "nf", "q", "nif", "nel"):
            setattr(self, a, getattr(self.host, a))
        assert np.array_equal(self.geo.x.to_numpy().reshape(self.n, -1), self.x) and self.nif == nif
        rng = np.random.default_rng(1000)
        self.fields = [rng.standard_normal((self.n, 3)) for _ in range(4)]
        self.dev = [M.HPCMatrix(z) for z in self.fields]
        self.f, self.fB = rng.standard_normal(self.n), rng.standard_normal((3, self.n))
        self.h, self.hB = rng.standard_normal((self.nf, self.q)), rng.standard_normal((3, self.nf, self.q))
        self.free = rng.random(self.nf) < 0.6
        self.free[0] = True

    def par(self, M, B=3, first=0, fields=None):
        return M.ParabolicSOL(self.geo, TS[first:first + B + 1], list((self.dev if fields is None else fields)[first:first + B + 1]))


_MESHES = {}


def mesh(M, shape):
    if shape not in _MESHES:
        _MESHES[shape] = Mesh(M, shape)
    return _MESHES[shape]


def compare(name, m, lib, ind, fields, ts, pv, u=0, f=None, r=2.0, scale=1.0, h=None, free=None):
    """The device result `ind` against the host restatement and the yardstick; returns the yardstick."""
    B = len(ts) - 1
    H = SR.host_estimate_steps(lib, m.host, fields, ts, pv, f=f, u=u, r=r, scale=scale, h=h, mask=free)
    Y = SR.step_indicators(m.ops, m.w, m.F, m.I, [z[:, u] for z in fields], ts, pv, f=f, r=r, scale=scale, h=h, mask=free)
    SR.check(name + " device against numpy", Y, ind.parts, ind.columns)
    SR.check(name + " device against host", dict(Y, parts=H["parts"], totals=H["totals"]), ind.parts, ind.columns)
    assert ind.parts.shape == (B, m.nel, 4) and ind.columns.shape == (B, 2, 5) and ind.r == r
    assert ind.ts.tobytes() == np.asarray(ts).tobytes() and ind.hs.tobytes() == np.diff(ts).tobytes()
    T, G = Y["totals"], Y["totals_mag"]

    def close(got, ref, bar):
        got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
        return np.array_equal(np.isnan(got), np.isnan(ref)) and (np.abs(got - ref)[~np.isnan(ref)] <= np.broadcast_to(bar, ref.shape)[~np.isnan(ref)]).all()

    assert close(ind.volume, T[:, 0, 0], KTOL * G[:, 0, 0]) and close(ind.jump, T[:, 0, 1], KTOL * G[:, 0, 1])
    assert close(ind.neumann, T[:, 0, 2], KTOL * G[:, 0, 2]) and close(ind.time, T[:, 1, 0], KTOL * G[:, 1, 0])
    assert close(ind.space, T[:, 0, :3].sum(axis=1), 4 * KTOL * G[:, 0].sum(axis=1))
    assert close(ind.rate ** r, T[:, 1, 1], 4 * KTOL * T[:, 1, 1]) and close(ind.rate_max, T[:, 1, 4], KTOL * T[:, 1, 4])
    assert close(ind.eta_max ** r, T[:, 0, 3], 4 * KTOL * T[:, 0, 3]) and close(ind.jump_max, T[:, 0, 4], KTOL * T[:, 0, 4])
    assert close(ind.time_max, T[:, 1, 3], np.where(T[:, 1, 3] <= KTOL * Y["tim_mag_max"], KTOL * Y["tim_mag_max"], KTOL * T[:, 1, 3]))
    hs = np.diff(ts)
    space, space_mag = math.fsum(hs * T[:, 0, :3].sum(axis=1)), math.fsum(hs * G[:, 0].sum(axis=1))
    tim, tim_mag = math.fsum(hs * T[:, 1, 0]), math.fsum(hs * G[:, 1, 0])
    assert close(ind.total_space ** r, space, 8 * KTOL * space_mag) and close(ind.total_time ** r, tim, 8 * KTOL * tim_mag)
    assert close(ind.total ** r, space + tim, 8 * KTOL * (space_mag + tim_mag))
    el = np.array([math.fsum(hs * Y["parts"][:, e, :3].sum(axis=1)) for e in range(m.nel)])
    el_mag = np.array([math.fsum(hs * Y["parts_mag"][:, e, :3].sum(axis=1)) for e in range(m.nel)])
    assert ind.elements().shape == (m.nel,) and close(ind.elements(), el, 8 * KTOL * el_mag)
    group = (2 ** m.dim) ** (m.L - 1)
    assert close(ind.coarse(m.L), el.reshape(-1, group).sum(axis=1), 16 * KTOL * el_mag.reshape(-1, group).sum(axis=1))
    return Y


# (r, label, f, h, mask?, u, scale): every power once, with and without f ((n,) and (B, n)), Neumann data (1 and B rows), a mask
def variants(m, B):
    return ((1.0, "plain", None, None, False, 2, 1.0), (2.0, "f h mask", m.f, m.h, True, 0, 1.0),
            (1.5, "fB hB mask", m.fB[:B], m.hB[:B], True, 0, 0.75), (2.0, "fB h", m.fB[:B], m.h, False, 1, 1.0))


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("p", P_VALUES)
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_device_against_host_and_numpy(M, lib, shape, p, B):
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    for r, label, f, h, masked, u, scale in variants(m, B):
        free = m.free if masked else (np.ones(m.nf, dtype=bool) if h is not None else None)
        kw = {} if h is None else dict(dirichlet=~free, neumann=h)
        ind = M.estimate_steps(m.par(M, B), pv, f1=0.0 if f is None else f, u=u, r=r, scale=scale, **kw)
        compare("%s p=%s B=%d r=%g %s" % (shape, p, B, r, label), m, lib, ind, m.fields[:B + 1], TS[:B + 1], pv, u=u, f=f, r=r, scale=scale,
                h=h, free=free)


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_bitwise_properties(M, shape):
    """1: a repeated call repeats; 2: a batch is its steps one by one; 3: sigma[m] is flux(par, p, k=m)."""
    m = mesh(M, shape)
    pv = ER.exponent("array", m.x)
    kw = dict(f1=m.fB, r=1.5, scale=0.75, dirichlet=~m.free, neumann=m.hB)
    a = M.estimate_steps(m.par(M), pv, **kw)
    M.estimate_steps(m.par(M, 1), 2.0)                                     # other calls in between reuse the buffers
    M.estimate(m.geo, 2.0, z=m.dev[0])
    b = M.estimate_steps(m.par(M), pv, **kw)
    sigma = a.sigma.to_numpy().reshape(4, m.n, m.dim)
    assert a.parts.tobytes() == b.parts.tobytes() and a.columns.tobytes() == b.columns.tobytes()
    assert sigma.tobytes() == b.sigma.to_numpy().tobytes()
    for k in range(3):
        one = M.estimate_steps(m.par(M, 1, first=k), pv, f1=m.fB[k], r=1.5, scale=0.75, dirichlet=~m.free, neumann=m.hB[k])
        assert one.parts[0].tobytes() == a.parts[k].tobytes() and one.columns[0].tobytes() == a.columns[k].tobytes(), k
        assert one.sigma.to_numpy().tobytes() == sigma[k:k + 2].tobytes()
    for k in range(4):
        assert M.flux(m.par(M), pv, k=k).to_numpy().tobytes() == sigma[k].tobytes(), k


@pytest.mark.parametrize("p", (1.5, "array"))
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_equal_snapshots_give_the_stationary_indicator(M, shape, p):
    """4: where two consecutive snapshots hold the same values, row 0 and vol, jump, neu of that step are estimate() on that snapshot
    with the same scale, f, h and mask, and tim, the rate and both maxima of row 1 are exactly 0."""
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    dev = [m.dev[0], m.dev[1], M.HPCMatrix(m.fields[1].copy()), m.dev[3]]
    for r, scale in ((2.0, 1.0), (1.5, 0.75)):
        ind = M.estimate_steps(m.par(M, fields=dev), pv, f1=m.fB, r=r, scale=scale, dirichlet=~m.free, neumann=m.h)
        one = M.estimate(m.geo, pv, f=m.fB[1], z=dev[2], r=r, scale=scale, dirichlet=~m.free, neumann=m.h)
        assert ind.parts[1, :, :3].tobytes() == one.parts.tobytes() and ind.columns[1, 0].tobytes() == np.array(one.columns).tobytes()
        assert (ind.parts[1, :, 3] == 0.0).all() and (ind.columns[1, 1] == 0.0).all()
        assert ind.time[1] == 0.0 and ind.rate[1] == 0.0 and ind.rate_max[1] == 0.0 and ind.time_max[1] == 0.0
        assert (ind.parts[0, :, 3] > 0.0).all() and ind.rate_max[0] > 0.0


@pytest.mark.parametrize("shape", ("fem1d_L2", "fem2d_L4", "fem3d_L2_k1"))
def test_a_nan_reaches_its_two_steps_and_no_other(M, lib, shape):
    m = mesh(M, shape)
    e0 = m.nel // 2
    kw = dict(f1=m.f, dirichlet=~m.free, neumann=m.h)
    clean = M.estimate_steps(m.par(M), 1.5, **kw)
    fields = [z.copy() for z in m.fields]
    fields[1][e0 * m.block, 0] = np.nan
    dev = [m.dev[0], M.HPCMatrix(fields[1]), m.dev[2], m.dev[3]]
    ind = M.estimate_steps(m.par(M, fields=dev), 1.5, **kw)
    compare("%s NaN in snapshot 1" % shape, m, lib, ind, fields, TS, 1.5, f=m.f, h=m.h, free=m.free)
    near = np.zeros(m.nel, dtype=bool)
    near[m.I["elements"][(m.I["elements"] == e0).any(axis=1)].reshape(-1).astype(int)] = True
    near[e0] = True
    for k in (0, 1):
        P = ind.parts[k]
        assert np.isnan(P[e0, 0]) and np.isnan(P[e0, 3]) and not np.isnan(np.delete(P[:, [0, 3]], e0, axis=0)).any()
        assert all(np.isnan(v[k]) for v in (ind.volume, ind.time, ind.rate, ind.rate_max, ind.time_max, ind.eta_max))
    assert np.isnan(ind.parts[0, near, 1]).all() and not np.isnan(ind.parts[0, ~near, 1]).any() and not np.isnan(ind.parts[1, :, 1]).any()
    assert ind.parts[2].tobytes() == clean.parts[2].tobytes() and ind.columns[2].tobytes() == clean.columns[2].tobytes()
    assert math.isnan(ind.total) and math.isnan(ind.total_time)


def test_argument_errors(M, lib):
    from mgb_amd import _lib
    import ctypes as C
    m = mesh(M, "fem2d_L2")
    par = m.par(M)
    for kw in (dict(r=0.5), dict(r=math.inf), dict(r="2"), dict(scale=math.nan), dict(scale=None), dict(u=3), dict(f1=np.zeros(5)),
               dict(f1=np.zeros((2, m.n))), dict(dirichlet=np.zeros(3, dtype=bool)), dict(dirichlet=~m.free, neumann=m.hB[:2])):
        with pytest.raises(ValueError):
            M.estimate_steps(par, 2.0, **kw)
    for p in (0.5, math.nan):
        with pytest.raises(ValueError, match="p must"):
            M.estimate_steps(par, p)
    with pytest.raises(ValueError, match="dirichlet"):
        M.estimate_steps(par, 2.0, neumann=lambda x: 1.0)
    with pytest.raises(ValueError, match="finite"):
        M.estimate_steps(par, 2.0, dirichlet=~m.free, neumann=np.full((m.nf, m.q), np.nan))
    with pytest.raises(TypeError, match="f1"):
        M.estimate_steps(par, 2.0, f1=lambda a, b, c: 0.0)
    with pytest.raises(TypeError, match="ParabolicSOL"):
        M.estimate_steps(m.geo, 2.0)
    with pytest.raises(TypeError, match="ParabolicSOL"):
        M.estimate(par, 2.0)                                               # estimate() keeps refusing a run
    with pytest.raises(ValueError, match="two snapshots"):
        M.estimate_steps(M.ParabolicSOL(m.geo, TS[:1], m.dev[:1]), 2.0)
    with pytest.raises(ValueError, match="snapshots for"):
        M.estimate_steps(M.ParabolicSOL(m.geo, TS, m.dev[:3]), 2.0)
    with pytest.raises(ValueError, match="strictly increasing"):
        M.estimate_steps(M.ParabolicSOL(m.geo, np.array([0.0, 0.5, 0.5, 1.0]), m.dev), 2.0)
    with pytest.raises(ValueError):
        M.estimate_steps(M.ParabolicSOL(m.geo, TS, m.dev[:3] + [np.zeros((m.n + 1, 3))]), 2.0)
    # the C ABI refuses before anything is launched or written
    M.estimate_steps(par, 2.0)
    bd, be = m.geo._boundary_dev, m.geo.x.backend
    nsig, npar = 4 * m.n * m.dim, 3 * m.nel * 4
    sigma, parts = M.HPCVector(np.full(nsig, 7.0), be), M.HPCVector(np.full(npar, 7.0), be)
    short, other, out = M.HPCVector(np.full(npar - 1, 7.0), be), M.HPCVector(np.zeros(m.n), be), np.full((3, 2, 5), 7.0)
    fn3 = M.HPCVector(np.zeros(3 * m.n), be)
    wide_vecs = [M.HPCVector(np.ones(nsig), be) for _ in range(4)]         # snapshots of S = 4 dim columns: as long as sigma
    wide = [v.handle.value for v in wide_vecs]
    hands = [z._v.handle.value for z in m.dev]
    ts_bad = {"flat": [0.0, 0.3, 0.3, 1.0], "back": [0.0, 0.5, 0.3, 1.0], "nan": [0.0, 0.3, math.nan, 1.0], "inf": [0.0, 0.3, 0.5, math.inf]}

    def rc(B=3, zs=hands, ts=TS, S=3, u=0, p=2.0, pn=None, f=None, f_rows=1, r=2.0, scale=1.0, h=None, h_rows=1, sg=sigma.handle,
           pa=parts.handle, o=out, b=bd):
        table = None if zs is None else (C.c_void_p * len(zs))(*zs)
        tv = None if ts is None else _lib.f64(ts)
        return lib.mgb_estimate_steps(b, B, table, _lib.dptr(tv), S, u, p, pn, f, f_rows, r, scale, _lib.dptr(h), h_rows, None, sg, pa,
                                      None if o is None else _lib.dptr(o))

    assert rc() == 0 and rc(zs=wide, S=4 * m.dim) == 0
    sigma, parts = M.HPCVector(np.full(nsig, 7.0), be), M.HPCVector(np.full(npar, 7.0), be)
    out[:] = 7.0
    for bad in (dict(b=None), dict(zs=None), dict(ts=None), dict(sg=None), dict(pa=None), dict(o=None), dict(zs=hands[:2] + [None, hands[3]]),
                dict(B=0), dict(B=-2), dict(B=65535), dict(ts=ts_bad["flat"]), dict(ts=ts_bad["back"]), dict(ts=ts_bad["nan"]),
                dict(ts=ts_bad["inf"]), dict(S=0), dict(S=2), dict(u=3), dict(u=-1), dict(p=0.5), dict(p=math.nan), dict(r=0.99),
                dict(r=math.inf), dict(scale=math.inf), dict(scale=math.nan), dict(f=other.handle, f_rows=2), dict(f=other.handle, f_rows=0),
                dict(f=other.handle, f_rows=3), dict(f=fn3.handle, f_rows=1), dict(h=m.h, h_rows=2), dict(h=m.h, h_rows=0),
                dict(pn=short.handle), dict(pa=short.handle), dict(sg=short.handle), dict(zs=hands[:3] + [other.handle.value]),
                dict(zs=wide[:3] + [sigma.handle.value], S=4 * m.dim), dict(zs=[sigma.handle.value] + wide[1:], S=4 * m.dim)):
        kw = dict(sg=sigma.handle, pa=parts.handle)                        # the last two: an output that is also an input, every length right
        kw.update(bad)
        assert rc(**kw) == MGB_E_ARG, bad
    assert (sigma.to_numpy() == 7.0).all() and (parts.to_numpy() == 7.0).all() and (out == 7.0).all()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    import ctypes as C
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    n = g.x.shape[0]
    zs = [M.HPCMatrix(np.full((n, 2), float(k)), be) for k in range(2)]
    par = M.ParabolicSOL(g, np.array([0.0, 0.5]), zs)
    ind = M.estimate_steps(par, 2.0, f1=0.0)                               # fine while the context is one rank
    assert ind.jump[0] == 0.0 and ind.time[0] == 0.0 and ind.rate_max[0] == 2.0
    sigma, parts, out = M.HPCVector(np.full(2 * n, 7.0), be), M.HPCVector(np.full(4 * (n // 2), 7.0), be), np.full((1, 2, 5), 7.0)
    table, ts = (C.c_void_p * 2)(*[z._v.handle.value for z in zs]), np.array([0.0, 0.5])
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.estimate_steps(par, 2.0)
        assert lib.mgb_estimate_steps(g._boundary_dev, 1, table, _lib.dptr(ts), 2, 0, 2.0, None, None, 1, 2.0, 1.0, None, 1, None, sigma.handle,
                                      parts.handle, _lib.dptr(out)) == MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
    assert (sigma.to_numpy() == 7.0).all() and (parts.to_numpy() == 7.0).all() and (out == 7.0).all()


def run_yardstick(M, par, p, f=0.5):
    g = par.geometry
    F = BR.facets(g)
    I = XR.interior_facets(g, F)
    w = g.w.to_numpy() if hasattr(g.w, "to_numpy") else np.asarray(g.w)
    fields = [np.asarray(M._to_cpu_array(z))[:, 0] for z in par.u]
    return SR.step_indicators(ER.operators(g), w, F, I, fields, par.ts, p, f=np.full(len(w), f))


@pytest.mark.parametrize("kind,L", [("fem1d", 3), ("fem2d", 2)])
def test_solved_runs(M, kind, L):
    """estimate_steps(parabolic_solve(...)) against the yardstick on the same snapshots, and the decrease of total_time when every
    step is halved.  On the CPU oracle's runs the yardstick gives sum h_k time_k = 6.49e-3, 2.07e-3 (fem1d L = 3) at h = 0.5, 0.25."""
    geo = M.fem1d_mpi(L) if kind == "fem1d" else M.fem2d_mpi(L)
    totals = []
    for ts in ([0.0, 0.5, 1.0], [0.0, 0.25, 0.5, 0.75, 1.0]):
        par = M.parabolic_solve(geo, p=2.0, ts=ts)
        ind = M.estimate_steps(par, 2.0)
        Y = run_yardstick(M, par, 2.0)
        SR.check("%s L=%d %d steps" % (kind, L, len(ts) - 1), Y, ind.parts, ind.columns)
        print("%s L=%d %d steps: total_time^2 %.6e total_space^2 %.6e, h_k time_k %s" % (kind, L, len(ts) - 1, ind.total_time ** 2,
                                                                                          ind.total_space ** 2, ind.hs * ind.time))
        totals.append(ind.total_time)
    assert 0.0 < totals[1] < totals[0]
    assert M.mark(ind.hs * ind.time, 0.5).tolist() == [0]


def test_adapt_time(M):
    rounds = M.adapt_time(M.fem1d_mpi(3), [0.0, 0.25, 0.5, 0.75, 1.0], 2.0, 2)
    assert len(rounds) == 3
    assert rounds[1][0].tolist() == [0.0, 0.125, 0.25, 0.5, 0.75, 1.0]
    for k, (ts, par, ind) in enumerate(rounds):
        assert par.ts.tobytes() == ts.tobytes() and len(par.u) == len(ts) and ind.parts.shape[0] == len(ts) - 1
        print("adapt_time round %d: %d steps, total_time %.6e, total %.6e" % (k, len(ts) - 1, ind.total_time, ind.total))
        if k + 1 < len(rounds):
            assert rounds[k + 1][0].tobytes() == M.refine_times(ts, M.mark(ind.hs * ind.time, 0.5)).tobytes()
    assert rounds[2][2].total_time < rounds[1][2].total_time < rounds[0][2].total_time
