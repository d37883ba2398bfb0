"""The host restatement of the error indicators of parabolic steps (mgb_geo_estimate_steps_host, csrc/estimate.hpp), refine_times()
and the Python layer as far as it goes without a device, on the CPU against the yardstick tests/estimate_steps_reference.py
(DESIGN.md section 4m).  Bars: KTOL = 1e-12 times the magnitude for a sum or a per-element value, KTOL relative for a maximum;
the bitwise properties bit for bit."""
import math

import numpy as np
import pytest

import energy_reference as ER
import estimate_reference as XR
import estimate_steps_reference as SR

MGB_E_ARG = -1
KTOL = SR.KTOL
SHAPES = ("fem1d_L2", "fem2d_L2", "fem3d_L1_k3")
TS = np.array([0.0, 0.3, 0.5, 1.0])
P_VALUES = (1.0, 1.5, 2.0, "array")
_MESHES = {}


def mesh(shape):
    if shape not in _MESHES:
        _MESHES[shape] = XR.Mesh(shape)
    return _MESHES[shape]


@pytest.fixture(scope="module")
def M():
    import mgb_amd
    return mgb_amd


def data(g, seed, B=3):
    rng = np.random.default_rng(seed)
    fields = [rng.standard_normal((g.n, 3)) for _ in range(B + 1)]
    return dict(fields=fields, f=rng.standard_normal(g.n), fB=rng.standard_normal((B, g.n)), h=rng.standard_normal((g.nf, g.q)),
                hB=rng.standard_normal((B, g.nf, g.q)), free=rng.random(g.nf) < 0.6)


def variants(D):
    """(label, f, h, mask, u, scale): with and without f ((n,) and (B, n)), with and without Neumann data (1 and B rows) and a mask."""
    return (("plain", None, None, None, 2, 1.0), ("f h mask", D["f"], D["h"], D["free"], 0, 1.0),
            ("fB hB mask", D["fB"], D["hB"], D["free"], 0, 0.75), ("fB h", D["fB"], D["h"], None, 1, 1.0))


@pytest.mark.parametrize("p", P_VALUES)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_steps_against_the_yardstick(lib, shape, p):
    g = mesh(shape)
    pv = ER.exponent(p, g.x)
    D = data(g, 800)
    for r in XR.R_VALUES:
        for label, f, h, mask, u, scale in variants(D):
            name = "%s p=%s r=%g %s" % (shape, p, r, label)
            R = SR.host_estimate_steps(lib, g, D["fields"], TS, pv, f=f, u=u, r=r, scale=scale, h=h, mask=mask)
            Y = SR.step_indicators(g.ops, g.w, g.F, g.I, [z[:, u] for z in D["fields"]], TS, pv, f=f, r=r, scale=scale, h=h, mask=mask)
            SR.check(name, Y, R["parts"], R["totals"], R["J"], R["N"])
            assert (R["totals"][:, 1, 2] == 0.0).all()
            flux = ER.host_energy(lib, g, D["fields"], pv, u=u, s=(u + 1) % 3)[1]
            assert R["sigma"].tobytes() == np.ascontiguousarray(flux).tobytes()      # Sigma^m is the flux of the energy module, bit for bit


@pytest.mark.parametrize("shape", SHAPES)
def test_a_batch_is_its_steps_one_by_one(lib, shape):
    """Property 2: B steps return the bits of B calls with B = 1."""
    g = mesh(shape)
    D = data(g, 810)
    pv = ER.exponent("array", g.x)
    R = SR.host_estimate_steps(lib, g, D["fields"], TS, pv, f=D["fB"], r=1.5, h=D["hB"], mask=D["free"])
    again = SR.host_estimate_steps(lib, g, D["fields"], TS, pv, f=D["fB"], r=1.5, h=D["hB"], mask=D["free"])
    assert all(R[k].tobytes() == again[k].tobytes() for k in R)
    for k in range(3):
        one = SR.host_estimate_steps(lib, g, D["fields"][k:k + 2], TS[k:k + 2], pv, f=D["fB"][k], r=1.5, h=D["hB"][k], mask=D["free"])
        for key in ("parts", "J", "N", "totals"):
            assert one[key][0].tobytes() == R[key][k].tobytes(), (k, key)
        assert one["sigma"].tobytes() == R["sigma"][k:k + 2].tobytes()


@pytest.mark.parametrize("p", (1.5, 2.0, "array"))
@pytest.mark.parametrize("shape", SHAPES)
def test_equal_snapshots_give_the_stationary_indicator(lib, shape, p):
    """Property 4: where two consecutive snapshots hold the same values, row 0 and vol, jump, neu are mgb_geo_estimate_host on that
    snapshot with own_scale, and the time part, the rate and both maxima of row 1 are exactly 0."""
    g = mesh(shape)
    pv = ER.exponent(p, g.x)
    D = data(g, 820)
    fields = [D["fields"][0], D["fields"][1], D["fields"][1].copy(), D["fields"][3]]
    for r, scale in ((2.0, 1.0), (1.5, 0.75)):
        R = SR.host_estimate_steps(lib, g, fields, TS, pv, f=D["fB"], r=r, scale=scale, h=D["h"], mask=D["free"])
        E = XR.host_estimate(lib, g, fields[2], pv, f=D["fB"][1], r=r, scale=scale, h=D["h"], mask=D["free"])
        assert R["parts"][1, :, :3].tobytes() == E["parts"].tobytes() and R["totals"][1, 0].tobytes() == E["totals"].tobytes()
        assert R["J"][1].tobytes() == E["J"].tobytes() and R["N"][1].tobytes() == E["N"].tobytes()
        assert (R["parts"][1, :, 3] == 0.0).all() and (R["totals"][1, 1] == 0.0).all()
        assert (R["parts"][0, :, 3] > 0.0).all() and R["totals"][0, 1, 4] > 0.0


@pytest.mark.parametrize("shape", ("fem1d_L2", "fem2d_L2"))
def test_a_nan_reaches_its_two_steps_and_no_other(lib, shape):
    """A NaN at one node of snapshot 1 of 4: steps 1 and 2 are NaN in its element, the jumps in its facet neighbours, and step 3
    carries the bits of the clean run."""
    g = mesh(shape)
    D = data(g, 830)
    e0 = g.nel // 2
    clean = SR.host_estimate_steps(lib, g, D["fields"], TS, 1.5, f=D["f"], h=D["h"], mask=D["free"])
    fields = [z.copy() for z in D["fields"]]
    fields[1][e0 * g.block, 0] = np.nan
    R = SR.host_estimate_steps(lib, g, fields, TS, 1.5, f=D["f"], h=D["h"], mask=D["free"])
    Y = SR.step_indicators(g.ops, g.w, g.F, g.I, [z[:, 0] for z in fields], TS, 1.5, f=D["f"], h=D["h"], mask=D["free"])
    SR.check("%s NaN in snapshot 1" % shape, Y, R["parts"], R["totals"], R["J"], R["N"])
    near = np.zeros(g.nel, dtype=bool)
    near[g.I["elements"][(g.I["elements"] == e0).any(axis=1)].reshape(-1).astype(int)] = True
    near[e0] = False
    for k in (0, 1):                                                       # steps 1 and 2
        P = R["parts"][k]
        assert np.isnan(P[e0, 0]) and np.isnan(P[e0, 3]) and not np.isnan(np.delete(P[:, [0, 3]], e0, axis=0)).any()
        assert np.isnan(R["totals"][k, 1, [0, 1, 3, 4]]).all() and np.isnan(R["totals"][k, 0, [0, 3]]).all()
    assert np.isnan(R["parts"][0, near, 1]).all() and np.isnan(R["parts"][0, e0, 1])      # step 1: Sigma^1 is the jumping flux
    assert not np.isnan(R["parts"][1, :, 1]).any()                                       # step 2 jumps over Sigma^2, which is clean
    assert all(R[key][2].tobytes() == clean[key][2].tobytes() for key in ("parts", "J", "N", "totals"))
    assert R["sigma"][[0, 2, 3]].tobytes() == clean["sigma"][[0, 2, 3]].tobytes()


def test_refused_inputs(lib, M):
    from mgb_amd import _lib
    g = mesh("fem2d_L2")
    D = data(g, 840)
    z = D["fields"]
    for bad in (dict(S=0), dict(u=3), dict(u=-1), dict(p=0.5), dict(p=math.nan), dict(p=np.where(np.arange(g.n) == 4, 0.5, 2.0)), dict(r=0.99),
                dict(r=math.nan), dict(r=math.inf), dict(scale=math.inf), dict(scale=math.nan), dict(B=0), dict(B=-1), dict(B=65535),
                dict(ts=[0.0, 0.3, 0.3, 1.0]), dict(ts=[0.0, 0.5, 0.3, 1.0]), dict(ts=[0.0, 0.3, math.nan, 1.0]), dict(ts=[0.0, 0.3, 0.5, math.inf]),
                dict(f=D["f"], f_rows=2), dict(f=D["f"], f_rows=0), dict(h=D["h"], h_rows=2), dict(h=D["h"], h_rows=-1)):
        kw = dict(p=2.0, ts=TS)
        kw.update(bad)
        rc, parts, out = SR.host_estimate_steps(lib, g, z, kw.pop("ts"), kw.pop("p"), rc_only=True, **kw)
        assert rc == MGB_E_ARG and (parts == 7.0).all() and (out == 7.0).all(), bad
    zs = [_lib.f64(v) for v in z]
    table = (_lib.c_dbl_p * 4)(*[_lib.dptr(v) for v in zs])
    holed = (_lib.c_dbl_p * 4)(_lib.dptr(zs[0]), None, _lib.dptr(zs[2]), _lib.dptr(zs[3]))
    parts, out = np.full((3, g.nel, 4), 7.0), np.full((3, 2, 5), 7.0)
    a = (3, 0, 2.0, None, None, 1, 2.0, 1.0, None, 1, None, None)
    fn = lib.mgb_geo_estimate_steps_host
    assert fn(None, 3, table, _lib.dptr(TS), *a, _lib.dptr(parts), None, None, _lib.dptr(out)) == MGB_E_ARG
    assert fn(g.handle, 3, None, _lib.dptr(TS), *a, _lib.dptr(parts), None, None, _lib.dptr(out)) == MGB_E_ARG
    assert fn(g.handle, 3, holed, _lib.dptr(TS), *a, _lib.dptr(parts), None, None, _lib.dptr(out)) == MGB_E_ARG
    assert fn(g.handle, 3, table, None, *a, _lib.dptr(parts), None, None, _lib.dptr(out)) == MGB_E_ARG
    assert fn(g.handle, 3, table, _lib.dptr(TS), *a, None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert fn(g.handle, 3, table, _lib.dptr(TS), *a, _lib.dptr(parts), None, None, None) == MGB_E_ARG
    assert (parts == 7.0).all() and (out == 7.0).all()
    assert fn(g.handle, 3, table, _lib.dptr(TS), *a, _lib.dptr(parts), None, None, _lib.dptr(out)) == 0      # and the good call goes through
    # the Python layer, as far as it goes without a device
    par = M.ParabolicSOL(g.py, TS, z)
    with pytest.raises(TypeError, match="ParabolicSOL"):
        M.estimate_steps(g.py, 2.0)
    with pytest.raises(TypeError, match="ParabolicSOL"):
        M.estimate(par, 2.0)                                               # estimate() keeps refusing a run
    with pytest.raises(ValueError, match="dirichlet"):
        M.estimate_steps(par, 2.0, neumann=lambda x: 1.0)
    with pytest.raises(ValueError, match="two snapshots"):
        M.estimate_steps(M.ParabolicSOL(g.py, TS[:1], z[:1]), 2.0)
    with pytest.raises(ValueError, match="snapshots for"):
        M.estimate_steps(M.ParabolicSOL(g.py, TS, z[:3]), 2.0)
    with pytest.raises(ValueError, match="strictly increasing"):
        M.estimate_steps(M.ParabolicSOL(g.py, TS[::-1], z), 2.0)
    with pytest.raises(TypeError, match="geometry"):
        M.estimate_steps(par, 2.0)                                         # a native geometry


def test_refine_times(M):
    ts = np.array([0.0, 0.1, 0.4, 1.0, 1.5])
    assert M.refine_times(ts, [1]).tolist() == [0.0, 0.1, 0.25, 0.4, 1.0, 1.5]                       # a single interval
    every = M.refine_times(ts, [3, 0, 2, 1])                                                        # all of them, in any order
    assert every.tolist() == [0.0, 0.05, 0.1, 0.25, 0.4, 0.7, 1.0, 1.25, 1.5]
    assert every[::2].tobytes() == ts.tobytes()                                                     # the survivors keep bits and order
    none = M.refine_times(ts, [])
    assert none.tobytes() == ts.tobytes() and none is not ts and M.refine_times(ts, np.zeros(0, dtype=int)).tobytes() == ts.tobytes()
    odd = np.array([0.1, 0.30000000000000004, 0.7])
    got = M.refine_times(odd, [1])
    assert got[[0, 1, 3]].tobytes() == odd.tobytes() and got[2] == (odd[1] + odd[2]) / 2
    assert M.refine_times([0, 1], [0]).tolist() == [0.0, 0.5, 1.0]
    for bad in ([4], [-1], [1, 1], [0, 2, 0]):
        with pytest.raises(ValueError):
            M.refine_times(ts, bad)
    with pytest.raises(TypeError):
        M.refine_times(ts, [0.5])
    with pytest.raises(ValueError, match="midpoint"):
        M.refine_times([1.0, np.nextafter(1.0, 2.0)], [0])                 # no double lies strictly between
    for bad in ([0.0], [0.0, 0.0], [1.0, 0.0], [0.0, math.nan], np.zeros((2, 2))):
        with pytest.raises(ValueError):
            M.refine_times(bad, [])


def test_the_time_indicator_of_a_solved_run_falls_when_every_step_is_halved(M):
    """One oracle run per step size on fem1d L = 3, p = 2, default data, r = 2, through the yardstick: sum_k h_k time_k decreases
    strictly under halving (DESIGN.md section 4m has the figures), and at h = 0.25 Doerfler marking with theta = 0.5 on
    h_k time_k marks interval 0 alone."""
    import mgb_oracle as O
    g = mesh_of_oracle = XR.Mesh("fem1d_L3")
    sums = {}
    for h in (0.5, 0.25):
        par = O.parabolic_solve(O.fem1d(3), p=2.0, h=h)
        assert np.array_equal(np.asarray(par.geometry.x).reshape(-1), g.x.reshape(-1)) and len(par.ts) == round(1.0 / h) + 1
        Y = SR.step_indicators(g.ops, g.w, g.F, g.I, [np.asarray(z)[:, 0] for z in par.u], par.ts, 2.0, f=np.full(g.n, 0.5))
        sums[h], terms = SR.time_sum(Y, par.ts)
        print("fem1d L=3 p=2 h=%g: sum h_k time_k = %.6e, terms %s, space %s" % (h, sums[h], terms, Y["totals"][:, 0, :3].sum(axis=1)))
    assert 0.0 < sums[0.25] < sums[0.5]
    marked = M.mark(terms, 0.5)
    print("share of interval 0 at h = 0.25: %.3f" % (terms[0] / sums[0.25]))
    assert marked.tolist() == [0]
    del mesh_of_oracle
