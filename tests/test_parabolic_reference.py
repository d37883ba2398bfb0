"""CPU checks of the reference time loop (tests/parabolic_reference.py) that the GPU parity tests of parabolic_solve are held
to, and of the argument handling of parabolic_solve that needs no device."""
import numpy as np
import pytest

import mgb_oracle as O
import parabolic_reference as PR


def test_autonomous_data_reproduce_the_oracle_bitwise():
    """g(t, x) = DEFAULT_G(x), f1 = 0.5 and uniform steps: the loop is O.parabolic_solve bit for bit, and nothing is lifted."""
    geo = O.fem1d(2)
    ts = 0.0 + 0.5 * np.arange(3)
    u, lifts = PR.reference_loop(geo, 2.0, ts, lambda t, x: 0.5, lambda t, x: O.DEFAULT_G[1](x))
    ref = O.parabolic_solve(geo, h=0.5, t1=1.0, p=2.0)
    assert np.array_equal(ref.ts, ts) and len(u) == len(ref.u)
    for uk, rk in zip(u, ref.u):
        assert np.array_equal(uk, rk)
    assert np.array_equal(lifts, np.zeros((2, 2)))


# lifts per step of the fixture cases, as the loop gives them on the CPU oracle (two decimals)
FIXTURE_LIFTS = {("fem1d", 3): [(0, 0), (1.42, 1.64), (2.28, 2.60)],
                 ("fem2d", 2): [(1.71, 0), (2.31, 2.00), (4.87, 3.53)]}


@pytest.mark.parametrize("kind,L", [("fem1d", 3), ("fem2d", 2)])
def test_fixture_cases_stay_inside_both_cones_and_take_both_lift_branches(kind, L):
    p = 1.0
    geo, u, lifts = PR.fixture_loop(kind, L, p)
    dim = geo.discretization["dim"]
    n = geo.x.shape[0]
    assert len(u) == len(PR.TS) and lifts.shape == (len(PR.TS) - 1, 2)
    assert len(PR.boundary_nodes(geo.subspaces["dirichlet"][-1])) == {("fem1d", 3): 2, ("fem2d", 2): 26}[(kind, L)]
    assert n == {("fem1d", 3): 16, ("fem2d", 2): 56}[(kind, L)]
    ops = ("dx", "dy")[:dim]
    for z in u:
        grad2 = sum((geo.operators[o] @ z[:, 0]) ** 2 for o in ops)
        assert np.all(z[:, 1] > z[:, 0] ** 2) and np.all(z[:, 2] > grad2 ** (p / 2.0))
    assert np.any(lifts == 0.0) and np.any(lifts > 0.0)
    assert np.all((lifts == 0.0) | (lifts >= 1.0))
    print("lifts", kind, L, lifts.tolist())
    assert np.allclose(lifts, np.array(FIXTURE_LIFTS[(kind, L)], dtype=float), rtol=0, atol=0.006)      # half a unit of the second decimal


def test_fixture_cases_cover_every_lift_combination():
    """The two cases together take a zero and a non-zero lift in every combination that the data can produce."""
    seen = set()
    for kind, L in (("fem1d", 3), ("fem2d", 2)):
        seen |= {(bool(a), bool(b)) for a, b in PR.fixture_loop(kind, L, 1.0)[2]}
    assert {(False, False), (True, False), (True, True)} <= seen


def test_boundary_values_follow_g_in_the_reference_loop():
    geo, u, _ = PR.fixture_loop("fem1d", 3, 1.0)
    bidx = PR.boundary_nodes(geo.subspaces["dirichlet"][-1])
    for t, z in zip(PR.TS, u):
        assert np.array_equal(z[bidx, 0], np.array([PR.G_T[1](t, geo.x[b])[0] for b in bidx]))


# ---- argument handling of parabolic_solve that needs no device

def test_arity_detection():
    import mgb_amd as M
    assert M._positional_arity(lambda x: 0.5, "f1") == 1
    assert M._positional_arity(lambda t, x: 0.5, "f1") == 2
    assert M._positional_arity(M.DEFAULT_G[1], "g") == 1 and M._positional_arity(M.DEFAULT_G[2], "g") == 1

    def two(t, x, *, scale=1.0):
        return scale

    assert M._positional_arity(two, "g") == 2
    for bad, name in ((lambda a, b, c: 0.5, "f1"), (lambda: 0.5, "g"), (lambda *a: 0.5, "f1")):
        with pytest.raises(TypeError, match=name):
            M._positional_arity(bad, name)


def test_ts_validation():
    import mgb_amd as M
    ts, hs = M._parabolic_times(0.2, 0.0, 1.0, [0.0, 0.3, 0.5, 1.0])
    assert np.array_equal(ts, PR.TS) and np.array_equal(hs, np.diff(PR.TS))
    ts, hs = M._parabolic_times(0.25, 0.0, 1.0, None)      # without ts= every step is h itself, as before
    assert np.array_equal(ts, 0.0 + 0.25 * np.arange(5)) and np.array_equal(hs, np.full(4, 0.25))
    for bad in ([0.0], [0.0, 0.5, 0.5], [0.0, 1.0, 0.5], [0.0, np.nan, 1.0], [0.0, np.inf], [[0.0, 1.0]], []):
        with pytest.raises(ValueError, match="ts"):
            M._parabolic_times(0.2, 0.0, 1.0, bad)


def test_forcing_forms():
    import mgb_amd as M
    x = np.linspace(0.0, 1.0, 5).reshape(-1, 1)
    ts = PR.TS
    timed, row = M._parabolic_forcing(lambda xi: 2.0 * xi[0], x, ts)
    assert not timed and np.array_equal(row(0), 2.0 * x[:, 0]) and np.array_equal(row(2), 2.0 * x[:, 0])
    timed, row = M._parabolic_forcing(lambda t, xi: t * xi[0], x, ts)
    assert timed and np.array_equal(row(1), ts[2] * x[:, 0])      # step k ends at ts[k + 1]
    timed, row = M._parabolic_forcing(np.arange(5.0), x, ts)
    assert not timed and np.array_equal(row(1), np.arange(5.0))
    F = np.arange(15.0).reshape(3, 5)
    timed, row = M._parabolic_forcing(F, x, ts)
    assert timed and np.array_equal(row(2), F[2])
    for bad in (np.zeros(4), np.zeros((2, 5)), np.zeros((4, 5)), np.zeros((3, 4))):
        with pytest.raises(ValueError, match="f1"):
            M._parabolic_forcing(bad, x, ts)
    with pytest.raises(TypeError, match="f1"):
        M._parabolic_forcing(lambda a, b, c: 0.0, x, ts)


def test_parabolic_sol_lift_defaults_to_none():
    import mgb_amd as M
    sol = M.ParabolicSOL("geometry", np.zeros(2), [1, 2])
    assert sol.lift is None and (sol.geometry, sol.u) == ("geometry", [1, 2])
    assert [f.name for f in __import__("dataclasses").fields(M.ParabolicSOL)] == ["geometry", "ts", "u", "lift"]
