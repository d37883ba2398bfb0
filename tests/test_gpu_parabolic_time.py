"""parabolic_solve with f1(t, x), g(t, x) and variable steps: the step transition between two barrier solves runs on the device
(csrc/parabolic.hip; contract in include/mgb_hip.h).  The kernels are held to the numpy restatement of
tests/parabolic_reference.py -- bitwise where the contract says so --, the whole loop to that module's reference loop over the
CPU oracle."""
import numpy as np
import pytest

import mgb_oracle as O
import parabolic_reference as PR

pytestmark = pytest.mark.gpu
KTOL = 1e-12      # the project's kernel-parity bar (tests/test_gpu_parabolic.py)
MGB_E_ARG, MGB_E_NUMERIC = -1, -3

# fem3d L=1 is the smallest mesh fem3d_mpi builds (Q3: the largest element block, n = 64 is below one workgroup); fem2d L=4
# (n = 896) is three and a half workgroups of 256: the cross-workgroup pass of the reduction and a partly idle last workgroup
SHAPES = {"fem1d_L2": ("fem1d", 2, 8, 2), "fem2d_L2": ("fem2d", 2, 56, 26), "fem3d_L1": ("fem3d", 1, 64, 56),
          "fem2d_L4": ("fem2d", 4, 896, None)}


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


class Problem:
    """An AMG with the parabolic layout on one of SHAPES, with the host pieces the numpy restatement needs."""

    def __init__(self, M, shape, p):
        kind, L, n, nb = SHAPES[shape]
        self.geo = getattr(M, kind + "_mpi")(L)
        self.p = float(p)
        state, D, self.K, cones, ops = O.parabolic_problem(self.geo, self.p)
        self.A = M.AMG(self.geo, state, D, self.p, cones=cones)
        self.n = self.A.n
        self.ops = [self.geo.operators[o].host for o in ops]
        self.bidx = PR.boundary_nodes(self.geo.subspaces["dirichlet"][-1].host)
        assert self.n == n and (nb is None or len(self.bidx) == nb)
        self.A.parabolic_begin(self.bidx)

    def grad_p(self, u):
        return sum((op @ u) ** 2 for op in self.ops) ** (self.p / 2.0)

    def feasible(self, u, rng):
        """[u; s1; s2] strictly inside both cones, by a margin of at least 1/2."""
        n = self.n
        return np.concatenate([u, u * u + 0.5 + rng.random(n), self.grad_p(u) + 0.5 + rng.random(n)])

    def reference(self, z, h, f, gb):
        return PR.step_transition(z, self.n, self.K, self.p, h, f, self.bidx, gb, self.ops)


_PROBLEMS = {}


def problem(M, shape, p):
    if (shape, p) not in _PROBLEMS:
        _PROBLEMS[(shape, p)] = Problem(M, shape, p)
    return _PROBLEMS[(shape, p)]


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def lifts_match(got, want, tol):
    for a, b in zip(got, want):
        if b == 0.0:
            assert a == 0.0, (got, want)
        else:
            assert abs(a - b) <= tol * abs(b), (got, want)


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_kernels_match_numpy(M, shape, p):
    P = problem(M, shape, p)
    A, n = P.A, P.n
    rng = np.random.default_rng(11)
    z = P.feasible(rng.standard_normal(n), rng)
    f, gb, h = rng.standard_normal(n), 2.0 * rng.standard_normal(len(P.bidx)), 0.3
    A.set_z(z)
    lifts = A.parabolic_step(h, p, M.HPCVector(f), M.HPCVector(gb))
    c_ref, z_ref, v_ref, l_ref = P.reference(z, h, f, gb)
    print("%s p=%g  v=(%.6g, %.6g)  lifts %r  reference %r" % (shape, p, v_ref[0], v_ref[1], lifts.tolist(), l_ref))
    assert np.array_equal(A.get_c(), c_ref)                                   # the cost, from the OLD u: bitwise
    z1 = A.get_z()
    interior = np.ones(n, dtype=bool)
    interior[P.bidx] = False
    assert np.array_equal(z1[:n][P.bidx], gb) and np.array_equal(z1[:n][interior], z[:n][interior])
    lifts_match(lifts, l_ref, KTOL)
    assert np.array_equal(z1[n:2 * n], z[n:2 * n] + lifts[0]) and np.array_equal(z1[2 * n:], z[2 * n:] + lifts[1])
    assert np.isfinite(A.f0(A.L - 1, np.zeros(A.level_size(A.L - 1)[0]), 0.1))


@pytest.mark.parametrize("case", ["last_node", "node_0", "nothing", "contact", "cone_2_only"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_placement_of_the_violation(M, shape, case):
    p = 1.5
    P = problem(M, shape, p)
    A, n = P.A, P.n
    rng = np.random.default_rng(5)
    u = rng.standard_normal(n)
    j = {"last_node": n - 1, "node_0": 0, "nothing": None, "contact": n // 2, "cone_2_only": n // 3}[case]
    if case == "contact":
        u[j] = 2.0
    z = P.feasible(u, rng)
    if case in ("last_node", "node_0"):
        z[n + j] = u[j] * u[j] - 0.5
    elif case == "contact":
        z[n + j] = 4.0
    elif case == "cone_2_only":
        z[2 * n + j] = P.grad_p(u)[j] - 0.25
    f = rng.standard_normal(n)
    A.set_z(z)
    lifts = A.parabolic_step(0.3, p, M.HPCVector(f), None)      # no boundary data: u stays
    _, z_ref, v_ref, l_ref = P.reference(z, 0.3, f, None)
    z1 = A.get_z()
    assert np.array_equal(z1[:n], z[:n])
    lifts_match(lifts, l_ref, KTOL)
    assert np.array_equal(z1[n:2 * n], z[n:2 * n] + lifts[0]) and np.array_equal(z1[2 * n:], z[2 * n:] + lifts[1])
    if case == "nothing":
        assert lifts[0] == 0.0 and lifts[1] == 0.0 and np.array_equal(z1, z)
    elif case == "contact":
        assert lifts[0] == 1.0 and lifts[1] == 0.0
    elif case == "cone_2_only":
        assert lifts[0] == 0.0 and lifts[1] > 1.0 and np.array_equal(z1[n:2 * n], z[n:2 * n])
    else:
        assert lifts[0] > 1.0 and lifts[1] == 0.0 and np.array_equal(z1[2 * n:], z[2 * n:])
    assert np.isfinite(A.f0(A.L - 1, np.zeros(A.level_size(A.L - 1)[0]), 0.1))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_snapshot(M, shape):
    P = problem(M, shape, 1.5)
    A, n = P.A, P.n
    rng = np.random.default_rng(2)
    z = P.feasible(rng.standard_normal(n), rng)
    A.set_z(z)
    s0 = A.snapshot()
    assert isinstance(s0, M.HPCMatrix) and s0.shape == (n, 3)
    assert np.array_equal(s0.to_numpy(), A.get_z().reshape(n, 3, order="F")) and np.array_equal(s0.to_numpy(), z.reshape(n, 3, order="F"))
    A.parabolic_step(0.3, 1.5, M.HPCVector(rng.standard_normal(n)), M.HPCVector(3.0 * np.ones(len(P.bidx))))
    s1 = A.snapshot()
    assert s1._v.handle.value != s0._v.handle.value
    assert np.array_equal(s0.to_numpy(), z.reshape(n, 3, order="F"))              # the earlier snapshot owns its storage
    assert np.array_equal(s1.to_numpy(), A.get_z().reshape(n, 3, order="F")) and not np.array_equal(s1.to_numpy(), s0.to_numpy())


def test_non_finite_state_is_an_error(M):
    """A NaN or an Inf in u (and with it in Dz0) or in a slack surfaces as an MGBError, never as a silent max."""
    P = problem(M, "fem2d_L4", 1.5)
    A, n = P.A, P.n
    rng = np.random.default_rng(3)
    f = M.HPCVector(rng.standard_normal(n))
    for where, bad in ((n - 1, np.nan), (300, np.inf), (n + 7, -np.inf), (2 * n + 600, np.inf)):
        z = P.feasible(rng.standard_normal(n), rng)
        z[where] = bad
        A.set_z(z)
        with pytest.raises(M.MGBError) as e:
            A.parabolic_step(0.3, 1.5, f, None)
        assert e.value.code == MGB_E_NUMERIC
        A.set_z(z)
        assert A.parabolic_step(0.3, 1.5, f, None, wait=False) is None      # ... and behind the call that does not wait
        with pytest.raises(M.MGBError) as e:
            A.parabolic_lifts()
        assert e.value.code == MGB_E_NUMERIC


SOLVE_CASES = [("fem1d", 2, 2.0), ("fem1d", 3, 1.0), ("fem2d", 2, 1.5), ("fem2d", 2, 1.0)]


@pytest.mark.parametrize("kind,L,p", SOLVE_CASES)
def test_solve_matches_reference_loop(M, kind, L, p):
    """Every snapshot against the reference loop at the bars of test_parabolic_matches_oracle: u to 1e-10 relative l2, all
    columns to 1e-8 (the slack columns sit within 1/t = 1e-8 of their cones along flat directions of the objective).  The
    oracle's own sensitivity to a 1e-14 relative perturbation of u0 on these cases is <= 8e-12 in u and <= 2e-11 overall."""
    go, u_ref, lift_ref = PR.fixture_loop(kind, L, p)
    dim = go.discretization["dim"]
    g = getattr(M, kind + "_mpi")(L)
    sol = M.parabolic_solve(g, p=p, f1=PR.F_T[dim], g=PR.G_T[dim], ts=PR.TS)
    assert isinstance(sol, M.ParabolicSOL) and sol.geometry is g and np.array_equal(sol.ts, PR.TS)
    assert len(sol.u) == len(PR.TS) and all(isinstance(uk, M.HPCMatrix) for uk in sol.u)
    nat = M.mpi_to_native(sol)
    assert np.array_equal(nat.lift, sol.lift) and sol.lift.shape == (len(PR.TS) - 1, 2)
    print("%s L=%d p=%g lifts %r  reference %r" % (kind, L, p, sol.lift.tolist(), lift_ref.tolist()))
    gaps = [(rel(uk[:, 0], rk[:, 0]), rel(uk, rk)) for uk, rk in zip(nat.u, u_ref)]
    print("%s L=%d p=%g snapshot gaps (u, all columns): %s" % (kind, L, p, ", ".join("(%.2e, %.2e)" % ab for ab in gaps)))
    for k in range(len(lift_ref)):
        lifts_match(sol.lift[k], lift_ref[k], 1e-10)
    for (gu, ga), uk, rk in zip(gaps, nat.u, u_ref):
        assert uk.shape == rk.shape
        assert gu < 1e-10
        assert ga < 1e-8


def test_autonomous_equivalence(M):
    """Uniform steps and data that do not depend on t: the (t, x) convention and the one-argument call give the same bits."""
    g = M.fem1d_mpi(2)
    a = M.parabolic_solve(g, h=0.5, t1=1.0, p=2.0, f1=lambda t, x: 0.5, g=lambda t, x: M.DEFAULT_G[1](x))
    b = M.parabolic_solve(g, h=0.5, t1=1.0, p=2.0)
    assert np.array_equal(a.ts, b.ts) and len(a.u) == len(b.u) == 3
    for ua, ub in zip(a.u, b.u):
        assert np.array_equal(ua.to_numpy(), ub.to_numpy())
    assert np.array_equal(a.lift, np.zeros((2, 2))) and np.array_equal(b.lift, np.zeros((2, 2)))


def test_array_forcing_is_the_callable_forcing(M):
    g = M.fem1d_mpi(2)
    x = g.x.to_numpy()
    F = np.array([[PR.F_T[1](t, xi) for xi in x] for t in PR.TS[1:]])
    a = M.parabolic_solve(g, p=2.0, f1=PR.F_T[1], g=PR.G_T[1], ts=PR.TS)
    b = M.parabolic_solve(g, p=2.0, f1=F, g=PR.G_T[1], ts=PR.TS)
    for ua, ub in zip(a.u, b.u):
        assert np.array_equal(ua.to_numpy(), ub.to_numpy())
    assert np.array_equal(a.lift, b.lift)


def test_errors(M):
    g = M.fem1d_mpi(2)
    n = g.x.shape[0]
    for bad in ([0.0, 0.5, 0.5], [0.0, 1.0, 0.5], [0.0], [0.0, np.nan, 1.0], [0.0, np.inf]):
        with pytest.raises(ValueError, match="ts"):
            M.parabolic_solve(g, ts=bad)
    with pytest.raises(TypeError, match="f1"):
        M.parabolic_solve(g, f1=lambda t, x, y: 0.5)
    with pytest.raises(TypeError, match="g"):
        M.parabolic_solve(g, g=lambda: np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="f1"):
        M.parabolic_solve(g, f1=np.zeros((2, n)), ts=PR.TS)               # three steps need three rows
    with pytest.raises(ValueError, match="f1"):
        M.parabolic_solve(g, f1=np.zeros((3, n + 1)), ts=PR.TS)
    A = M.AMG(g)                                                           # the default two-variable layout
    with pytest.raises(M.MGBError) as e:
        A.parabolic_begin([0, n - 1])
    assert e.value.code == MGB_E_ARG
    with pytest.raises(M.MGBError) as e:                                   # ... and no step without a begin
        A.parabolic_step(0.3, 1.0, M.HPCVector(np.zeros(n)), None)
    assert e.value.code == MGB_E_ARG
    P = problem(M, "fem1d_L2", 1.5)
    for bad in ([0, n], [-1]):
        with pytest.raises(M.MGBError) as e:
            P.A.parabolic_begin(bad)
        assert e.value.code == MGB_E_ARG
    P.A.parabolic_begin(P.bidx)
    f = M.HPCVector(np.zeros(n))
    for args in ((0.0, 1.5, f, None), (-0.1, 1.5, f, None), (0.3, 0.5, f, None), (0.3, 1.5, M.HPCVector(np.zeros(n + 1)), None),
                 (0.3, 1.5, f, M.HPCVector(np.zeros(len(P.bidx) + 1)))):
        with pytest.raises(M.MGBError) as e:
            P.A.parabolic_step(*args)
        assert e.value.code == MGB_E_ARG
