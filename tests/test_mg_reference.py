"""CPU tests of tests/mg_reference.py, the restatement test_gpu_vcycle.py holds the device V-cycle and CG to: what the
restatement must be by construction (an exact solve on one level, a symmetric positive operator, CG that stops after one step
with an exact preconditioner and reaches the direct solution), and how far its float64 run is from its long-double run on
every input the GPU tests use.  Those distances feed the GPU tolerances (mg_reference.bound); run with -s for the figures
(profiles/vcycle_reference.txt keeps them)."""
import numpy as np
import pytest
import scipy.sparse as sp

import mg_reference as R

LD = R.LD
DEGREES = (1, 2, 3, 4)


_id = R.case_id


@pytest.mark.parametrize("case", R.CASES, ids=_id)
def test_inputs_are_inside_the_cone_and_positive_definite(case):
    """The guard of every case (fem1d L=8 p=2 with this s fails it: an indefinite H): the point is strictly inside the cone, the
    top Hessian has a Cholesky factor, the levels are the ones the shapes were chosen for, and R_{l+1} P_l = R_l."""
    S = R.system(*case)
    assert S.inside and S.is_spd()
    want = {("fem2d", 4): (1, [50, 194, 770]), ("fem2d", 5): (1, [50, 194, 770, 3074]), ("fem3d", 3): (0, [72, 468, 3528]),
            ("fem1d", 7): (5, [128, 256]), ("fem1d", 6): (5, [128]), ("fem2d", 2): (1, [50]),
            ("fem2d", 3, "graded4"): (0, [182, 722, 2882]), ("fem2d", 4, "lshape"): (0, [38, 146, 578, 2306])}[case[:2] + case[3:]]
    assert (S.c0, S.sizes[S.c0:]) == want
    if case[3:] == ("graded4",):      # no level is small enough for the dense inverse: level 0 it is, above kDenseMax
        assert S.c0 == 0 and min(S.sizes) > R.DENSE_MAX
    for l in range(S.c0, S.top):
        assert abs(S.Mo.R[l + 1] @ S.P[l] - S.Mo.R[l]).max() < 1e-12
        # Galerkin: the oracle's H_l is P_l' H_{l+1} P_l
        G = S.P[l].T @ S.H[l + 1] @ S.P[l]
        assert abs(G - S.H[l]).max() <= 1e-12 * abs(S.H[l]).max()


@pytest.mark.parametrize("case", R.COARSE, ids=_id)
def test_vcycle_on_one_level_is_the_inverse(case):
    S = R.system(*case)
    assert S.top == S.c0
    b = S.random(R.B_SEED)
    H = S.H[S.top]
    x = S.V(2, LD)(b)
    assert R.rel(R.Mat(H, LD) @ x, b) < 1e-12
    assert R.rel(x, np.linalg.solve(H.toarray(), b)) < 1e-9
    assert R.rel(S.V(2, np.float64)(b), x) < 1e-11


@pytest.mark.parametrize("case", R.MULTI, ids=_id)
def test_vcycle_is_symmetric_and_positive(case):
    S = R.system(*case)
    g, u = S.random(R.B_SEED), S.random(R.U_SEED)
    for degree in DEGREES:
        for dt, tol in ((LD, 1e-14), (np.float64, 1e-12)):
            V = S.V(degree, dt)
            Vg, Vu = V(g), V(u)
            a, b = u.astype(dt) @ Vg, g.astype(dt) @ Vu
            print("%s degree %d %-10s |<u,Vg> - <g,Vu>| / |<u,Vg>| = %.1e" % (_id(case), degree, dt.__name__, abs(a - b) / abs(a)))
            assert abs(a - b) <= tol * abs(a)
            assert g.astype(dt) @ Vg > 0 and u.astype(dt) @ Vu > 0


@pytest.mark.parametrize("case", [("fem2d", 4, 1.0), ("fem3d", 3, 1.5), ("fem1d", 7, 1.0)], ids=_id)
def test_bound_tells_a_wrong_vcycle_apart(case):
    """What the 1e-11 of the GPU tests can see: a lambda off by 1e-9 relative on one level, a coarse correction off by 1e-6
    relative, and a post-smoothing that starts from the pre-smoothed x (a stale vector) all move V(b) by more than that bound."""
    S = R.system(*case)
    b = S.random(R.B_SEED)
    for degree in DEGREES:
        V = S.V(degree, LD)
        want = V(b)
        lam = dict(S.lam)
        lam[S.top] *= 1 + 1e-9
        assert R.rel(S.V(degree, LD, lam=lam)(b), want) > 1e-11

        class Scaled(R.Vcycle):
            def __call__(self, b, l=None):
                x = super().__call__(b, l)
                return x * (1 + LD(1e-6)) if l is not None and l == self.top - 1 else x

        assert R.rel(Scaled(S.H, S.P, S.lam, S.c0, S.top, degree, LD)(b), want) > 1e-11
        H = R.Mat(S.H[S.top], LD)
        x = R.cheb(H, b.astype(LD), np.zeros(S.N, dtype=LD), S.lam[S.top], degree)
        stale = R.cheb(H, b.astype(LD), x, S.lam[S.top], degree)      # the prolonged correction never reached x
        assert R.rel(stale, want) > 1e-3


@pytest.mark.parametrize("case", R.COARSE, ids=_id)
def test_pcg_with_an_exact_preconditioner_stops_after_one_iteration(case):
    S = R.system(*case)
    for dt in (np.float64, LD):
        res = S.cg(2, 1e-11, 300, dt)
        assert (res.it, res.code) == (1, 1)
        assert R.rel(res.x[1], S.direct(S.g)) < 1e-9


@pytest.mark.parametrize("case", R.MULTI, ids=_id)
def test_pcg_reaches_the_direct_solution(case):
    S = R.system(*case)
    want = S.direct(S.g)
    for degree in (1, 2, 3):
        res = S.cg(degree, 1e-11, 300, np.float64)
        assert res.code == 1 and 1 < res.it < 60
        assert R.rel(res.x[-1], want) < 1e-8
        assert all(a > 0 for a in res.alpha) and all(b > 0 for b in res.beta)


def test_pcg_stop_codes():
    """Zero right-hand side: code 1 at iteration 0; a NaN: code 2 at iteration 0; the cap: code 3 with it == maxit, and the
    tolerance is looked at before the cap."""
    S = R.system("fem2d", 4, 1.0)
    H, V = R.Mat(S.H[S.top], np.float64), S.V(2, np.float64)
    z = R.pcg(H, V, np.zeros(S.N), 1e-11, 10)
    assert (z.it, z.code) == (0, 1) and not z.x[0].any()
    g = S.g.copy()
    g[3] = np.nan
    n = R.pcg(H, V, g, 1e-11, 10)
    assert (n.it, n.code) == (0, 2)
    for k in (1, 2, 3, 4):
        r = S.cg(2, 1e-14, k, np.float64)
        assert (r.it, r.code, len(r.x)) == (k, 3, k + 1)
    full = S.cg(2, 1e-11, 300, np.float64)
    assert R.pcg(H, V, S.g, 1e-11, full.it).code == 1      # converged at the cap: converged


@pytest.mark.parametrize("case", R.CASES, ids=_id)
def test_float64_and_long_double_restatements_agree(case):
    """The condition of the 1e-11 the GPU tests give V(b): on each chosen input the two restatements agree to 1e-12.  Prints
    the distances that mg_reference.bound turns into the bounds of x_k and relres."""
    S = R.system(*case)
    b = S.random(R.B_SEED)
    for degree in (DEGREES if case in R.MULTI else (2,)):
        d = R.rel(S.V(degree, np.float64)(b), S.V(degree, LD)(b))
        print("%s degree %d: V(b) float64 - long double %.2e" % (_id(case), degree, d))
        assert d < 1e-12
    if case not in R.MULTI:
        return
    for degree in (1, 2):
        r64, rld = S.cg(degree, 1e-14, 4, np.float64), S.cg(degree, 1e-14, 4, LD)
        assert r64.it == rld.it == 4
        for k in (1, 2, 3, 4):
            dx = R.rel(r64.x[k], rld.x[k])
            dr = abs(r64.relres(k) - rld.relres(k)) / rld.relres(k)
            print("%s degree %d k=%d: x_k %.2e (bound %.1e)  relres %.2e (bound %.1e)  alpha %.1e beta %.1e"
                  % (_id(case), degree, k, dx, R.bound(dx), dr, R.bound(dr), abs(r64.alpha[k - 1] / rld.alpha[k - 1] - 1),
                     abs(r64.beta[k - 1] / rld.beta[k - 1] - 1)))
            assert dx < 1e-12 and dr < 1e-12


@pytest.mark.parametrize("key", sorted(R.COUNT_CASES), ids=lambda k: "%s-L%d-p%g-degree%d" % k)
def test_iteration_count_inputs_stop_away_from_the_threshold(key):
    """The seeds of COUNT_CASES: at the last two iterations <r, V r> / (rtol^2 <r0, V r0>) is outside [0.25, 4] in both
    restatements, which count the same."""
    kind, L, p, degree = key
    S = R.system(kind, L, p)
    r64 = S.cg(degree, R.COUNT_RTOL, 300, np.float64, R.COUNT_CASES[key])
    rld = S.cg(degree, R.COUNT_RTOL, 300, LD, R.COUNT_CASES[key])
    m = R.count_margins(rld)
    print("%s-L%d-p%g degree %d: %d iterations, <r,Vr> / threshold %.2f then %.3f" % (kind, L, p, degree, rld.it, m[0], m[1]))
    assert rld.code == r64.code == 1 and rld.it == r64.it
    assert m[0] > 4 and m[1] < 0.25
    m64 = R.count_margins(r64)
    assert m64[0] > 4 and m64[1] < 0.25


def test_nodal_prolongation_and_dense_helpers():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((40, 40))
    A = A @ A.T + 40 * np.eye(40)
    for dt in (np.float64, LD):
        Lc = R.cholesky(A.astype(dt))
        assert R.rel((Lc @ Lc.T).ravel(), A.ravel()) < 1e-14
        X = R.chol_solve(Lc, np.eye(40, dtype=dt)[:, :7])
        assert R.rel((A.astype(dt) @ X).ravel(), np.eye(40)[:, :7].ravel()) < 1e-13
    with pytest.raises(np.linalg.LinAlgError):
        R.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))
    M = sp.random(30, 20, 0.2, random_state=1, format="csr")
    x = rng.standard_normal(20)
    assert R.rel(R.Mat(M, LD) @ x.astype(LD), M @ x) < 1e-14
    assert R.rel(R.Mat(M, LD).T @ np.ones(30, dtype=LD), M.T @ np.ones(30)) < 1e-14
