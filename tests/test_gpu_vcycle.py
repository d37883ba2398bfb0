"""GPU tests of what lies between the multigrid pieces and the whole solver="pcg" (`-m gpu`, through the C ABI): the V-cycle
Amg::mg_vcycle as CG enqueues it, the dense coarse inverse, every CG iterate with its scalars, the stop codes and the `done`
flag, chunk / maxit, and the fallback bookkeeping of a solve.

Reference: tests/mg_reference.py, a numpy restatement of the V-cycle and of CG run in long double on the oracle's Hessians
H_l (the oracle's f2 on R_l at the top-level point).  Two hooks make the device comparable with it: AMG.pin_lmax hands every
level the lambda_max(D^-1 H_l) that scipy's eigsh computes from the reference H_l (the device's own warm-started estimate
differs from call to call), and AMG.vcycle returns V(b) itself and the lambda each level used.  P_l of the library is held to
the reference's own nodal restatement here, on top of R_{l+1} P_l = R_l in test_gpu_mg.py.

Two hierarchies come from coarse meshes of tests/mesh_cases.py: fem2d L=3 on graded4 (N = 182, 722, 2882: no level fits the dense
inverse, so mg_coarsest is level 0 and the coarse solve of the V-cycle is the device Cholesky) and fem2d L=4 on the L shape (N = 38
.. 2306: the dense inverse under an irregular hierarchy).

Tolerances, none from the code under test (figures: profiles/vcycle_reference.txt, from test_mg_reference.py -s and a run of
this file with -s):
  V(b)                    1e-11 relative, what test_gpu_mg.py gives the same recurrences on one level; the float64 and long-double
                          restatements agree to 1e-12 on every input used (3.5e-15 at worst), test_mg_reference.py asserts it
  x_k, relres, Ainv       mg_reference.bound: 100 times the distance between the float64 and the long-double restatement of the
                          same quantity (the device sums in another order), at least 1e-11
  symmetry of V           1e-12 relative (the float64 restatement: 1e-15 in 2-D and 3-D, 5.5e-14 on fem1d L=7 at degree 1, where
                          <u, V g> cancels; the device there: 4.9e-13)
  the device's own lambda [0.9, 1 + 1e-10] lambda_max, the bound test_gpu_mg.py uses on one level
  iteration counts        equal; the inputs stop a factor 4 away from the threshold on either side (COUNT_CASES)"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import mg_reference as R
from test_gpu_parity import _match_columns, rel, ZTOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LD = R.LD
DEFAULTS = dict(rtol=1e-9, maxit=200, degree=2, chunk=4, fallback=True, assembled_top=False, giveup=3,
                lo_frac=R.LO_FRAC, hi_frac=R.HI_FRAC)      # PcgOptions, csrc/amg.hpp


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_id = R.case_id


class Dev:
    """The library's AMG of a case next to the reference System: same c, z0, s; pi[l] maps the oracle's numbering of level l to
    the library's; every level of the V-cycle pinned to the reference's lambda_max."""

    def __init__(self, M, case):
        kind, L, p = case[:3]
        mesh = case[3] if len(case) > 3 else None      # a name of mesh_cases.MESHES: fem2d_mpi(L, K)
        self.S = S = R.system(*case)
        assert S.inside and S.is_spd()      # strictly inside the cone, and the top Hessian has a Cholesky factor
        self.A = A = M.AMG(getattr(M, kind + "_mpi")(L) if mesh is None else M.fem2d_mpi(L, R.MESHES[mesh]), p=p)
        A.set_c(S.c)
        A.set_z(S.z0)
        sub = A.geometry.subspaces
        self.pi = {}
        for l in range(S.c0, L):
            Rg = sp.block_diag([sub["dirichlet"][l].host, sub["full"][l].host], format="csr")
            self.pi[l] = _match_columns(S.Mo.R[l], Rg)
            assert A.level_size(l)[0] == S.sizes[l]
        assert A.mg_coarsest(S.top) == S.c0
        if mesh == "graded4":      # the case of the Cholesky coarse solve: level 0, too large for the dense inverse
            assert A.mg_coarsest(S.top) == 0 and A.level_size(0)[0] == S.sizes[0] > R.DENSE_MAX
        for l in range(S.c0, S.top):
            Pg = A.prolongation(l).tocsr()
            assert abs(Pg[self.pi[l + 1]][:, self.pi[l]] - S.P[l]).max() < 1e-13
        self.sg = self.to_dev(S.s)
        self.pin()
        A.set_pcg(**DEFAULTS)

    def pin(self, on=True):
        for l, lam in self.S.lam.items():
            self.A.pin_lmax(l, lam if on else 0.0)

    def to_dev(self, v):
        out = np.zeros(self.S.N)
        out[self.pi[self.S.top]] = v
        return out

    def V(self, b):
        """(V(b) in the oracle's numbering, lambda used per level)"""
        x, used = self.A.vcycle(self.S.top, self.sg, self.to_dev(b))
        return x[self.pi[self.S.top]], used

    def cg(self, g):
        x, it, rr, ok = self.A.pcg_solve_linear(self.S.top, self.sg, self.to_dev(g))
        return x[self.pi[self.S.top]], it, rr, ok


_devs = {}


def _dev(M, case):
    if case not in _devs:
        _devs[case] = Dev(M, case)
    d = _devs[case]
    d.pin()
    d.A.set_pcg(**DEFAULTS)
    return d


# ---------------------------------------------------------------------------------------------------------------- 1, 2: V
@pytest.mark.parametrize("case", R.MULTI, ids=_id)
def test_vcycle_matches_restatement(M, case):
    """1. V(b) of the device against the long-double restatement at 1e-11, degrees 1 .. 4 (degree 1: the extra waxpby launch),
    top level matrix-free and assembled; the lambda each level used is the pinned one, bit for bit."""
    D = _dev(M, case)
    S = D.S
    b = S.random(R.B_SEED)
    lam = np.zeros(S.L)
    for l, v in S.lam.items():
        lam[l] = v
    worst = 0.0
    for degree in (1, 2, 3, 4):
        want = S.V(degree, LD)(b)
        for assembled in (False, True):
            D.A.set_pcg(degree=degree, assembled_top=assembled)
            got, used = D.V(b)
            err = rel(got, want.astype(np.float64))
            worst = max(worst, err)
            print("%s degree %d assembled_top %d: V(b) device - long double %.2e (bound 1e-11)" % (_id(case), degree, assembled, err))
            assert np.array_equal(used, lam)
            assert err < 1e-11
    assert worst < 1e-11


@pytest.mark.parametrize("case", R.MULTI, ids=_id)
def test_vcycle_is_a_symmetric_positive_reproducible_operator(M, case):
    """2. <u, V g> = <g, V u> to 1e-12, <g, V g> > 0, three calls bit for bit; and unpinned, every level's own estimate lies in
    [0.9, 1 + 1e-10] lambda_max."""
    D = _dev(M, case)
    S = D.S
    g, u = S.random(R.B_SEED), S.random(R.U_SEED)
    for degree in (1, 2, 3):
        for assembled in (False, True):
            D.A.set_pcg(degree=degree, assembled_top=assembled)
            Vg, _ = D.V(g)
            Vu, _ = D.V(u)
            a, b = u @ Vg, g @ Vu
            print("%s degree %d assembled_top %d: |<u,Vg> - <g,Vu>| / |<u,Vg>| = %.1e" % (_id(case), degree, assembled, abs(a - b) / abs(a)))
            assert abs(a - b) <= 1e-12 * abs(a)
            assert g @ Vg > 0 and u @ Vu > 0
            assert all(np.array_equal(Vg, D.V(g)[0]) for _ in range(3))
    D.A.set_pcg(degree=2, assembled_top=False)
    Vg = D.V(g)[0]
    D.pin(False)
    try:
        _, used = D.V(g)
    finally:
        D.pin()
    for l in range(S.L):
        if l in S.lam:
            print("%s level %d: device estimate / lambda_max = %.4f" % (_id(case), l, used[l] / S.lam[l]))
            assert 0.9 * S.lam[l] <= used[l] <= S.lam[l] * (1 + 1e-10)
        else:
            assert used[l] == 0.0
    # pinned again: the pinned cycle is back, bit for bit
    assert np.array_equal(D.V(g)[0], Vg)


def test_pin_lmax_rejects_bad_arguments(M):
    D = _dev(M, ("fem2d", 4, 1.0))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(M._lib.MGBError):
            D.A.pin_lmax(2, bad)
    for l in (-1, D.S.L):
        with pytest.raises(M._lib.MGBError):
            D.A.pin_lmax(l, 1.0)


# ---------------------------------------------------------------------------------------------------------------- 3: coarse inverse
@pytest.mark.parametrize("case", R.COARSE, ids=_id)
def test_coarse_inverse_matches_long_double_solve(M, case):
    """3. top == c0: V is the dense inverse.  Its columns V(e_j) (all of them at N = 50, a random third at N = 128) are exactly
    symmetric among themselves, H Ainv = I and Ainv and V(b) match the long-double Cholesky solve within mg_reference.bound of
    the float64 Cholesky solve's own distance; CG on such a level stops after one iteration, converged."""
    D = _dev(M, case)
    S = D.S
    N, pi = S.N, D.pi[S.top]
    assert S.top == S.c0 and N <= R.DENSE_MAX
    rng = np.random.default_rng(3)
    J = np.arange(N) if N <= 64 else np.sort(rng.choice(N, N // 3, replace=False))      # columns, in the oracle's numbering
    E = np.eye(N)[:, J]
    got = np.stack([D.V(E[:, k])[0] for k in range(len(J))], axis=1)
    assert np.array_equal(got[J, :], got[J, :].T)      # the kernel's last loop: 0.5 (M_ij + M_ji), exactly symmetric
    Hd = S.H[S.top].toarray()
    Lld, L64 = R.cholesky(Hd.astype(LD)), R.cholesky(Hd)
    want, w64 = R.chol_solve(Lld, E.astype(LD)), R.chol_solve(L64, E)
    fro = lambda a: float(np.sqrt((np.asarray(a, dtype=LD) ** 2).sum()))
    d_inv = fro(w64 - want) / fro(want)
    e_inv = fro(got - want) / fro(want)
    d_res = fro(Hd.astype(LD) @ w64.astype(LD) - E) / fro(E)
    e_res = fro(Hd.astype(LD) @ got.astype(LD) - E) / fro(E)
    print("%s: Ainv device %.2e float64 %.2e (bound %.1e); |H Ainv - I| device %.2e float64 %.2e (bound %.1e)"
          % (_id(case), e_inv, d_inv, R.bound(d_inv), e_res, d_res, R.bound(d_res)))
    assert e_inv <= R.bound(d_inv)
    assert e_res <= R.bound(d_res)
    for seed in (R.B_SEED, R.U_SEED):
        b = S.random(seed)
        x, used = D.V(b)
        assert not used.any()
        xl = R.chol_solve(Lld, b.astype(LD))
        d = R.rel(R.chol_solve(L64, b), xl)
        e = R.rel(x, xl)
        print("%s: V(b) device %.2e float64 %.2e (bound %.1e)" % (_id(case), e, d, R.bound(d)))
        assert e <= R.bound(d)
    D.A.set_pcg(rtol=1e-11, maxit=300)
    x, it, rr, ok = D.cg(S.g)
    assert (it, ok) == (1, True)
    assert rel(x, S.direct(S.g)) < 1e-8


# ---------------------------------------------------------------------------------------------------------------- 4 .. 7: CG
@pytest.mark.parametrize("degree", (1, 2))
@pytest.mark.parametrize("case", R.MULTI, ids=_id)
def test_cg_iterates_match_restatement(M, case, degree):
    """4. maxit = k = 1 .. 4 at rtol = 1e-14: x is the reference's x_k, it == k, not converged (code 3: the cap), relres is
    sqrt(<r_k, V r_k> / <r_0, V r_0>) -- alpha from the MG_PAP epilogue, beta, the update and the order of the stop tests."""
    D = _dev(M, case)
    S = D.S
    r64, rld = S.cg(degree, 1e-14, 4, np.float64), S.cg(degree, 1e-14, 4, LD)
    assert rld.it == 4 and rld.code == 3
    for k in (1, 2, 3, 4):
        D.A.set_pcg(degree=degree, maxit=k, rtol=1e-14)
        x, it, rr, ok = D.cg(S.g)
        dx = R.rel(r64.x[k], rld.x[k])
        dr = abs(r64.relres(k) - rld.relres(k)) / rld.relres(k)
        ex = R.rel(x, rld.x[k])
        er = abs(rr - rld.relres(k)) / rld.relres(k)
        print("%s degree %d k=%d: x_k device %.2e float64 %.2e (bound %.1e); relres device %.2e float64 %.2e (bound %.1e)"
              % (_id(case), degree, k, ex, dx, R.bound(dx), er, dr, R.bound(dr)))
        assert it == k and not ok
        assert ex <= R.bound(dx)
        assert er <= R.bound(dr)


@pytest.mark.parametrize("key", sorted(R.COUNT_CASES), ids=lambda k: "%s-L%d-p%g-degree%d" % k)
def test_cg_iteration_count_matches_restatement(M, key):
    """5. rtol = 1e-11: the device counts the reference's iterations and reaches the direct solution at 1e-8.  The right-hand
    side (COUNT_CASES) makes the reference stop with <r, V r> a factor 4 away from the threshold on either side, asserted here."""
    kind, L, p, degree = key
    D = _dev(M, (kind, L, p))
    S = D.S
    seed = R.COUNT_CASES[key]
    rld = S.cg(degree, R.COUNT_RTOL, 300, LD, seed)
    m = R.count_margins(rld)
    assert rld.code == 1 and m[0] > 4 and m[1] < 0.25
    g = R.count_rhs(S, seed)
    D.A.set_pcg(degree=degree, rtol=R.COUNT_RTOL, maxit=300)
    x, it, rr, ok = D.cg(g)
    print("%s-L%d-p%g degree %d: device %d iterations, reference %d (<r,Vr> / threshold %.2f then %.3f); relres %.2e"
          % (kind, L, p, degree, it, rld.it, m[0], m[1], rr))
    assert ok and it == rld.it
    assert rel(x, S.direct(g)) < 1e-8


@pytest.mark.parametrize("case", [("fem2d", 4, 1.0), ("fem3d", 3, 1.5), ("fem1d", 7, 1.0)], ids=_id)
def test_cg_chunk_and_maxit(M, case):
    """6. chunk 1, 3, 8: the same bits of x, the same it and relres -- the launches enqueued behind `done` move nothing (the
    SpMVs on P and P' ignore the flag: they write z and level vectors only).  maxit = 5 with chunk = 4 stops at 5."""
    D = _dev(M, case)
    S = D.S
    ref = None
    for chunk in (1, 3, 8):
        D.A.set_pcg(rtol=1e-11, maxit=300, chunk=chunk)
        out = D.cg(S.g)
        print("%s chunk %d: %d iterations, relres %.3e, converged %d" % (_id(case), chunk, out[1], out[2], out[3]))
        assert out[3]
        if ref is None:
            ref = out
            assert out[1] % 8 != 0      # launches do ride behind the flag at chunk 8
        assert np.array_equal(out[0], ref[0]) and out[1:] == ref[1:]
    D.A.set_pcg(rtol=1e-14, maxit=5, chunk=4)
    x5, it, rr, ok = D.cg(S.g)
    assert (it, ok) == (5, False)
    D.A.set_pcg(chunk=1)
    x5b, itb, rrb, okb = D.cg(S.g)
    assert np.array_equal(x5, x5b) and (itb, rrb, okb) == (it, rr, ok)
    rld, r64 = S.cg(2, 1e-14, 5, LD), S.cg(2, 1e-14, 5, np.float64)
    assert R.rel(x5, rld.x[5]) <= R.bound(R.rel(r64.x[5], rld.x[5]))


@pytest.mark.parametrize("case", [("fem2d", 4, 1.5), ("fem1d", 6, 1.0)], ids=_id)
def test_cg_stop_codes(M, case):
    """7. g = 0: x = 0 at iteration 0, converged.  One NaN in g: a numeric stop at iteration 0, not converged -- and the next
    call with a finite g gives the bits it gave before."""
    D = _dev(M, case)
    S = D.S
    D.A.set_pcg(rtol=1e-11, maxit=300)
    before = D.cg(S.g)
    assert before[3]
    x, it, rr, ok = D.cg(np.zeros(S.N))
    assert not x.any() and (it, ok) == (0, True)
    g = S.g.copy()
    g[S.N // 2] = np.nan
    x, it, rr, ok = D.cg(g)
    assert (it, ok) == (0, False)
    after = D.cg(S.g)
    assert np.array_equal(after[0], before[0]) and after[1:] == before[1:]
    Vb = D.V(S.g)[0]
    assert np.isfinite(Vb).all()


# ---------------------------------------------------------------------------------------------------------------- 8: fallback
def test_fallback_bookkeeping(M):
    """8. fem2d L=3 p=1 with a CG that cannot converge (maxit = 1, rtol = 1e-14): three systems fall back to the device Cholesky,
    then the solve gives up on CG (giveup = 3) and z is the golden's; with giveup = 0 every system is tried and falls back."""
    gold = np.load(os.path.join(HERE, "golden", "fem2d_L3_p1_0.npz"))
    sol = M.fem2d_mpi_solve(L=3, p=1.0, solver="pcg", pcg=dict(maxit=1, rtol=1e-14, giveup=3))
    pc = sol.SOL_main["pcg"]
    print("giveup 3: %r" % (pc,))
    assert pc["fallbacks"] == 3 and pc["gave_up_at"] == 3
    assert rel(M.mpi_to_native(sol).z, gold["z"]) < ZTOL
    sol = M.fem2d_mpi_solve(L=3, p=1.0, solver="pcg", pcg=dict(maxit=1, rtol=1e-14, giveup=0))
    pc = sol.SOL_main["pcg"]
    print("giveup 0: %r, newton %d" % (pc, int(sol.SOL_main["its"].sum())))
    assert pc["solves"] > 3 and pc["fallbacks"] == pc["solves"] and pc["gave_up_at"] < 0
    assert rel(M.mpi_to_native(sol).z, gold["z"]) < ZTOL
