"""Whole solves on coarse meshes K beyond the default square (tests/mesh_cases.py: the L shape, L shapes graded towards the
re-entrant corner as adapt() produces them, a domain of two components) against the live CPU oracle on the same mesh:
amgb(fem2d_mpi(L, K), p) against mgb_oracle.fem2d_solve(L, K, p) at ZTOL = 1e-10 relative l2, the bound of every whole solve
of test_gpu_parity.py.  The oracle and the device number the continuous unknowns differently, but z is nodal and the two build
the same nodes (test_mesh_cases.py), so z compares directly.

Each case runs with the device Cholesky (solver="gpu": elimination trees of a geometric nested dissection on graded
coordinates), the host Cholesky and, on the graded meshes, solver="pcg": no level of fem2d(L, graded4) has 128 unknowns or
fewer (182 at level 0), so the V-cycle's coarse solve is the device Cholesky instead of the dense inverse
(Amg::mg_coarsest, mg_prepare); test_gpu_vcycle.py holds that V-cycle to its restatement, here it runs inside the Newton loop.
One oracle solve per case is shared by the solver variants.

Measured distances to the oracle (relative l2): solver="gpu" 2.7e-15 .. 8.7e-12, solver="host" 1.3e-13 .. 9.7e-11 -- the
largest is the L shape at L=4, p=1.5 with the host Cholesky, 9.681e-11 in two runs (the device Cholesky on the same mesh:
8.0e-14; both take 105 Newton steps, the oracle 108): the end points are centres converged to the Newton stopping rule, and
this one sits close to the bound."""
import numpy as np
import pytest

import mesh_cases as MC
import mgb_oracle as O
from test_gpu_parity import rel, ZTOL

pytestmark = pytest.mark.gpu

CASES = [("lshape", 3, 1.0), ("lshape", 4, 1.5), ("graded4", 2, 1.5), ("graded4", 3, 1.0), ("two_squares", 3, 1.0)]
PCG_CASES = [("graded4", 2, 1.5), ("graded4", 3, 1.0)]


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_ORACLE = {}


def oracle(mesh, L, p, **kw):
    """the oracle's solve of a case, once per module"""
    key = (mesh, L, p) + tuple(sorted(kw.items()))
    if key not in _ORACLE:
        _ORACLE[key] = O.fem2d_solve(L=L, K=MC.MESHES[mesh], p=p, **kw)
    return _ORACLE[key]


@pytest.mark.parametrize("solver", ["gpu", "host"])
@pytest.mark.parametrize("mesh,L,p", CASES)
def test_solve_matches_live_oracle(M, mesh, L, p, solver):
    so = oracle(mesh, L, p)
    sol = M.amgb(M.fem2d_mpi(L, MC.MESHES[mesh]), p=p, solver=solver)
    z = M.mpi_to_native(sol).z
    err = rel(z, so.z)
    its, oits = int(sol.SOL_main["its"].sum()), int(so.SOL_main["its"].sum())
    print("%s L=%d p=%g solver=%s: %d rows, newton %d (oracle %d), rel l2 to the oracle %.3e" % (mesh, L, p, solver, z.shape[0], its,
                                                                                             oits, err))
    assert z.shape == so.z.shape == (7 * MC.TRIANGLES[mesh] * 4 ** (L - 1), 2)
    assert err < ZTOL
    assert abs(its - oits) <= max(3, 0.25 * oits)      # test_solve_matches_oracle_and_golden's rule for the step counts


@pytest.mark.parametrize("mesh,L,p", PCG_CASES)
def test_pcg_solve_with_the_cholesky_coarse_solve_matches_live_oracle(M, mesh, L, p):
    """solver="pcg" where the V-cycle's coarsest level is level 0 with more than 128 unknowns: the device Cholesky is the coarse
    solve of every V-cycle of the Newton loop.  CG must have solved systems itself (a solve that fell back to the direct solver
    every time would reach the oracle's z without the V-cycle).  Measured: graded4 L=2 p=1.5: 91 Newton systems, 45 given to
    CG, 3 fallbacks (then the solve gives up on CG): share 0.462, z at 9.3e-15 of the oracle's; graded4 L=3 p=1: 245 systems, 39
    given to CG, 3 fallbacks: share 0.147, z at 1.4e-13."""
    so = oracle(mesh, L, p)
    g = M.fem2d_mpi(L, MC.MESHES[mesh])
    A = M.AMG(g, p=p)
    assert A.mg_coarsest(L - 1) == 0 and A.level_size(0)[0] == MC.LEVEL_SIZES[("graded4", 3)][0] > 128      # 182 unknowns
    sol = M.amgb(g, p=p, solver="pcg")
    z = M.mpi_to_native(sol).z
    pc = sol.SOL_main["pcg"]
    newton = int(sol.SOL_main["its"].sum())
    share = (pc["solves"] - pc["fallbacks"]) / max(newton, 1)
    print("%s L=%d p=%g pcg: newton %d, systems given to CG %d, fallbacks %d, gave up at %d, CG iterations %d (%.1f per system); "
          "share of the Newton systems CG solved %.3f; rel l2 to the oracle %.3e"
          % (mesh, L, p, newton, pc["solves"], pc["fallbacks"], pc["gave_up_at"], pc["iterations"],
             pc["iterations"] / max(pc["solves"], 1), share, rel(z, so.z)))
    assert rel(z, so.z) < ZTOL
    assert pc["solves"] > pc["fallbacks"] and share > 0.0


def test_level_loop_schedule_on_the_l_shape_matches_oracle(M):
    """schedule="all" (the literal coarse -> fine level loop) on the L shape against the oracle with the same schedule."""
    mesh, L, p = "lshape", 3, 1.0
    so = oracle(mesh, L, p, schedule="all")
    sol = M.amgb(M.fem2d_mpi(L, MC.MESHES[mesh]), p=p, schedule="all")
    z = M.mpi_to_native(sol).z
    its = sol.SOL_main["its"]
    print("lshape L=3 p=1 schedule=all: newton %d (oracle %d), rel l2 %.3e" % (int(its.sum()), int(so.SOL_main["its"].sum()), rel(z, so.z)))
    assert rel(z, so.z) < ZTOL
    assert its.shape[0] == L and np.all(its.sum(axis=1) > 0)                  # every level visited
    assert abs(int(its.sum()) - int(so.SOL_main["its"].sum())) <= max(3, 0.25 * so.SOL_main["its"].sum())
    assert rel(z, oracle(mesh, L, p).z) < 1e-9                                # and the default schedule's end point


def test_parabolic_on_the_l_shape_matches_oracle(M):
    """parabolic_solve on fem2d_mpi(2, lshape), h = 0.5, p = 2 against the oracle's loop, snapshot by snapshot: the bounds of
    test_gpu_parabolic.py::test_parabolic_matches_oracle."""
    K = MC.MESHES["lshape"]
    g = M.fem2d_mpi(2, K)
    sol = M.parabolic_solve(g, h=0.5, t1=1.0, p=2.0, verbose=False)
    nat = M.mpi_to_native(sol)
    ref = O.parabolic_solve(O.fem2d(2, K), h=0.5, t1=1.0, p=2.0)
    assert np.array_equal(nat.ts, ref.ts) and len(nat.u) == len(ref.u) >= 2
    for k, (uk, rk) in enumerate(zip(nat.u, ref.u)):
        assert uk.shape == rk.shape
        print("parabolic lshape L=2 h=0.5 p=2 snapshot %d: u %.3e, all columns %.3e" % (k, rel(uk[:, 0], rk[:, 0]), rel(uk, rk)))
        assert rel(uk[:, 0], rk[:, 0]) < 1e-10
        assert rel(uk, rk) < 1e-8
