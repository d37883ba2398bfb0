"""The Newton loop step by step (csrc/amg.cpp: Amg::newton, dev_f2_solve, launch_step_graph, amgb_step, solve) through the
trace of AMG.set_trace, against tests/newton_reference.py.  Run with -m gpu -s on an MI355X; profiles/newton_trace_margins.txt
is the output of such a run.

exact tier (every step of every small case, with vectors)
  start      y and |g| before the first step of every newton() call are the exact values at s = 0 within the bounds of the
             objective sums and of the gradient's SpMV.  (That y and |g| before step k + 1 are bitwise those after step k, and
             that ymin / gmin are the running minima, is asserted too, but holds by construction of the trace -- the same host
             variables -- and guards the record's own bookkeeping, not the loop.)
  rotation   the traced accepted s is s_k - sigma nstep to (|sigma nstep| + |s_k|) u per entry (bitwise s_k when rejected) and
             the traced accepted Dz is Dz0 + B s within the SpMV bound: the buffers the next step reads are the accepted
             trial's, whichever slot held it
  decision   the traced sigma is among the lengths newton_reference.replay_step can reach; at decisive steps it is the one
             length, and the objective evaluations launched are the path's minus the speculated points consumed
  stop       reason, k and `converged` are newton_reference.replay_stop's; the t of every newton() call, its and ts are
             newton_reference.replay_outer's
  direction  inc = <g, n> against the exact inc_ref (newton_reference.reference_direction), STEP BY STEP: the device's relative
             error at a step against INC_FACTOR = 16 times the larger of the fp64 oracle step's error at that step (oracle f1,
             f2 and splu on the same matrices at the same point) and a floor, the first-order effect on inc of the fp64 bounds
             of g and H alone (U (2 b_g' |n| + |n|' b_H |n|) / |inc_ref|), below which no fp64 step can be asked to stay.  16:
             the device's sums run in another order, a multifrontal elimination order replaces LU's, and both errors scale
             with the same cond(H).  At the last steps of a centering the gradient is at rounding level and floor and
             yardstick are of order one; two thirds of a case's steps must allow less than 0.1, so an inc off by a factor or
             a sign fails there

so that the exact tier cannot pass by calling everything ambiguous: at most 40 % of a case's steps are ambiguous, at least 10
decisive steps are damped below 1/4 (beyond the three speculated points: the slot-swapping evaluations run) and at least one
decisive step is served from speculation alone.

bitwise tier (trace scalars and z as bytes)
  (a) kernel timing on (sampled plain launches, timed chain, graphs) against off (graphs only); the mode column shows that
      each mode ran     (b) tracing with vectors, without vectors, off: z, its, c_dot_Dz     (c) a second solve on the same
  handle from the same start (its graphs replayed through rotated buffers)     (d) MGB_CHOL_GRAPH=0 in one fresh child process
  (e) solver = host and solver = pcg are not bitwise: their traces pass the decision and stop checks and name their own modes

stale state   one handle solved with scalar p = 1.5, then given p(x) (mgb_amg_set_exponents) or a term mask
  (mgb_amg_set_term_mask), set back to the start and solved again: trace and z bitwise those of a fresh handle that had them
  before its first solve.  Before set_exponents / set_term_mask dropped the captured step graphs, the replayed graphs evaluated
  the speculated trials with the old exponents and mask (BarrierParams is baked into the kernel arguments by value).

Measured on an MI355X (profiles/newton_trace_margins.txt has the whole run).  inc, per step: steps that allow less than 0.1,
the worst device and oracle errors among them, the worst device error over its allowance; then the steps at rounding level:

  fem1d L=4 p=1     76 of 93 tight: device 6.72e-07, oracle 6.72e-07, device / allowed 0.001     17 loose: device 3.3e-01, oracle 3.3e-01
  fem2d L=3 p=1     80 of 91 tight: device 8.53e-07, oracle 1.43e-06, device / allowed 0.001     11 loose: device 7.0e-02, oracle 2.5e-01
  fem2d L=3 p=1.5   73 of 86 tight: device 1.36e-06, oracle 8.72e-07, device / allowed 0.005     13 loose: device 3.8e-01, oracle 3.7e-01
  fem2d L=3 p=2     75 of 83 tight: device 1.16e-04, oracle 9.63e-05, device / allowed 0.002      8 loose: device 3.6e-01, oracle 2.4e-01
  fem3d L=2 p=1     74 of 89 tight: device 1.26e-06, oracle 5.68e-07, device / allowed 0.000     15 loose: device 1.9e-01, oracle 3.2e-01

At every step the floor is above the oracle's own error (the any-order bounds of g and H are worst cases), so the floor is
what the allowance comes from; against the oracle's error alone the device is up to 620 times off at single steps where the
oracle happens to be nearly exact, which is why the floor is there.  Ambiguous steps: 30, 29, 26, 27, 30 % (10 % with
schedule "all").

Without the two drop_step_graphs() calls (one run, the library built with them disabled) both stale-state tests FAIL, with
wrong values and no fault: after set_exponents the used handle takes 101 Newton steps where the fresh one takes 87, after
set_term_mask 121 against 86; z ends 3.9e-15 and 2.6e-14 away -- the stale trials cost steps, not accuracy, which is why no
end-point test saw it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import barrier_reference as BR
import chol_reference as CR
import linesearch_reference as LR
import mgb_oracle as O
import newton_reference as NR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
U, MARGIN, LD = NR.U, NR.MARGIN, NR.LD
INC_FACTOR = 16.0
TIGHT, TIGHT_SHARE = 0.1, 2.0 / 3.0      # the direction check: this share of a case's steps must allow a relative error below TIGHT
MAX_STEPS = 4000
SMALL = [("fem1d", 4, 1.0, "fine"), ("fem2d", 3, 1.0, "fine"), ("fem2d", 3, 1.5, "fine"), ("fem2d", 3, 2.0, "fine"),
         ("fem3d", 2, 1.0, "fine"), ("fem2d", 3, 1.5, "all")]
BITWISE = SMALL[:5] + [("fem2d", 5, 1.5, "fine")]
IDS = lambda cs: ["%s L=%d p=%g %s" % c for c in cs]
NOMODE = [i for i in range(14) if i != NR.S_MODE]
PFUN = lambda x: 1.6 + 0.5 * x[0]                                            # test_x_dependent_exponent_matches_oracle
OBST_G = lambda x: np.array([0.3 + 0.5 * (x[0] ** 2 + x[1] ** 2), 100.0])    # test_piecewise_set_matches_oracle
OBST_F = lambda x: np.array([5.0, 0.0, 0.0, 1.0])
SELECT = lambda x: (True, x[0] > 0.0)


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


def start(M, kind, L, p, g=None, f=None, **kw):
    gm = getattr(M, kind + "_mpi")(L)
    dim = gm.discretization["dim"]
    x = gm.x.to_numpy()
    A = M.AMG(gm, p=p, **kw)
    z0 = O.map_rows(g or O.DEFAULT_G[dim], x).reshape(-1, order="F")
    c = O.map_rows(f or O.DEFAULT_F[dim], x)
    A.set_c(c)
    A.set_z(z0)
    return gm, A, z0, c


def solved(M, case, trace=(MAX_STEPS, False), time_kernels=True, solver="gpu"):
    kind, L, p, schedule = case
    gm, A, z0, c = start(M, kind, L, p)
    if trace:
        A.set_trace(*trace)
    A.set_time_kernels(time_kernels)
    sol = A.solve(schedule=schedule, solver=solver)
    return dict(A=A, gm=gm, z0=z0, c=c, sol=sol, z=A.get_z(), trace=A.trace() if trace else None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def same_trace(a, b):
    return same_bits(a["centerings"], b["centerings"]) and same_bits(a["steps"][:, NOMODE], b["steps"][:, NOMODE])


def modes(tr):
    return np.bincount(tr["steps"][:, NR.S_MODE].astype(int), minlength=9)


def library_B(M, gm, A, l):
    """B = D R of level l as the library forms it (test_gpu_linesearch.py library_B: its own sparse product)."""
    ops = {k: v.host for k, v in gm.operators.items()}
    subs = {k: [m.host for m in v] for k, v in gm.subspaces.items()}
    Dfull, _ = BR.level_matrices(ops, subs, A.state_variables, A.D, l, A.n)
    R = sp.csr_matrix(sp.block_diag([subs[sv[1]][l] for sv in A.state_variables], format="csr"))
    return (M.HPCSparseMatrix(Dfull) @ M.HPCSparseMatrix(R)).host


# ---------------------------------------------------------------------------------------------------------- the exact tier
_cases = {}


def replayed(M, case, solver="gpu"):
    """Solved once with vectors and replayed once: per step its StepReplay, per centering replay_stop, replay_outer."""
    key = (case, solver)
    if key in _cases:
        return _cases[key]
    kind, L, p, schedule = case
    run = solved(M, case, trace=(MAX_STEPS, True), solver=solver)
    A, gm, tr = run["A"], run["gm"], run["trace"]
    dim = gm.discretization["dim"]
    w = gm.w.to_numpy()
    terms = BR.default_terms(dim, p)
    cent, steps = tr["centerings"], tr["steps"]
    run["levels"] = {l: NR.LevelData(library_B(M, gm, A, l), A.K, w, run["c"], terms, depth=LR.depth_trial(A.n))
                     for l in sorted({int(c[NR.C_LEVEL]) for c in cent})}
    run["replay"] = [None] * len(steps)
    run["stop"] = []
    for ci, ce in enumerate(cent):
        f, ns = int(ce[NR.C_FIRST]), int(ce[NR.C_STEPS])
        lv = run["levels"][int(ce[NR.C_LEVEL])]
        run["stop"].append(NR.replay_stop(ce, steps[f:f + ns], float(w.min())))
        for i in range(f, f + ns):
            if steps[i, NR.S_REASON] in (NR.R_INC, NR.R_PIVOT, NR.R_NONFINITE):
                continue      # no line search ran
            run["replay"][i] = NR.replay_step(lv, ce[NR.C_T], tr["Dz0"][ci], tr["s"][i], tr["nstep"][i], steps[i, NR.S_Y], steps[i, NR.S_INC])
    run["outer"] = NR.replay_outer(cent, A.L, schedule_all=schedule == "all")
    _cases[key] = run
    return run


def centering_of(run, i):
    ci = int(run["trace"]["steps"][i, NR.S_CENT])
    return ci, run["trace"]["centerings"][ci]


@pytest.mark.parametrize("case", SMALL, ids=IDS(SMALL))
def test_values_chain_from_step_to_step_and_start_exact(M, case):
    run = replayed(M, case)
    tr = run["trace"]
    cent, steps = tr["centerings"], tr["steps"]
    assert len(steps) >= 80 and np.isfinite(steps[:, [NR.S_Y, NR.S_G, NR.S_YNEXT, NR.S_GNEXT]]).all()
    for ci, ce in enumerate(cent):
        f, ns = int(ce[NR.C_FIRST]), int(ce[NR.C_STEPS])
        assert ns == ce[NR.C_K] >= 1
        assert same_bits(steps[f + 1:f + ns, [NR.S_Y, NR.S_G]], steps[f:f + ns - 1, [NR.S_YNEXT, NR.S_GNEXT]])
        assert (steps[f:f + ns, NR.S_CENT] == ci).all()
        assert not tr["s"][f].any()      # every newton() starts from s = 0
        lv = run["levels"][int(ce[NR.C_LEVEL])]
        P = NR.evaluate(lv, ce[NR.C_T], tr["Dz0"][ci], np.zeros(lv.N))
        assert abs(float(LD(steps[f, NR.S_Y]) - P.y)) <= MARGIN * U * P.by, (case, ci, steps[f, NR.S_Y], float(P.y))
        Lv = BR.level_reference(lv.B, lv.K, lv.w, lv.c, ce[NR.C_T], tr["Dz0"][ci], lv.terms, hessian=False)
        gn = float(np.sqrt((Lv.g * Lv.g).sum()))
        # | |g + e| - |g| | <= |e| <= |b_g| u; the N squares summed in any order and the root: (N + 2) u |g|
        tol = MARGIN * U * (float(np.linalg.norm(Lv.b_g)) + (lv.N + 2) * gn)
        assert abs(steps[f, NR.S_G] - gn) <= tol, (case, ci, steps[f, NR.S_G], gn, tol)


@pytest.mark.parametrize("case", SMALL, ids=IDS(SMALL))
def test_accepted_buffers_are_the_accepted_trial(M, case):
    run = replayed(M, case)
    tr = run["trace"]
    steps = tr["steps"]
    worst_s = worst_dz = 0.0
    for i, row in enumerate(steps):
        ci, ce = centering_of(run, i)
        lv = run["levels"][int(ce[NR.C_LEVEL])]
        s, n, sn, sigma = tr["s"][i], tr["nstep"][i], tr["s_next"][i], row[NR.S_STEP]
        if i > int(ce[NR.C_FIRST]):
            assert same_bits(s, tr["s_next"][i - 1])
        if sigma == 0.0:
            assert same_bits(sn, s) and same_bits(tr["Dz_next"][i], tr["Dz_next"][i - 1] if i > int(ce[NR.C_FIRST]) else tr["Dz0"][ci])
            continue
        step = LD(sigma) * n.astype(LD)
        x = s.astype(LD) - step
        worst_s = max(worst_s, BR.ratio(sn, x, np.abs(step) + np.abs(x)))
        bs, bb = BR.spmv_reference(lv.B, sn)
        dz = tr["Dz0"][ci].reshape(-1).astype(LD) + bs
        worst_dz = max(worst_dz, BR.ratio(tr["Dz_next"][i].reshape(-1), dz, bb + np.abs(np.asarray(dz, dtype=np.float64))))
    print("%s: accepted s %.2f u-bounds, accepted Dz %.2f SpMV bounds" % (IDS([case])[0], worst_s, worst_dz))
    assert worst_s <= 1.0 and worst_dz <= MARGIN


def check_decisions(run, label):
    steps = run["trace"]["steps"]
    amb = damped = spec = searched = 0
    for i, (row, R) in enumerate(zip(steps, run["replay"])):
        if R is None:
            assert row[NR.S_STEP] == 0.0
            continue
        searched += 1
        sigma = row[NR.S_STEP]
        assert sigma in R.reachable, (label, i, sigma, sorted(R.reachable), R.ambiguous)
        if not R.decisive:
            amb += 1
            continue
        assert R.reachable == {sigma}
        damped += sigma < 0.25
        if row[NR.S_MODE] != 6:      # the host solver speculates nothing
            used = bin(int(row[NR.S_CONSUMED])).count("1")
            assert row[NR.S_EVALS] == R.evals - used, (label, i, sigma, R.visited, row[NR.S_EVALS], row[NR.S_CONSUMED])
            assert int(row[NR.S_CONSUMED]) == sum(1 << k for k in R.visited if k <= 2)      # steps 1, 1/2, 1/4 are speculated at these sizes
            spec += row[NR.S_EVALS] == 0 and used > 0
        else:
            assert row[NR.S_EVALS] == R.evals and row[NR.S_CONSUMED] == 0
    print("%s: %d steps, %d ambiguous (%.0f %%), %d decisive damped below 1/4, %d decisive from speculation alone" % (
        label, len(steps), amb, 100.0 * amb / len(steps), damped, spec))
    return amb, damped, spec


def check_stops(run, label):
    tr = run["trace"]
    cent, steps = tr["centerings"], tr["steps"]
    for ci, (ce, (k, converged, reasons, ymins, gmins)) in enumerate(zip(cent, run["stop"])):
        f, ns = int(ce[NR.C_FIRST]), int(ce[NR.C_STEPS])
        assert (k, converged) == (int(ce[NR.C_K]), bool(ce[NR.C_CONVERGED])), (label, ci)
        assert reasons == [int(r) for r in steps[f:f + ns, NR.S_REASON]], (label, ci)
        assert same_bits(ymins, steps[f:f + ns, NR.S_YMIN]) and same_bits(gmins, steps[f:f + ns, NR.S_GMIN]), (label, ci)
    out = run["outer"]
    assert same_bits(out["t"], cent[:, NR.C_T]) and np.array_equal(out["level"], cent[:, NR.C_LEVEL])
    assert np.array_equal(out["final"], cent[:, NR.C_FINAL] != 0)
    assert np.array_equal(out["its"], run["sol"]["its"]) and same_bits(out["ts"], run["sol"]["ts"])
    assert out["converged"]


@pytest.mark.parametrize("case", SMALL, ids=IDS(SMALL))
def test_every_step_length_is_reachable_and_decisive_ones_are_exact(M, case):
    run = replayed(M, case)
    amb, damped, spec = check_decisions(run, IDS([case])[0])
    assert amb <= 0.4 * len(run["trace"]["steps"])
    assert damped >= 10 and spec >= 1


@pytest.mark.parametrize("case", SMALL, ids=IDS(SMALL))
def test_stop_reasons_counts_and_continuation(M, case):
    run = replayed(M, case)
    check_stops(run, IDS([case])[0])
    if case[3] == "all":      # the coarse levels' theta and decrement rule ran
        cent, steps = run["trace"]["centerings"], run["trace"]["steps"]
        coarse = cent[:, NR.C_FINEST] == 0
        assert coarse.any() and (cent[coarse, NR.C_CONVERGED] == 1).any()
        last = (cent[coarse, NR.C_FIRST] + cent[coarse, NR.C_STEPS] - 1).astype(int)
        assert (steps[last, NR.S_REASON] == NR.R_DECREMENT).any()


@pytest.mark.parametrize("case", SMALL[:5], ids=IDS(SMALL[:5]))
def test_decrement_against_the_exact_direction(M, case):
    """Step by step: the device's relative error of inc against INC_FACTOR times the larger of the oracle's error AT THE SAME
    STEP and the floor of newton_reference.reference_direction (what the fp64 bounds of g and H alone do to inc).  At the last
    steps of a centering the gradient is at rounding level, floor and yardstick are of order one and the check says nothing;
    TIGHT_SHARE of the steps must allow less than TIGHT, so that an inc off by a factor or a sign fails at most steps."""
    run = replayed(M, case)
    tr = run["trace"]
    steps = tr["steps"]
    rows, failures = [], []
    for i, row in enumerate(steps):
        ci, ce = centering_of(run, i)
        lv = run["levels"][int(ce[NR.C_LEVEL])]
        Dz = tr["Dz0"][ci] if i == int(ce[NR.C_FIRST]) else tr["Dz_next"][i - 1]
        _, _, inc_ref, floor = NR.reference_direction(lv, ce[NR.C_T], Dz)
        inc_o = NR.oracle_direction(lv, ce[NR.C_T], Dz)
        yard = float(abs(LD(inc_o) - inc_ref) / abs(inc_ref))
        dev = float(abs(LD(row[NR.S_INC]) - inc_ref) / abs(inc_ref))
        allowed = INC_FACTOR * max(yard, floor)
        rows.append((yard, floor, dev, allowed))
        if not dev <= allowed:
            failures.append((i, row[NR.S_INC], float(inc_ref), dev, yard, floor))
    r = np.array(rows)
    tight = r[:, 3] < TIGHT
    print("%s: inc against inc_ref over %d steps: %d steps allow less than %g (worst device error there %.2e, oracle %.2e, worst device / "
          "allowed %.3f); the other %d (gradient at rounding level): worst device error %.2e, oracle %.2e; worst device / allowed "
          "over all steps %.3f, worst device / oracle error %.1f" % (
              IDS([case])[0], len(r), tight.sum(), TIGHT, r[tight, 2].max(), r[tight, 0].max(), (r[tight, 2] / r[tight, 3]).max(),
              (~tight).sum(), r[~tight, 2].max() if (~tight).any() else 0.0, r[~tight, 0].max() if (~tight).any() else 0.0,
              (r[:, 2] / r[:, 3]).max(), (r[:, 2] / r[:, 0]).max()))
    assert not failures, failures
    assert tight.sum() >= TIGHT_SHARE * len(r)


# ---------------------------------------------------------------------------------------------------------- the bitwise tier
@pytest.mark.parametrize("case", BITWISE, ids=IDS(BITWISE))
def test_launch_modes_tracing_and_replayed_graphs_are_bitwise(M, case):
    on = solved(M, case)
    off = solved(M, case, time_kernels=False)
    m_on, m_off = modes(on["trace"]), modes(off["trace"])
    print("%s: modes with timing %s, without %s" % (IDS([case])[0], m_on.tolist(), m_off.tolist()))
    assert m_on[0] > 0 and m_on[1] > 0 and m_on[2] > 0 and m_on[3] > 0, "(a) graph replay, capture, sampled and timed chain all ran"
    assert m_off[2] == 0 and m_off[3] == 0 and m_off[0] + m_off[1] + m_off[8] == len(off["trace"]["steps"]) and m_off[8] <= off["A"].L
    assert same_trace(on["trace"], off["trace"]) and same_bits(on["z"], off["z"]), "(a)"
    vec = solved(M, case, trace=(MAX_STEPS, True))
    none = solved(M, case, trace=None)
    assert same_trace(on["trace"], vec["trace"]) and same_bits(on["trace"]["steps"], vec["trace"]["steps"]), "(b)"
    for other in (vec, none):
        assert same_bits(on["z"], other["z"]) and np.array_equal(on["sol"]["its"], other["sol"]["its"]), "(b)"
        assert same_bits(on["sol"]["c_dot_Dz"], other["sol"]["c_dot_Dz"]) and same_bits(on["sol"]["ts"], other["sol"]["ts"]), "(b)"
    A = on["A"]
    A.set_z(on["z0"])
    sol2 = A.solve(schedule=case[3])
    tr2 = A.trace()
    assert same_trace(on["trace"], tr2) and same_bits(on["z"], A.get_z()) and np.array_equal(on["sol"]["its"], sol2["its"]), "(c)"
    assert modes(tr2)[1] < m_on[1], "(c) the second solve replays graphs of the first"


CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/oracle", sys.argv[2]]
import numpy as np
import mgb_amd as M
import test_gpu_newton_trace as T
case = (sys.argv[3], int(sys.argv[4]), float(sys.argv[5]), sys.argv[6])
run = T.solved(M, case)
np.savez(sys.argv[7], centerings=run["trace"]["centerings"], steps=run["trace"]["steps"], z=run["z"])
"""


_CRASHED = []      # a child that died of a signal or ran into its time limit: nothing further is started on the GPU


@pytest.fixture(autouse=True)
def _nothing_after_a_crashed_child():
    if _CRASHED:
        pytest.fail("not started: the child process ended abnormally (%s)" % _CRASHED[0])


def test_chain_without_its_graph_in_a_child_process_is_bitwise(M, tmp_path):
    case = ("fem2d", 3, 1.5, "fine")
    here = solved(M, case)
    out = str(tmp_path / "child.npz")
    cmd = [sys.executable, "-c", CHILD, ROOT, HERE, case[0], str(case[1]), str(case[2]), case[3], out]
    try:
        r = subprocess.run(cmd, env=CR.child_env(os.environ, "GRAPH=0"), timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CRASHED.append("MGB_CHOL_GRAPH=0 child: time limit")
        raise
    if r.returncode < 0:
        _CRASHED.append("MGB_CHOL_GRAPH=0 child: signal %d" % -r.returncode)
    assert r.returncode == 0, "child: exit %d\n%s" % (r.returncode, r.stderr[-3000:])
    got = np.load(out)
    m = np.bincount(got["steps"][:, NR.S_MODE].astype(int), minlength=9)
    assert m[0] == 0 and m[1] == 0 and m[8] > 0, "the child ran no step graph"
    assert same_trace(here["trace"], dict(centerings=got["centerings"], steps=got["steps"])) and same_bits(here["z"], got["z"])


@pytest.mark.parametrize("solver,own", [("host", (6,)), ("pcg", (4, 5))])
def test_other_solvers_pass_the_decision_and_stop_checks(M, solver, own):
    case = ("fem2d", 3, 1.5, "fine")
    run = replayed(M, case, solver=solver)
    m = modes(run["trace"])
    print("solver %s: modes %s" % (solver, m.tolist()))
    assert sum(m[list(own)]) > 0 and (solver != "host" or m[6] == len(run["trace"]["steps"]))
    amb, damped, spec = check_decisions(run, "solver " + solver)
    assert amb <= 0.4 * len(run["trace"]["steps"]) and damped >= 10
    check_stops(run, "solver " + solver)
    gpu = replayed(M, case)
    assert np.abs(run["z"] - gpu["z"]).max() <= 1e-10 * np.abs(gpu["z"]).max()


# ---------------------------------------------------------------------------------------------------------- stale state
def assert_no_graph_survived(M, used, fresh):
    """The used handle's second solve launched exactly as the fresh handle's first: every graph captured anew, none of the
    first solve's replayed.  That there were graphs to go stale is part (c) of the bitwise tier: a second solve on a handle
    whose parameters did not change captures fewer graphs than the first, i.e. it replays the first one's."""
    assert np.array_equal(used["steps"][:, NR.S_MODE], fresh["steps"][:, NR.S_MODE])
    assert modes(used)[1] == modes(fresh)[1] > 0


def test_exponents_set_after_a_solve_reach_the_replayed_graphs(M):
    gm, A, z0, c = start(M, "fem2d", 3, 1.5)
    pn = np.array([PFUN(xi) for xi in gm.x.to_numpy()])
    A.set_trace(MAX_STEPS, False)
    A.solve()
    assert modes(A.trace())[1] > 0
    A.set_exponents(0, pn)
    A.set_z(z0)
    A.solve()
    used, z_used = A.trace(), A.get_z()
    _, F, _, _ = start(M, "fem2d", 3, 1.0, cones=[([1, 2, 3], PFUN)])
    F.set_trace(MAX_STEPS, False)
    F.solve()
    fresh, z_fresh = F.trace(), F.get_z()
    assert same_trace(used, fresh) and same_bits(z_used, z_fresh), "used handle: %d steps, fresh handle: %d steps, max |z - z_fresh| %.3e" % (
        len(used["steps"]), len(fresh["steps"]), np.abs(z_used - z_fresh).max())
    assert_no_graph_survived(M, used, fresh)


def test_term_mask_set_after_a_solve_reaches_the_replayed_graphs(M):
    p, psi = 2.0, 0.2       # a case of test_piecewise_set_matches_oracle
    cones = [([1, 2, 3], p), ("linear", [0], [1.0], -psi)]
    gm, A, z0, c = start(M, "fem2d", 3, p, g=OBST_G, f=OBST_F, cones=cones)
    mask = np.array([SELECT(xi) for xi in gm.x.to_numpy()], dtype=np.uint8)
    A.set_trace(MAX_STEPS, False)
    A.solve()
    assert modes(A.trace())[1] > 0
    A.set_term_mask(mask)
    A.set_z(z0)
    A.solve()
    used, z_used = A.trace(), A.get_z()
    _, F, _, _ = start(M, "fem2d", 3, p, g=OBST_G, f=OBST_F, cones=cones, select=SELECT)
    F.set_trace(MAX_STEPS, False)
    F.solve()
    fresh, z_fresh = F.trace(), F.get_z()
    assert same_trace(used, fresh) and same_bits(z_used, z_fresh), "used handle: %d steps, fresh handle: %d steps, max |z - z_fresh| %.3e" % (
        len(used["steps"]), len(fresh["steps"]), np.abs(z_used - z_fresh).max())
    assert_no_graph_survived(M, used, fresh)


def test_trace_limits_are_argument_errors(M):
    gm, A, z0, c = start(M, "fem2d", 3, 1.5)
    A.set_trace(10, False)
    with pytest.raises(M.MGBError) as e:
        A.solve()
    assert e.value.code == -1 and len(A.trace()["steps"]) == 0       # below one Newton budget: refused before the first step
    A.set_trace(60, True)
    A.set_z(z0)
    with pytest.raises(M.MGBError) as e:
        A.solve()
    part = A.trace()      # partial, and consistent: the interrupted newton() call owns the steps it recorded
    assert e.value.code == -1 and len(part["steps"]) == 60
    assert part["centerings"][:, NR.C_STEPS].sum() == 60 and np.array_equal(part["centerings"][:, NR.C_K], part["centerings"][:, NR.C_STEPS])
    assert len(part["Dz0"]) == len(part["centerings"]) and all(len(part[k]) == 60 for k in ("s", "nstep", "s_next", "Dz_next"))
    A.set_trace(0, False)
    A.set_z(z0)
    A.solve()
    assert len(A.trace()["steps"]) == 0
    ref = solved(M, ("fem2d", 3, 1.5, "fine"), trace=None)
    assert same_bits(A.get_z(), ref["z"])
