"""newton_reference.py against the ORACLE's own runs (CPU only): before the restatement judges the device it must reproduce the
code it restates.  oracle.newton / linesearch_backtracking / amgb_step are wrapped here (oracle/ is not edited) to keep what
every line search started from and returned; replay_step must then give the oracle's step length and its number of objective
evaluations at every decisive step, replay_stop its `converged` and k, replay_outer its `its` and `ts`.  The kappa logic, which
no small problem exercises, is checked on scripted centerings against oracle.amgb_core itself."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import barrier_reference as BR
import mgb_oracle as O
import newton_reference as NR

CASES = [("fem1d", 3, 1.0, "fine"), ("fem2d", 2, 1.5, "fine"), ("fem2d", 2, 1.0, "all")]
_runs = {}


def oracle_run(kind, L, p, schedule):
    """The oracle's solve with every newton() call recorded: dict(level, t, final, budget, k, converged, Dz0, c (scaled by t),
    steps = [dict(s, nstep, y, g, inc, sigma, evals, ynext, gnext)])."""
    key = (kind, L, p, schedule)
    if key in _runs:
        return _runs[key]
    go = getattr(O, kind)(L)
    Mo = O.amg(go)
    dim = go.x.shape[1] if go.x.ndim > 1 else 1
    K = len(Mo.D)
    Bar = O.Barrier(O.convex_Euclidian_power(list(range(K - dim - 1, K)), p))
    z0 = O.map_rows(lambda xi: O.DEFAULT_G[dim](xi), Mo.x).reshape(-1, order="F")
    c = O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), Mo.x)
    calls, ctx = [], {}
    orig_ls, orig_newton, orig_step = O.linesearch_backtracking, O.newton, O.amgb_step

    def ls(x, y, g, n, inc, F0, F1, phi=None):
        count = [0]

        def F0c(xx, ref):
            count[0] += 1
            return F0(xx, ref)

        out = orig_ls(x, y, g, n, inc, F0c, F1, phi)
        ctx["steps"].append(dict(s=np.array(x), nstep=np.array(n), y=y, g=float(np.linalg.norm(g)), inc=inc, sigma=out[3],
                                 evals=count[0], ynext=out[1], gnext=float(np.linalg.norm(out[2]))))
        return out

    def newton(F0, F1, F2, x, maxit, crit, log=None):
        J = ctx["levels"].pop(0)
        ctx["steps"] = []
        SOL = orig_newton(F0, F1, F2, x, maxit, crit, log)
        Lr = len(Mo.R)
        # `final` as the device means it (Amg::solve final_at): with centering "exact" every centre is resolved
        calls.append(dict(level=J, t=ctx["t"], final=ctx["final"] or O.CENTERING == "exact", finest=J == Lr - 1, budget=maxit, k=SOL["k"], converged=SOL["converged"],
                          Dz0=ctx["Dz0"], c=ctx["c"], steps=ctx["steps"]))
        ctx["Dz0"] = Bar._Dz(SOL["x"], None, Mo.D, None, (ctx["Dz0"], Mo.BR[J]))       # as amgb_step carries it forward
        return SOL

    def step(B, M, z, Dz0, cc, maxit, lam_tol, log=None, schedule=None, final=True):
        ctx.update(levels=O.level_schedule(len(M.R), schedule), Dz0=np.array(Dz0), c=np.array(cc), final=final,
                   t=float(cc[0, 0] / c[0, 0]))      # c[0, 0] = 1/2: the quotient is t itself
        return orig_step(B, M, z, Dz0, cc, maxit, lam_tol, log, schedule, final)

    O.linesearch_backtracking, O.newton, O.amgb_step = ls, newton, step
    try:
        SOL = O.amgb_core(Bar, Mo, z0, c, math.sqrt(np.finfo(np.float64).eps), schedule=schedule)
    finally:
        O.linesearch_backtracking, O.newton, O.amgb_step = orig_ls, orig_newton, orig_step
    assert c[0, 0] == 0.5
    terms = BR.default_terms(dim, p)
    levels = {l: NR.LevelData(BR.interleave(Mo.BR[l]), K, Mo.w, c, terms) for l in sorted(Mo.BR)}
    _runs[key] = dict(calls=calls, SOL=SOL, levels=levels, Mo=Mo, L=len(Mo.R))
    return _runs[key]


def trace_rows(call, index):
    """The call as rows of the device's trace (AMG.trace): (centering row, step rows).  A step that ended the loop before its
    line search (inc <= 0, a non-finite direction) left no record in the oracle: it is put back with a stand-in inc."""
    rows = []
    ymin = gmin = None
    for st in call["steps"]:
        if ymin is None:
            ymin, gmin = st["y"], st["g"]
        rows.append([index, st["y"], st["g"], ymin, gmin, st["inc"], st["sigma"], st["ynext"], st["gnext"], 0, 0, 0, 0, 0])
        ymin, gmin = min(ymin, st["ynext"]), min(gmin, st["gnext"])
    if call["k"] > len(call["steps"]):
        assert call["k"] == len(call["steps"]) + 1
        last = call["steps"][-1] if call["steps"] else dict(ynext=0.0, gnext=0.0)
        rows.append([index, last["ynext"], last["gnext"], ymin or 0.0, gmin or 0.0, -0.0 if call["converged"] else math.nan, 0.0,
                     last["ynext"], last["gnext"], 0, 0, 0, 0, 0])
    cent = [call["level"], call["t"], call["finest"], call["final"], call["budget"], call["k"], call["converged"], 0, len(rows)]
    return np.array(cent, dtype=np.float64), np.array(rows, dtype=np.float64).reshape(-1, 14)


@pytest.mark.parametrize("kind,L,p,schedule", CASES)
def test_replay_step_reproduces_the_oracles_line_searches(kind, L, p, schedule):
    run = oracle_run(kind, L, p, schedule)
    total = decisive = damped = 0
    for call in run["calls"]:
        lv = run["levels"][call["level"]]
        # the oracle hands newton() the cost already scaled by t
        lvt = NR.LevelData(lv.B, lv.K, lv.w, call["c"], lv.terms)
        for st in call["steps"]:
            R = NR.replay_step(lvt, 1.0, call["Dz0"], st["s"], st["nstep"], st["y"], st["inc"])
            total += 1
            assert st["sigma"] in R.reachable, (call["level"], call["t"], st["sigma"], R.reachable, R.ambiguous)
            if R.decisive:
                decisive += 1
                damped += st["sigma"] < 0.25
                assert R.reachable == {st["sigma"]} and R.sigma == st["sigma"]
                assert R.evals == st["evals"], (call["level"], call["t"], st["sigma"], R.visited, st["evals"])
                # a neighbouring step length is told from the right one
                assert st["sigma"] / 2 not in R.reachable and st["sigma"] * 2 not in R.reachable
    print("%s L=%d p=%g %s: %d steps, %d decisive (%d of them damped below 1/4)" % (kind, L, p, schedule, total, decisive, damped))
    assert total - decisive <= 0.4 * total
    assert damped >= 5


@pytest.mark.parametrize("kind,L,p,schedule", CASES)
def test_replay_stop_and_outer_reproduce_the_oracles_counts(kind, L, p, schedule):
    run = oracle_run(kind, L, p, schedule)
    w_min = float(run["Mo"].w.min())
    cents = []
    for i, call in enumerate(run["calls"]):
        cent, rows = trace_rows(call, i)
        k, converged, reasons, _, _ = NR.replay_stop(cent, rows, w_min)
        assert (k, converged) == (call["k"], call["converged"]), (i, call["level"], call["t"], k, converged, reasons)
        assert all(r == NR.R_NONE for r in reasons[:-1])
        assert (reasons[-1] in (NR.R_INC, NR.R_DECREMENT, NR.R_STAGNATION)) == converged
        cents.append(cent)
    out = NR.replay_outer(np.array(cents), run["L"], schedule_all=schedule == "all")
    assert np.array_equal(out["t"], [c["t"] for c in run["calls"]])
    assert np.array_equal(out["level"], [c["level"] for c in run["calls"]])
    assert np.array_equal(out["its"], run["SOL"]["its"]) and np.array_equal(out["ts"], run["SOL"]["ts"])
    if schedule == "all":      # the coarse levels' decrement rule ended some loop
        assert any(NR.replay_stop(*trace_rows(c, 0), w_min)[2][-1] == NR.R_DECREMENT for c in run["calls"] if not c["finest"])


def test_replay_stop_rules_one_by_one():
    w_min = 1e-3
    row = lambda y, g, inc, yn, gn, pivot=0: [0, y, g, 0, 0, inc, 1.0, yn, gn, pivot, 0, 0, 0, 0]
    cent = lambda finest, final, budget=5: np.array([0, 1.0, finest, final, budget, 0, 0, 0, 0], dtype=np.float64)
    stop = lambda c, rows: NR.replay_stop(c, np.array(rows, dtype=np.float64), w_min)[:3]
    # stagnation: y did not fall below the minimum and |g| is not below theta gmin; theta is 0.1 on the finest level, 0.5 below it
    assert stop(cent(1, 1), [row(1.0, 1.0, 1.0, 0.5, 0.5), row(0.5, 0.5, 1.0, 0.5, 0.06)]) == (2, True, [0, NR.R_STAGNATION])
    assert stop(cent(1, 1), [row(1.0, 1.0, 1.0, 0.5, 0.5), row(0.5, 0.5, 1.0, 0.5, 0.04)])[1] is False
    assert stop(cent(0, 1), [row(1.0, 1.0, 1.0, 0.5, 0.5), row(0.5, 0.5, 1.0, 0.5, 0.26)]) == (2, True, [0, NR.R_STAGNATION])
    assert stop(cent(0, 1), [row(1.0, 1.0, 1.0, 0.5, 0.5), row(0.5, 0.5, 1.0, 0.5, 0.24)])[1] is False
    # the minima run: a rise after a fall is measured against the fall
    assert stop(cent(1, 1), [row(1.0, 1.0, 1.0, 0.2, 1.0), row(0.2, 1.0, 1.0, 0.3, 1.0)]) == (2, True, [0, NR.R_STAGNATION])
    # decrement rule: DECREMENT_FRAC min w on the finest level, sqrt(min w) / 2 below it, never at finest and final
    small_f, small_c = 0.5 * O.DECREMENT_FRAC * w_min, 0.9 * math.sqrt(w_min) / 2
    assert stop(cent(1, 0), [row(1.0, 1.0, small_f, 0.5, 0.5)]) == (1, True, [NR.R_DECREMENT])
    assert stop(cent(1, 1), [row(1.0, 1.0, small_f, 0.5, 0.5)]) == (1, False, [NR.R_NONE])
    assert stop(cent(0, 1), [row(1.0, 1.0, small_c, 0.5, 0.5)]) == (1, True, [NR.R_DECREMENT])
    assert stop(cent(1, 0), [row(1.0, 1.0, small_c, 0.5, 0.5)]) == (1, False, [NR.R_NONE])
    # inc <= 0 converges, a pivot failure and a non-finite decrement end the loop without converging, the budget ends it
    assert stop(cent(1, 1), [row(1.0, 1.0, 0.0, 1.0, 1.0)]) == (1, True, [NR.R_INC])
    assert stop(cent(1, 1), [row(1.0, 1.0, 1.0, 1.0, 1.0, pivot=1)]) == (1, False, [NR.R_PIVOT])
    assert stop(cent(1, 1), [row(1.0, 1.0, math.inf, 1.0, 1.0)]) == (1, False, [NR.R_NONFINITE])
    falling = [row(1.0 - 0.1 * i, 1.0, 1.0, 0.9 - 0.1 * i, 0.5 ** (i + 1)) for i in range(3)]
    assert stop(cent(1, 1, budget=3), falling) == (3, False, [0, 0, NR.R_BUDGET])
    with pytest.raises(AssertionError):
        stop(cent(1, 1, budget=2), falling)


SCRIPTS = {
    "never reduced": [(True, 10)] * 10,
    "first centre takes three budgets": [(False, 48), (False, 48), (True, 20)] + [(True, 10)] * 9,
    "kappa halves twice, grows back after an easy centre": [(True, 10), (False, 48), (False, 48), (True, 30), (True, 12), (True, 12)] + [(True, 12)] * 12,
    "a hard centre keeps kappa down": [(True, 10), (False, 48), (True, 13), (True, 13), (True, 13)] + [(True, 13)] * 30,
    "the last step is clipped at t_stop": [(True, 10), (False, 48), (True, 40)] + [(True, 40)] * 30,
}


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_replay_outer_against_amgb_core_on_scripted_centerings(name, monkeypatch):
    """oracle.amgb_core with amgb_step replaced by a script of (converged, Newton steps): replay_outer must consume the same
    calls at the same t and give the same its and ts."""
    script = list(SCRIPTS[name])
    seen = []
    L = 2

    class Mfake:
        w = np.array([1.0])
        R = [None] * L
        D = [sp.identity(1, format="csr")]

    def step(B, M, z, Dz0, cc, maxit, lam_tol, log=None, schedule=None, final=True):
        ok, k = script[len(seen)]
        seen.append((float(cc[0, 0]), final, ok, k))
        return dict(z=z, Dz0=Dz0, its=np.array([0, k]), converged=ok)

    monkeypatch.setattr(O, "amgb_step", step)
    SOL = O.amgb_core(O.Barrier(None), Mfake, np.zeros(1), np.ones((1, 1)), math.sqrt(np.finfo(np.float64).eps))
    cents = np.array([[L - 1, t, 1, 1, 48, k, ok, 0, 0] for t, final, ok, k in seen], dtype=np.float64)
    out = NR.replay_outer(cents, L)
    assert np.array_equal(out["t"], [s[0] for s in seen]), name
    assert np.array_equal(out["its"], SOL["its"]) and np.array_equal(out["ts"], SOL["ts"]), name
    assert out["converged"] and out["ts"][-1] == max(s[0] for s in seen)
    if "clipped" in name:      # the last t is t_stop itself, not kappa times the one before
        assert out["ts"][-1] < out["kappas"][-1] * out["ts"][-2]
    if "kappa" in name or "hard" in name or "clipped" in name:
        assert (out["kappas"] < 10.0).any()
    if "grows back" in name:
        assert out["kappas"][-1] == 10.0
    if "hard" in name:
        assert (out["kappas"][1:] < 10.0).all()
    # one call too many or too few in the trace is noticed
    with pytest.raises(AssertionError):
        NR.replay_outer(cents[:-1], L)
    with pytest.raises(AssertionError):
        NR.replay_outer(np.vstack([cents, cents[-1:]]), L)
