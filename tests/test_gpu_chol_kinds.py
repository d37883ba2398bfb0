"""Every launch kind of the device multifrontal Cholesky (csrc/gpuchol.hip) against a refined reference solve.

For each workload of chol_reference.CASES and each knob setting (variant) that forces a launch kind, a fresh child process
(the knobs are read once per process) solves, through solve_linear(..., solver="gpu"), four matrices on the level's
pattern with two right-hand sides each: (a) random SPD, (b) (a) badly scaled, (c) the Newton Hessian at the start, (d) the
Hessian at the end of a finished solve (Newton systems solved by the host Cholesky, so that no matrix under test depends on
the device solver).  Per case:

  * coverage: the launch kinds AMG.chol_schedule() reports contain the kinds the variant is meant to force;
  * reference: eta <= 16 max(eta_baseline, u) and phi <= 16 max(phi_baseline, u) against chol_reference.Reference (phi
    only where the refined reference is exact; that must hold for (a), (b), (c));
  * bitwise: the variants DESIGN.md section 4b calls bitwise the same (chol_reference.BITWISE) give the default's solution.

The two largest sizes (fem2d L=8, fem3d L=4) get matrix (a) with the eta check alone, eta <= 16 u.  The replay test
(chol_reference.REPLAY; on graded4 the fronts hit include ones with a Step launch and one solved by Bwd1024) solves in one
process, through the same captured chain, (a), (c), a series of copies of (a) with one diagonal entry set to -1 (the first non-positive pivot is then that unknown's, in a front of every tree height, own columns 0, 31, 32 and
ns - 1: MGB_E_NUMERIC each time), and (a) again, which must be bitwise the first solution.

Besides the default interval, square and cube, five workloads run on coarse meshes of tests/mesh_cases.py (the key of a
workload is (kind, L, mesh)): fem2d L=4 and L=3 on graded4, L=4 on graded7, L=5 on the L shape, L=4 on two squares.  The
nested dissection cuts between distinct coordinate values, so a graded mesh gives a tree unlike the square's: at 11 522 and
18 434 unknowns the default schedule holds Step, Panel2 / Update2, BwdRect, Bwd256 and Bwd1024 (on the square only fem2d L=8
or forced knobs reach them, where the reference is eta alone), no Leaf launch, and a backward sweep of Bwd1024, BwdRect and
Bwd256 heights above the fused launch.  The two squares give a root without own columns or rows: its Start launch has no
job and is passed over.

The output of the GPU run is profiles/chol_kinds_reference.txt.  Worst ratios over every case whose schedule contains the
kind: phi / max(phi_baseline, u) where phi is checked, eta / max(eta_baseline, u), and eta / u at the two largest sizes:

  Leaf 5.40 / 1.73 / 2.17         Single 5.40 / 3.30 / -          SingleNarrow 5.40 / 1.62 / -
  SingleDense 5.40 / 1.62 / 2.17  SingleDenseNarrow 5.40 / 1.62 / 2.17                   Start 5.40 / 3.30 / 2.17
  Step 5.40 / 3.30 / -            Step2 5.40 / 3.30 / 2.17        Panel2 5.40 / 3.30 / 2.17
  Update2 5.40 / 3.30 / 2.17      BwdRect 5.40 / 3.30 / 2.17      Bwd256 5.40 / 2.03 / 2.17
  Bwd1024 1.72 / 3.30 / 2.17      BwdFused 5.40 / 3.30 / 2.17

On the trees of the coarse meshes alone no phi ratio is above 1.99 (Bwd1024: 1.72, matrix (b) on graded4 under MGB_LEAF=160)
and no eta ratio above 3.30, which is matrix (c) on graded7 (eta 6.4e-16 against 1.9e-16 of the splu baseline), the same
under both variants.

The 5.40 (and every ratio above 4) is matrix (c) at fem2d L=4 / 6, the same under every variant: kappa(S) ~ 1e4 there, and
the host MfChol (same tree, host operation order) sits at 4.65 / 4.77 of the splu baseline on the same systems while the
device and host solutions differ by 2e-15 - 3e-15 relative -- the nested-dissection Cholesky against splu's ordering, not
the device arithmetic.  Those figures are at the end of the profile."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import mgb_amd as M
import chol_reference as R
mode, kind, L, inp, out = sys.argv[3], sys.argv[4], int(sys.argv[5]), sys.argv[6], sys.argv[7]
mesh = None if sys.argv[8] == "-" else sys.argv[8]      # a name of mesh_cases.MESHES: the coarse mesh K of fem2d_mpi(L, K)
geo = getattr(M, kind + "_mpi")(L) if mesh is None else M.fem2d_mpi(L, R.MESHES[mesh])
A = M.AMG(geo, p=1.0)
dim = {"fem1d": 1, "fem2d": 2, "fem3d": 3}[kind]
x = geo.x.to_numpy()
A.set_c(np.vstack([M.DEFAULT_F[dim](xi) for xi in x]))
A.set_z(np.vstack([M.DEFAULT_G[dim](xi) for xi in x]).reshape(-1, order="F"))
l = A.L - 1
N = A.level_size(l)[0]
res = {}
if mode == "prep":                      # pattern, the Hessian at the start and (full flag) at the end of a solve
    rp, ci = A.hessian_pattern(l)
    res.update(rp=rp, ci=ci)
    if inp == "full":
        res["c"] = A.f2(l, np.zeros(N), 1.0)[1]
        sol = A.solve(solver="host")    # the matrices under test do not depend on the solver under test
        res["d"] = A.f2(l, np.zeros(N), sol["ts"][-1])[1]
else:
    data = np.load(inp)
    mats, rhs = list(data["names"]), data["rhs"]
    sched = A.chol_schedule(l)
    res.update(kinds=np.array(sched["kinds"]), workgroups=sched["workgroups"])
    if mode == "solve":
        hg, hp, hdim, _, _ = R.plan(kind, L, mesh)    # the host plan of the same tree, knobs from this process's environment
        host = R.plan_schedule(hp, hdim)
        R.free_plan(hg, hp)
        res.update(host_kinds=np.array(host["kinds"]), host_workgroups=host["cnt"])
        def solve(vals, g):             # a pivot flagged on these SPD matrices is a failure of that case: NaN, not an exit
            try:
                return A.solve_linear(l, vals, g, solver="gpu")
            except M.MGBError:
                return np.full(N, np.nan)
        res["x"] = np.array([[solve(data["m_" + m], g) for g in rhs] for m in mats])
    else:                               # replay: the same level buffers, new values each time
        a, c, g = data["m_a"], data["m_c"], rhs[0]
        x1 = A.solve_linear(l, a, g, solver="gpu")
        xc = A.solve_linear(l, c, g, solver="gpu")
        diag = R.diagonal_positions(*A.hessian_pattern(l))
        node, col, ns, height = sched["unknown_node"], sched["unknown_col"], sched["ns"], sched["height"]
        picks, codes, with_pivots = [], [], []
        for h in range(int(height.max()) + 1):
            t = int(np.flatnonzero(height == h)[np.argmax(ns[height == h])])      # the widest front of the height
            if ns[t] > 0:                                                       # (not a height of pass-through fronts)
                with_pivots.append(h)
            for k in sorted({0, 31, 32, int(ns[t]) - 1}):
                if 0 <= k < ns[t]:
                    i = int(np.flatnonzero((node == t) & (col == k))[0])
                    bad = a.copy()
                    bad[diag[i]] = -1.0
                    try:
                        A.solve_linear(l, bad, g, solver="gpu")
                        codes.append(0)
                    except M.MGBError as e:
                        codes.append(e.code)
                    picks.append((h, t, k, int(ns[t]), int(sched["nf"][t])))
        x1b = A.solve_linear(l, a, g, solver="gpu")
        res.update(x1=x1, xc=xc, x1b=x1b, picks=np.array(picks), codes=np.array(codes), with_pivots=np.array(with_pivots))
np.savez(out, **res)
"""


_CRASHED = []      # a child that died of a signal or a timeout: no further GPU process is started in this session


def _name(kind, L, mesh):
    return "%s L=%d%s" % (kind, L, "" if mesh is None else " " + mesh)


def _child(tmp_path, mode, kind, L, mesh, variant, inp, tag):
    if _CRASHED:
        pytest.fail("not started: an earlier child crashed (%s)" % _CRASHED[0])
    out = str(tmp_path / ("%s_%s_%d_%s.npz" % (mode, kind, L, tag)))
    cmd = [sys.executable, "-c", CHILD, ROOT, HERE, mode, kind, str(L), inp, out, mesh or "-"]
    try:
        r = subprocess.run(cmd, env=R.child_env(os.environ, variant), timeout=240, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CRASHED.append("%s %s %s: timeout" % (mode, _name(kind, L, mesh), variant))
        raise
    if r.returncode < 0:
        _CRASHED.append("%s %s %s: signal %d" % (mode, _name(kind, L, mesh), variant, -r.returncode))
    assert r.returncode == 0, "%s %s %s: exit %d\n%s" % (mode, _name(kind, L, mesh), variant, r.returncode, r.stderr[-3000:])
    return np.load(out)


def _schedule_text(got):
    seen = {}
    for k, w in zip(got["kinds"], got["workgroups"]):
        n, s = seen.get(str(k), (0, 0))
        seen[str(k)] = (n + 1, s + int(w))
    return " ".join("%s:%dx/%dwg" % (k, n, s) for k, (n, s) in seen.items())


def _coverage(got, must, never):
    kinds = set(str(k) for k in got["kinds"])
    return sorted(set(must) - kinds), sorted(set(never) & kinds)


def _host_plan_differs(got):
    """the host plan (mgb_plan_chol_schedule, taken in the child) against AMG.chol_schedule(): kinds and workgroups"""
    return not (np.array_equal(got["host_kinds"], got["kinds"]) and np.array_equal(got["host_workgroups"], got["workgroups"]))


_WORKLOADS = {}


def _workload(tmp_path_factory, kind, L, mesh=None):
    """pattern, the four matrices, two right-hand sides and the reference of every (matrix, rhs), once per workload"""
    if (kind, L, mesh) not in _WORKLOADS:
        tmp = tmp_path_factory.mktemp("%s%d%s" % (kind, L, mesh or ""))
        prep = _child(tmp, "prep", kind, L, mesh, "default", "full", "prep")
        rp, ci = prep["rp"], prep["ci"]
        N = len(rp) - 1
        a = R.random_spd(rp, ci, seed=100 + L)
        mats = {"a": a, "b": R.scaled(rp, ci, a, seed=200 + L), "c": prep["c"], "d": prep["d"]}
        rhs = np.array([R.rhs(N, seed=300 + 10 * L + k) for k in range(2)])
        refs = {}
        for m, vals in mats.items():
            ref = R.Reference(rp, ci, vals, N)
            refs[m] = (ref, [ref.solve(g) for g in rhs])
        inp = str(tmp / "mats.npz")
        np.savez(inp, names=np.array(list(mats)), rhs=rhs, **{"m_" + m: v for m, v in mats.items()})
        _WORKLOADS[(kind, L, mesh)] = dict(tmp=tmp, N=N, mats=mats, rhs=rhs, refs=refs, inp=inp)
    return _WORKLOADS[(kind, L, mesh)]


@pytest.mark.parametrize("kind,L,mesh", list(R.CASES), ids=[R.case_id(*c) for c in R.CASES])
def test_every_launch_kind_meets_the_reference(gpu_required, tmp_path_factory, kind, L, mesh):
    w = _workload(tmp_path_factory, kind, L, mesh)
    failures, xdef = [], None
    name = _name(kind, L, mesh)
    for variant, (must, never) in R.CASES[(kind, L, mesh)].items():
        got = _child(w["tmp"], "solve", kind, L, mesh, variant, w["inp"], variant.replace(" ", "_").replace("=", ""))
        missing, present = _coverage(got, must, never)
        sched = _schedule_text(got)
        if missing or present:
            failures.append("%s %s: schedule lacks %s / has %s (%s)" % (name, variant, missing, present, sched))
        if _host_plan_differs(got):
            failures.append("%s %s: the host plan differs from the device schedule (%s)" % (name, variant, sched))
        for mi, m in enumerate(w["mats"]):
            ref, sols = w["refs"][m]
            for k, g in enumerate(w["rhs"]):
                x = got["x"][mi, k]
                r = ref.metrics(x, g, sols[k])
                checked = r["exact"]
                print("%s  %-22s (%s) rhs %d  eta %.2e (x%.2f)  phi %.2e (x%.2f)%s  | %s" %
                      (name, variant, m, k, r["eta"], r["eta_ratio"], r["phi"], r["phi_ratio"],
                       "" if checked else " [phi not checked: reference not exact, step %.1e]" % sols[k]["refine_step"], sched))
                if m in "abc" and not checked:
                    failures.append("%s %s (%s) rhs %d: reference not exact (step %.2e)" % (name, variant, m, k,
                                                                                          sols[k]["refine_step"]))
                if not np.all(np.isfinite(x)) or not r["eta_ok"] or (checked and not r["phi_ok"]):
                    failures.append("%s %s (%s) rhs %d: eta %.3e (base %.3e) phi %.3e (base %.3e)" %
                                    (name, variant, m, k, r["eta"], r["eta_base"], r["phi"], r["phi_base"]))
        if variant == "default":
            xdef = got["x"]
        elif variant in R.BITWISE:
            same = np.array_equal(got["x"], xdef)
            print("%s  %-22s bitwise the default: %s" % (name, variant, same))
            if not same:
                failures.append("%s %s: not bitwise the default (max |dx| %.3e)" % (name, variant,
                                                                                    np.abs(got["x"] - xdef).max()))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind,L,mesh", list(R.LARGE), ids=[R.case_id(*c) for c in R.LARGE])
def test_largest_sizes_meet_the_backward_error_bound(gpu_required, tmp_path, kind, L, mesh):
    name = _name(kind, L, mesh)
    prep = _child(tmp_path, "prep", kind, L, mesh, "default", "pattern", "prep")
    rp, ci = prep["rp"], prep["ci"]
    N = len(rp) - 1
    a = R.random_spd(rp, ci, seed=100 + L)
    rhs = np.array([R.rhs(N, seed=300 + 10 * L + k) for k in range(2)])
    inp = str(tmp_path / "mats.npz")
    np.savez(inp, names=np.array(["a"]), rhs=rhs, m_a=a)
    ref = R.Reference(rp, ci, a, N, factor=False)
    failures = []
    for variant, (must, never) in R.LARGE[(kind, L, mesh)].items():
        got = _child(tmp_path, "solve", kind, L, mesh, variant, inp, variant.replace(" ", "_").replace("=", ""))
        missing, present = _coverage(got, must, never)
        sched = _schedule_text(got)
        if missing or present:
            failures.append("%s %s: schedule lacks %s / has %s (%s)" % (name, variant, missing, present, sched))
        if _host_plan_differs(got):
            failures.append("%s %s: the host plan differs from the device schedule (%s)" % (name, variant, sched))
        for k, g in enumerate(rhs):
            x = got["x"][0, k]
            eta = ref.eta(x, g)
            print("%s  %-22s (a) rhs %d  eta %.2e (x%.2f of u)  [eta only]  | %s" % (name, variant, k, eta, eta / R.U, sched))
            if not np.all(np.isfinite(x)) or not eta <= R.MARGIN * R.U:
                failures.append("%s %s rhs %d: eta %.3e" % (name, variant, k, eta))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind,L,mesh,variant", list(R.REPLAY), ids=[R.case_id(*c) for c in R.REPLAY])
def test_replay_with_new_values_and_pivot_failures(gpu_required, tmp_path_factory, kind, L, mesh, variant):
    w = _workload(tmp_path_factory, kind, L, mesh)
    name = _name(kind, L, mesh)
    got = _child(w["tmp"], "replay", kind, L, mesh, variant, w["inp"], "replay_" + variant.replace(" ", "_").replace("=", ""))
    ref, sols = w["refs"]["c"]
    r = ref.metrics(got["xc"], w["rhs"][0], sols[0])
    print("%s  %-22s replay (c) rhs 0  eta %.2e (x%.2f)  phi %.2e (x%.2f)" % (name, variant, r["eta"], r["eta_ratio"],
                                                                              r["phi"], r["phi_ratio"]))
    assert r["exact"] and r["eta_ok"] and r["phi_ok"], r
    picks, codes = got["picks"], got["codes"]
    for (h, t, k, ns, nf), code in zip(picks, codes):
        print("%s  %-22s pivot -1 at height %d node %d (ns %d, nf %d) column %d: code %d" % (name, variant, h, t, ns, nf,
                                                                                          k, code))
    assert len(picks) > 0 and set(int(h) for h in picks[:, 0]) == set(int(h) for h in got["with_pivots"])      # every height
    assert any(int(k) == 32 for k in picks[:, 2])                 # a second pivot block of a two-panel launch
    assert all(int(c) == -3 for c in codes), codes                # MGB_E_NUMERIC every time
    assert np.array_equal(got["x1b"], got["x1"])
