"""Pre-mapped child contributions of the device Cholesky (MGB_CHOL_PREMAP, csrc/chol_premap.hpp) against the gather.

The arithmetic of the factorisation does not change by one operation, so under MGB_CHOL_PREMAP = 0 (every launch gathers
through the index maps), 1 (front_single launches read slabs) and 2 (front_start launches too) solve_linear(...,
solver="gpu") must return bitwise the same solutions.  Per case -- the smallest trees that contain each situation -- a
fresh child process per mode (the knobs are read once per process; each child under its own timeout; after a child that
died of a signal or a timeout no further child is started) solves a random SPD matrix and the Newton Hessian at the start
with two right-hand sides each and reports its schedule.  A case whose expected launches do not report "consumer" fails.

The replay test solves in one process, under mode 2, matrix (a), then (c), then (a) with one diagonal entry set to -1 in
a leaf and in a single-panel front (MGB_E_NUMERIC both times), then (a) again: bitwise the first solution.  That checks the
zero-once invariant of the slabs and that NaNs a failed factorisation left in them are overwritten.

fem3d L=2: the default schedule of this tree does have Leaf and Single* launches (profiles/chol_kinds_reference.txt), so by
the rule its single launches are consumers; the case checks equality there, and the same tree with the leaf and single
kinds off -- no Leaf / Single* launch at all -- must report nothing pre-mapped.  The cases set the tile limit themselves
(512, or none where a launch is larger); one more test runs fem2d L=6 with no knob set at all, the shipped defaults."""
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
geo = getattr(M, kind + "_mpi")(L)
A = M.AMG(geo, p=1.0)
dim = {"fem1d": 1, "fem2d": 2, "fem3d": 3}[kind]
x = geo.x.to_numpy()
A.set_c(np.vstack([M.DEFAULT_F[dim](xi) for xi in x]))
A.set_z(np.vstack([M.DEFAULT_G[dim](xi) for xi in x]).reshape(-1, order="F"))
l = A.L - 1
N = A.level_size(l)[0]
res = {}
if mode == "prep":                      # pattern and the Newton Hessian at the start
    rp, ci = A.hessian_pattern(l)
    res.update(rp=rp, ci=ci, c=A.f2(l, np.zeros(N), 1.0)[1])
else:
    data = np.load(inp)
    rhs = data["rhs"]
    sched = A.chol_schedule(l)
    res.update(kinds=np.array(sched["kinds"]), workgroups=sched["workgroups"], consumer=sched["premap_consumer"],
               producers=sched["premap_producers"], slab_bytes=A.chol_info(l)["slab_bytes"])
    hg, hp, hdim, _, _ = R.plan(kind, L)      # the host plan of the same tree, knobs from this process's environment
    host = R.plan_schedule(hp, hdim)
    R.free_plan(hg, hp)
    res.update(host_consumer=host["consumer"].astype(bool), host_producers=host["producers"])
    if mode == "solve":
        res["x"] = np.array([[A.solve_linear(l, data["m_" + m], g, solver="gpu") for g in rhs] for m in "ac"])
    else:                               # replay: the same level buffers and slabs, new values each time
        a, c, g = data["m_a"], data["m_c"], rhs[0]
        x1 = A.solve_linear(l, a, g, solver="gpu")
        xc = A.solve_linear(l, c, g, solver="gpu")
        diag = R.diagonal_positions(*A.hessian_pattern(l))
        node, col, ns, nf, height = (sched[k] for k in ("unknown_node", "unknown_col", "ns", "nf", "height"))
        picks, codes = [], []
        for h in (0, 2):                # a leaf and a single-panel front (both store pre-mapped under mode 2)
            t = int(np.flatnonzero(height == h)[np.argmax(ns[height == h])])
            i = int(np.flatnonzero((node == t) & (col == 0))[0])
            bad = a.copy()
            bad[diag[i]] = -1.0
            try:
                A.solve_linear(l, bad, g, solver="gpu")
                codes.append(0)
            except M.MGBError as e:
                codes.append(e.code)
            picks.append((h, t, int(ns[t]), int(nf[t])))
        x1b = A.solve_linear(l, a, g, solver="gpu")
        res.update(x1=x1, xc=xc, x1b=x1b, picks=np.array(picks), codes=np.array(codes))
np.savez(out, **res)
"""

_CRASHED = []      # a child that died of a signal or a timeout: no further GPU process is started in this session
_FIRST = ("Leaf", "Single", "SingleNarrow", "SingleDense", "SingleDenseNarrow", "Start")      # the first launch of a height
_SINGLE = _FIRST[1:5]


def _child(tmp, mode, kind, L, env, inp, tag):
    if _CRASHED:
        pytest.fail("not started: an earlier child crashed (%s)" % _CRASHED[0])
    out = str(tmp / ("%s_%s_%d_%s.npz" % (mode, kind, L, tag)))
    cmd = [sys.executable, "-c", CHILD, ROOT, HERE, mode, kind, str(L), inp, out]
    e = R.child_env(os.environ, "default")
    e.update(env)
    try:
        r = subprocess.run(cmd, env=e, timeout=240, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CRASHED.append("%s %s L=%d %s: timeout" % (mode, kind, L, env))
        raise
    if r.returncode < 0:
        _CRASHED.append("%s %s L=%d %s: signal %d" % (mode, kind, L, env, -r.returncode))
    assert r.returncode == 0, "%s %s L=%d %s: exit %d\n%s" % (mode, kind, L, env, r.returncode, r.stderr[-3000:])
    return np.load(out)


_WORKLOADS = {}


def _workload(tmp_path_factory, kind, L, env):
    """pattern, the two matrices and two right-hand sides, once per tree (MGB_LEAF changes the tree, not the pattern)"""
    if (kind, L) not in _WORKLOADS:
        tmp = tmp_path_factory.mktemp("premap_%s%d" % (kind, L))
        prep = _child(tmp, "prep", kind, L, {}, "-", "prep")
        rp, ci = prep["rp"], prep["ci"]
        N = len(rp) - 1
        rhs = np.array([R.rhs(N, seed=300 + 10 * L + k) for k in range(2)])
        inp = str(tmp / "mats.npz")
        np.savez(inp, rhs=rhs, m_a=R.random_spd(rp, ci, seed=100 + L), m_c=prep["c"])
        _WORKLOADS[(kind, L)] = dict(tmp=tmp, inp=inp)
    return _WORKLOADS[(kind, L)]


def _first_launches(got):
    """(kind, consumer, producers) of the first launch of every height, leaves first; the host plan (mgb_plan_chol_schedule,
    taken in the child) must report the same consumers and producers as AMG.chol_schedule()"""
    assert np.array_equal(got["host_consumer"], got["consumer"]) and np.array_equal(got["host_producers"], got["producers"])
    return [(str(k), bool(c), int(p)) for k, c, p in zip(got["kinds"], got["consumer"], got["producers"]) if str(k) in _FIRST]


def _text(got):
    return " ".join("%s%s%s" % (k, "*" if c else "", "(%d)" % p if p else "") for k, c, p in _first_launches(got))


# (kind, L, extra environment) -> per mode 1 / 2: the heights whose first launch must report "consumer" (every other launch
# must not), and the launch kinds the case is about
CASES = {
    "fem1d8": ("fem1d", 8, {}, {1: [1, 2, 3, 4], 2: [1, 2, 3, 4]}, ("Leaf", "SingleNarrow")),
    "fem2d4": ("fem2d", 4, {}, {1: [1, 2, 3, 4], 2: [1, 2, 3, 4]}, ("Leaf", "SingleNarrow", "Single")),
    "fem2d6": ("fem2d", 6, {}, {1: [1, 2, 3, 4, 5], 2: [1, 2, 3, 4, 5, 6]}, ("Leaf", "Single", "Start")),
    "fem2d6_dense": ("fem2d", 6, {"MGB_CHOL_DENSE_TILES": "0", "MGB_CHOL_PREMAP_TILES": "100000"},
                     {1: [1, 2, 3, 4, 5], 2: [1, 2, 3, 4, 5, 6]}, ("SingleDense", "SingleDenseNarrow")),
    "fem2d6_noleaf": ("fem2d", 6, {"MGB_CHOL_LEAF": "0"}, {1: [2, 3, 4, 5], 2: [2, 3, 4, 5, 6]}, ("Start", "Single")),
    "fem2d6_tiles100": ("fem2d", 6, {"MGB_CHOL_PREMAP_TILES": "100"}, {1: [2, 3, 4, 5], 2: [2, 3, 4, 5, 6]}, ("Leaf", "Single")),
    "fem2d6_leaf8": ("fem2d", 6, {"MGB_LEAF": "8", "MGB_CHOL_PREMAP_TILES": "100000"},
                     {1: [1, 2, 3, 4, 5, 6, 7, 8], 2: [1, 2, 3, 4, 5, 6, 7, 8, 9]}, ("Leaf", "SingleNarrow", "Single")),
    "fem3d2": ("fem3d", 2, {}, {1: [1, 2], 2: [1, 2, 3]}, ("Leaf", "Single", "Start")),
    "fem3d2_nosingle": ("fem3d", 2, {"MGB_CHOL_LEAF": "0", "MGB_CHOL_SINGLE": "0"}, {1: [], 2: []}, ("Start",)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_premapped_solutions_are_bitwise_the_gathered_ones(gpu_required, tmp_path_factory, case):
    kind, L, env, expect, kinds = CASES[case]
    w = _workload(tmp_path_factory, kind, L, env)
    got, failures = {}, []
    for mode in (0, 1, 2):
        e = dict(env, MGB_CHOL_PREMAP=str(mode))
        e.setdefault("MGB_CHOL_PREMAP_TILES", "512")
        got[mode] = _child(w["tmp"], "solve", kind, L, e, w["inp"], "%s_m%d" % (case, mode))
        first = _first_launches(got[mode])
        print("%s PREMAP=%d  slabs %.0f bytes  | %s" % (case, mode, float(got[mode]["slab_bytes"]), _text(got[mode])))
        missing = set(kinds) - set(k for k, _, _ in first)
        if missing:
            failures.append("%s mode %d: the schedule lacks %s" % (case, mode, sorted(missing)))
        cons = [h for h, (_, c, _) in enumerate(first) if c]
        want = [] if mode == 0 else expect[mode]
        if cons != want:
            failures.append("%s mode %d: consumer heights %s, expected %s" % (case, mode, cons, want))
        # only first launches consume, a launch stores pre-mapped for its consumer parents only, and slabs exist iff used
        nfirst = sum(bool(c) for c in got[mode]["consumer"])
        if nfirst != len(cons):
            failures.append("%s mode %d: a panel or backward launch reports consumer" % (case, mode))
        prod = [h for h, (_, _, p) in enumerate(first) if p]
        if (len(prod) > 0) != (len(cons) > 0) or (float(got[mode]["slab_bytes"]) > 0) != (len(cons) > 0):
            failures.append("%s mode %d: producers %s / slab bytes %.0f do not match consumers %s" %
                            (case, mode, prod, float(got[mode]["slab_bytes"]), cons))
        if not np.all(np.isfinite(got[mode]["x"])):
            failures.append("%s mode %d: non-finite solution" % (case, mode))
    for mode in (1, 2):
        same = np.array_equal(got[mode]["x"], got[0]["x"])
        print("%s PREMAP=%d bitwise PREMAP=0: %s" % (case, mode, same))
        if not same:
            failures.append("%s mode %d: not bitwise the gather (max |dx| %.3e)" % (case, mode,
                                                                                  np.abs(got[mode]["x"] - got[0]["x"]).max()))
    if case == "fem2d6_noleaf":      # a producer launch that mixes both stores: height 1 (parents at height 2 consume) ...
        first = _first_launches(got[2])
        if not (first[1][2] > 0 and not first[1][1] and first[0][2] == 0):      # ... gathers itself from the front_start fronts
            failures.append("fem2d6_noleaf: height 0 / 1 producers %d / %d" % (first[0][2], first[1][2]))
    assert not failures, "\n".join(failures)


def test_default_knobs_are_bitwise_the_gather(gpu_required, tmp_path_factory):
    """no MGB_CHOL_PREMAP* variable at all: the defaults (front_single consumers, 400 workgroups) against PREMAP=0"""
    w = _workload(tmp_path_factory, "fem2d", 6, {})
    off = _child(w["tmp"], "solve", "fem2d", 6, {"MGB_CHOL_PREMAP": "0"}, w["inp"], "defaults_off")
    got = _child(w["tmp"], "solve", "fem2d", 6, {}, w["inp"], "defaults")
    first = _first_launches(got)
    print("defaults  slabs %.0f bytes  | %s" % (float(got["slab_bytes"]), _text(got)))
    assert [h for h, (_, c, _) in enumerate(first) if c] == [1, 2, 3, 4, 5]
    assert [h for h, (_, _, p) in enumerate(first) if p] == [0, 1, 2, 3, 4]
    assert np.all(np.isfinite(got["x"])) and np.array_equal(got["x"], off["x"])


def test_replay_keeps_the_slabs_consistent(gpu_required, tmp_path_factory):
    w = _workload(tmp_path_factory, "fem2d", 6, {})
    got = _child(w["tmp"], "replay", "fem2d", 6, {"MGB_CHOL_PREMAP": "2"}, w["inp"], "replay")
    first = _first_launches(got)
    print("replay PREMAP=2 | %s" % _text(got))
    assert [h for h, (_, c, _) in enumerate(first) if c] == [1, 2, 3, 4, 5, 6]
    assert first[0][2] > 0 and first[2][2] > 0          # the leaf and the height-2 launch store pre-mapped
    for (h, t, ns, nf), code in zip(got["picks"], got["codes"]):
        print("replay pivot -1 at height %d node %d (ns %d, nf %d): code %d" % (h, t, ns, nf, code))
    assert len(got["codes"]) == 2 and all(int(c) == -3 for c in got["codes"]), got["codes"]      # MGB_E_NUMERIC
    assert np.all(np.isfinite(got["xc"]))
    assert np.array_equal(got["x1b"], got["x1"])
