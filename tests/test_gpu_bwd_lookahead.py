"""The look-ahead panel loop of the fused backward sweep (backward_fused_kernel: the substituting wave of a group applies
a solved panel to the 32 columns below it and substitutes them straight away, the other waves update the earlier columns
meanwhile, one barrier per panel) against the per-height launches (MGB_CHOL_BWD_FUSED=0): bit for bit.

Per tree the two matrices of chol_reference (random_spd, scaled) on the plan's pattern with three right-hand sides of
chol_reference.rhs; every solve is done twice in the child and must repeat itself.  The knobs are read once per process, so
every schedule runs in a fresh child process under its own timeout; the per-height solution of a tree is computed once.

The trees are the smallest that hold each shape of the loop (test_trees_hold_the_shapes checks that on the host, from the
ns / nf / parent of mgb_plan_chol_tree alone):
  fem2d L=5          root 63 = 2 panels, the last one 31 wide; leaves of 2 panels (ns 43) side by side
  fem2d L=6          root 127 = 4 panels; path fronts of 62 = 2 panels, the last one 30 wide, with boundaries
  fem3d L=2          root 50: last panel 18 wide
  fem3d L=3          242 = 8 panels (last 18 wide), 110 = 4 panels (last 14 wide), fronts up to nf = 352
  fem1d L=8          leaves of exactly two full panels, ancestors with ns = 2
  fem2d L=4, LEAF=8  eight heights of one narrow panel each
Schedules: MGB_CHOL_BWD_CUT 1 / 2 / 4 at 256 and 512 threads (256: four waves, so groups of ONE wave on the wider subtree
levels, which play both roles in sequence), and the front-size thresholds of test_gpu_bwd_fused.MIXED (ancestors read
from y)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_reference as R
import test_gpu_bwd_fused as BF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PB = 32

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import mgb_amd as M
kind, L, inp, out = sys.argv[3], int(sys.argv[4]), sys.argv[5], sys.argv[6]
geo = getattr(M, kind + "_mpi")(L)
A = M.AMG(geo, p=1.0)
dim = {"fem1d": 1, "fem2d": 2, "fem3d": 3}[kind]
x = geo.x.to_numpy()
A.set_c(np.vstack([M.DEFAULT_F[dim](xi) for xi in x]))
A.set_z(np.vstack([M.DEFAULT_G[dim](xi) for xi in x]).reshape(-1, order="F"))
l = A.L - 1
data = np.load(inp)
rp, ci = A.hessian_pattern(l)
assert np.array_equal(rp, data["rp"]) and np.array_equal(ci, data["ci"]), "the level's pattern is not the plan's"
kinds = np.array(A.chol_schedule(l)["kinds"])
xs = [np.array([[A.solve_linear(l, data["m_" + m], g, solver="gpu") for g in data["rhs"]] for m in "ab"]) for _ in range(2)]
np.savez(out, x=xs[0], x2=xs[1], kinds=kinds)
"""

TREES = (("fem2d", 5, None), ("fem2d", 6, None), ("fem3d", 2, None), ("fem3d", 3, None), ("fem1d", 8, None), ("fem2d", 4, "8"))
# the front-size thresholds of test_gpu_bwd_fused.MIXED; that of fem2d L=4 (44) also splits its MGB_LEAF=8 tree (nf 45 at
# height 6, at most 44 below: two per-height launches, then the fused one)
MIXED = {tree: BF.MIXED[tree[:2]] for tree in TREES if tree[:2] in BF.MIXED}
OLD = {"MGB_CHOL_BWD_FUSED": "0"}


def _schedules(tree):
    out = [("cut%d_%d" % (c, t), {"MGB_CHOL_BWD_FUSED": "1", "MGB_CHOL_BWD_CUT": str(c), "MGB_CHOL_BWD_FUSED_THREADS": str(t)})
           for c in (1, 2, 4) for t in (256, 512)]
    if tree in MIXED:
        out.append(("mixed", {"MGB_CHOL_BWD_FUSED": "1", "MGB_CHOL_BWD_FUSED_NF": MIXED[tree]}))
    return out


CASES = [(tree, name, env) for tree in TREES for name, env in _schedules(tree)]


def _tree(kind, L, leaf):
    """(ns, nf, parent, height above the leaves) of the plan's elimination tree, rp, ci: host only"""
    saved = os.environ.pop("MGB_LEAF", None)
    try:
        if leaf is not None:
            os.environ["MGB_LEAF"] = leaf      # read on every analysis
        g, p, dim, N, nz = R.plan(kind, L)
        ns, nf, par = (a.astype(np.int64) for a in R.plan_tree(p, dim))
        rp, ci = R.plan_pattern(p, N, nz)
        R.free_plan(g, p)
    finally:
        os.environ.pop("MGB_LEAF", None)
        if saved is not None:
            os.environ["MGB_LEAF"] = saved
    h = np.zeros(len(ns), dtype=np.int64)
    for t in range(len(ns)):      # postorder: children before their parent
        if par[t] >= 0:
            h[par[t]] = max(h[par[t]], h[t] + 1)
    return ns, nf, par, h, rp, ci


def _widest_level(par, h, cut):
    """most fronts at one depth of one maximal subtree of height <= cut"""
    depth = np.zeros(len(par), dtype=np.int64)
    root = np.arange(len(par))
    for t in range(len(par) - 1, -1, -1):      # parents before their children
        if par[t] >= 0 and h[par[t]] <= cut:
            depth[t], root[t] = depth[par[t]] + 1, root[par[t]]
    sub = h <= cut
    return int(np.unique(np.stack([root[sub], depth[sub]]), axis=1, return_counts=True)[1].max())


def test_trees_hold_the_shapes():
    T = {tree: _tree(*tree)[:4] for tree in TREES}
    panels = lambda n: (n + PB - 1) // PB
    ns, nf, par, h = T[("fem2d", 5, None)]
    assert ns[par < 0].tolist() == [63] and np.count_nonzero((h == 0) & (ns == 43)) >= 2
    ns, nf, par, h = T[("fem2d", 6, None)]
    assert ns[par < 0].tolist() == [127] and np.count_nonzero((h > 4) & (ns == 62) & (nf > ns)) >= 2
    ns, nf, par, h = T[("fem3d", 2, None)]
    assert ns[par < 0].tolist() == [50]
    ns, nf, par, h = T[("fem3d", 3, None)]
    assert ns[par < 0].tolist() == [242] and 110 in ns[h > 4] and nf.max() == 352
    ns, nf, par, h = T[("fem1d", 8, None)]
    assert 64 in ns[h == 0] and np.all(ns[h > 0] == 2)
    ns, nf, par, h = T[("fem2d", 4, "8")]
    assert h.max() == 7 and ns.max() < PB
    # over the schedules (cut 1, 2, 4; 4 or 8 waves): a path front (height above the cut) of at least three panels, one whose
    # last panel is narrower than 32 behind a full one, and a subtree level with more fronts than the workgroup has waves
    for cut in (1, 2, 4):
        path = [(n, tree) for tree, (ns, nf, par, h) in T.items() for n in ns[h > cut]]
        assert any(panels(n) >= 3 for n, _ in path), cut
        assert any(panels(n) >= 2 and n % PB for n, _ in path), cut
    # the kernel's rule for the waves per front of a level: halved until every front of the level has a group
    def group(W, cnt):
        G = W
        while G > 1 and W // G < cnt:
            G >>= 1
        return G
    for W in (4, 8):      # 256 and 512 threads
        wide = {cut: max(_widest_level(par, h, cut) for ns, nf, par, h in T.values()) for cut in (1, 2, 4)}
        assert wide[4] > W, (W, wide)                     # more fronts than waves: several rounds of groups of one wave
        assert group(W, wide[1]) >= 2, (W, wide)          # groups of at least two waves below the path as well
    assert group(4, max(_widest_level(par, h, 2) for ns, nf, par, h in T.values())) == 1      # as many fronts as waves


_CRASHED = []      # a child that died of a signal or a timeout: no further GPU process is started in this session
_WORK = {}


def _child(tmp, tree, name, env, inp):
    if _CRASHED:
        pytest.fail("not started: an earlier child crashed (%s)" % _CRASHED[0])
    kind, L, leaf = tree
    out = str(tmp / ("%s.npz" % name))
    e = R.child_env(os.environ, "default")
    e.update(env)
    if leaf is not None:
        e["MGB_LEAF"] = leaf
    cmd = [sys.executable, "-c", CHILD, ROOT, HERE, kind, str(L), inp, out]
    try:
        r = subprocess.run(cmd, env=e, timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _CRASHED.append("%s %s: timeout" % (tree, name))
        raise
    if r.returncode < 0:
        _CRASHED.append("%s %s: signal %d" % (tree, name, -r.returncode))
    assert r.returncode == 0, "%s %s: exit %d\n%s" % (tree, name, r.returncode, r.stderr[-3000:])
    return np.load(out)


def _work(tmp_path_factory, tree):
    """matrices, right-hand sides and the per-height solution of one tree, once"""
    if tree not in _WORK:
        kind, L, leaf = tree
        tmp = tmp_path_factory.mktemp("%s%d%s" % (kind, L, leaf or ""))
        rp, ci = _tree(*tree)[4:]
        N = len(rp) - 1
        a = R.random_spd(rp, ci, seed=100 + L)
        rhs = np.array([R.rhs(N, seed=300 + 10 * L + k) for k in range(3)])
        inp = str(tmp / "mats.npz")
        np.savez(inp, rp=rp, ci=ci, rhs=rhs, m_a=a, m_b=R.scaled(rp, ci, a, seed=200 + L))
        _WORK[tree] = dict(tmp=tmp, inp=inp)      # (kept before the child runs: a crash is not repeated per case)
        old = _child(tmp, tree, "old", OLD, inp)
        assert "BwdFused" not in set(str(k) for k in old["kinds"])
        assert np.all(np.isfinite(old["x"])) and np.array_equal(old["x"], old["x2"])
        _WORK[tree]["old"] = old["x"]
    assert "old" in _WORK[tree], "the per-height solve of %s failed earlier" % (tree,)
    return _WORK[tree]


@pytest.mark.gpu
@pytest.mark.parametrize("tree,name,env", CASES, ids=["%s%d%s-%s" % (t[0], t[1], "leaf" + t[2] if t[2] else "", n) for t, n, _ in CASES])
def test_look_ahead_sweep_is_bitwise_the_per_height_sweep(gpu_required, tmp_path_factory, tree, name, env):
    w = _work(tmp_path_factory, tree)
    got = _child(w["tmp"], tree, name, env, w["inp"])
    assert "BwdFused" in set(str(k) for k in got["kinds"]), "%s %s: no fused launch in the schedule" % (tree, name)
    x, xo = got["x"], w["old"]
    print("%s %-9s max |x - x_old| = %.3e" % (tree, name, np.abs(x - xo).max()))
    assert np.array_equal(x, got["x2"])
    assert np.array_equal(x, xo)
