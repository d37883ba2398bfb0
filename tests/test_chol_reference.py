"""Host-only companions of test_gpu_chol_kinds.py (no GPU needed):

  * the case table of the device test names every one of the 14 launch kinds, in the order the C header documents;
  * the elimination trees of the table's workloads and MGB_LEAF values contain the front shapes at the tile edges
    (pass-through fronts, own sizes at the 32-column panel edges, front sizes at the 64-row tile edges, large fronts);
  * the trees of the coarse meshes of mesh_cases.py (chol_reference.NEW_TREES) have the sizes the cases were chosen for, and the
    domain of two components a root without own columns and two children;
  * the host multifrontal Cholesky (MfChol, solver="host") meets the bounds of chol_reference.py against the refined
    reference, which runs the reference machinery on every CI run and pins the baseline ratios."""
import os
import re

import numpy as np
import pytest

import chol_reference as R
import mesh_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = [("fem2d", 5, None), ("fem2d", 6, None), ("fem3d", 3, None), ("fem2d", 3, "graded4"), ("fem2d", 4, "graded4")]


def test_chol_kind_table_covers_every_kind():
    import mgb_amd as M
    with open(os.path.join(ROOT, "include", "mgb_hip.h")) as f:
        hdr = f.read()
    block = hdr[hdr.index("Kind codes (GpuChol::Kind):"):]
    block = block[:block.index("unknown_node")]
    documented = re.findall(r"(\d+) (\w+)", block)
    assert [int(c) for c, _ in documented] == list(range(14))
    assert tuple(n for _, n in documented) == R.KINDS == M.AMG.CHOL_KINDS
    with open(os.path.join(ROOT, "multigridbarriermpi.jl_amd", "csrc", "chol_plan.hpp")) as f:
        enum = re.search(r"enum class Kind : unsigned char \{([^}]*)\}", f.read()).group(1)
    assert tuple(k.strip() for k in enum.split(",") if k.strip()) == R.KINDS
    covered = set()
    for table in (R.CASES, R.LARGE):
        for variants in table.values():
            for name, (must, never) in variants.items():
                assert name in R.VARIANTS
                assert set(must) <= set(R.KINDS) and set(never) <= set(R.KINDS)
                covered |= set(must)
    assert covered == set(R.KINDS), sorted(set(R.KINDS) - covered)
    for kind, L, mesh, variant in R.REPLAY:
        assert variant in R.CASES[(kind, L, mesh)]
    for key in R.NEW_TREES:
        assert key in R.CASES and key[2] in MC.NAMES


def _shapes(ns, nf, par=None):
    return {
        "ns = 0": int(np.sum(ns == 0)),
        "ns = 0 (mod 32)": int(np.sum((ns > 0) & (ns % 32 == 0))),
        "ns = 1 (mod 32)": int(np.sum((ns > 1) & (ns % 32 == 1))),
        "ns = 31 (mod 32)": int(np.sum(ns % 32 == 31)),
        "nf + 1 = 0 (mod 64)": int(np.sum((nf + 1) % 64 == 0)),
        "nf + 1 = 1 (mod 64)": int(np.sum((nf > 0) & ((nf + 1) % 64 == 1))),
        "nf + 1 = 63 (mod 64)": int(np.sum((nf + 1) % 64 == 63)),
        "nf > 384": int(np.sum(nf > 384)),
        "internal node with ns = 0": 0 if par is None else int(np.sum((ns == 0) & (np.bincount(par[par >= 0], minlength=len(ns)) > 0))),
    }


def test_tree_shapes_cover_the_tile_edges(monkeypatch):
    found = {}
    for kind, L, mesh, leaf in R.SHAPE_TREES:
        if leaf is None:
            monkeypatch.delenv("MGB_LEAF", raising=False)
        else:
            monkeypatch.setenv("MGB_LEAF", leaf)
        h, p, dim, N, nz = R.plan(kind, L, mesh)
        try:
            ns, nf, par = R.plan_tree(p, dim)
        finally:
            R.free_plan(h, p)
        assert int(ns.sum()) == N
        for shape, cnt in _shapes(ns, nf, par).items():
            if cnt:
                found.setdefault(shape, []).append("%s L=%d%s%s: %d" % (kind, L, "" if mesh is None else " " + mesh,
                                                                         "" if leaf is None else " MGB_LEAF=" + leaf, cnt))
    for shape in _shapes(np.zeros(1, dtype=int), np.zeros(1, dtype=int)):
        print("%-22s %s" % (shape, "; ".join(found.get(shape, ["-"]))))
    missing = [s for s in _shapes(np.zeros(1, dtype=int), np.zeros(1, dtype=int)) if s not in found]
    assert not missing, "no tree of the table has a front with " + ", ".join(missing)


def test_new_trees_are_the_ones_the_cases_were_chosen_for(monkeypatch):
    """N and the largest own / front size of the trees of the coarse meshes; two_squares: the root has no own column (the
    empty separator between the two components) and two children, and graded4 L = 4 has no front without own columns."""
    monkeypatch.delenv("MGB_LEAF", raising=False)
    want = {("fem2d", 4, "graded4"): (11522, 228, 394), ("fem2d", 3, "graded4"): (2882, 112, 197),
            ("fem2d", 4, "graded7"): (18434, 498, 671), ("fem2d", 5, "lshape"): (9218, 127, 243),
            ("fem2d", 4, "two_squares"): (1540, 43, 64)}
    assert set(want) == set(R.NEW_TREES)
    for key in R.NEW_TREES:
        h, p, dim, N, nz = R.plan(*key)
        try:
            ns, nf, par = R.plan_tree(p, dim)
        finally:
            R.free_plan(h, p)
        assert (N, int(ns.max()), int(nf.max())) == want[key], key
        root = len(ns) - 1
        assert par[root] == -1 and np.count_nonzero(par == -1) == 1
        if key[2] == "two_squares":
            assert ns[root] == 0 and nf[root] == 0 and np.count_nonzero(par == root) == 2
        else:
            assert ns[root] > 0


@pytest.mark.parametrize("leaf", [None, "8"])
@pytest.mark.parametrize("kind,L,mesh", HOST_CASES, ids=[R.case_id(*c) for c in HOST_CASES])
def test_host_cholesky_meets_the_reference(monkeypatch, kind, L, mesh, leaf):
    import ctypes as C
    from mgb_amd import _lib
    if leaf is None:
        monkeypatch.delenv("MGB_LEAF", raising=False)
    else:
        monkeypatch.setenv("MGB_LEAF", leaf)
    h, p, dim, N, nz = R.plan(kind, L, mesh)
    ch = C.c_void_p()
    try:
        rp, ci = R.plan_pattern(p, N, nz)
        _lib.call("mgb_plan_hostchol_create", p, dim, C.byref(ch))
        a = R.random_spd(rp, ci, seed=1000 + L)
        mats = {"a": a, "b": R.scaled(rp, ci, a, seed=2000 + L)}
        bad = []
        for name, vals in mats.items():
            ref = R.Reference(rp, ci, vals, N)
            for k in range(2):
                g = R.rhs(N, seed=3000 + 10 * L + k)
                r = ref.solve(g)
                x = np.empty(N)
                _lib.call("mgb_hostchol_factor_solve", ch, _lib.dptr(vals), _lib.dptr(g), _lib.dptr(x))
                m = ref.metrics(x, g, r)
                print("%s L=%d%s leaf=%s (%s) rhs %d: eta %.2e (base %.2e, ratio %.2f)  phi %.2e (base %.2e, ratio %.2f)  refined eta %.1e" %
                      (kind, L, "" if mesh is None else " " + mesh, leaf or "default", name, k, m["eta"], m["eta_base"], m["eta_ratio"],
                       m["phi"], m["phi_base"], m["phi_ratio"], r["refine_eta"]))
                if not (m["exact"] and m["eta_ok"] and m["phi_ok"]):
                    bad.append((name, k, m))
        assert not bad, bad
    finally:
        if ch.value:
            _lib.call("mgb_hostchol_destroy", ch)
        R.free_plan(h, p)
