"""Host-only companions of test_gpu_chol_kinds.py (no GPU needed):

  * the case table of the device test names every one of the 14 launch kinds, in the order the C header documents;
  * the elimination trees of the table's workloads and MGB_LEAF values contain the front shapes at the tile edges
    (pass-through fronts, own sizes at the 32-column panel edges, front sizes at the 64-row tile edges, large fronts);
  * the host multifrontal Cholesky (MfChol, solver="host") meets the bounds of chol_reference.py against the refined
    reference, which runs the reference machinery on every CI run and pins the baseline ratios."""
import os
import re

import numpy as np
import pytest

import chol_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    for kind, L, variant in R.REPLAY:
        assert variant in R.CASES[(kind, L)]


def _shapes(ns, nf):
    return {
        "ns = 0": int(np.sum(ns == 0)),
        "ns = 0 (mod 32)": int(np.sum((ns > 0) & (ns % 32 == 0))),
        "ns = 1 (mod 32)": int(np.sum((ns > 1) & (ns % 32 == 1))),
        "ns = 31 (mod 32)": int(np.sum(ns % 32 == 31)),
        "nf + 1 = 0 (mod 64)": int(np.sum((nf + 1) % 64 == 0)),
        "nf + 1 = 1 (mod 64)": int(np.sum((nf > 0) & ((nf + 1) % 64 == 1))),
        "nf + 1 = 63 (mod 64)": int(np.sum((nf + 1) % 64 == 63)),
        "nf > 384": int(np.sum(nf > 384)),
    }


def test_tree_shapes_cover_the_tile_edges(monkeypatch):
    found = {}
    for kind, L, leaf in R.SHAPE_TREES:
        if leaf is None:
            monkeypatch.delenv("MGB_LEAF", raising=False)
        else:
            monkeypatch.setenv("MGB_LEAF", leaf)
        h, p, dim, N, nz = R.plan(kind, L)
        try:
            ns, nf, par = R.plan_tree(p, dim)
        finally:
            R.free_plan(h, p)
        assert int(ns.sum()) == N
        for shape, cnt in _shapes(ns, nf).items():
            if cnt:
                found.setdefault(shape, []).append("%s L=%d%s: %d" % (kind, L, "" if leaf is None else " MGB_LEAF=" + leaf, cnt))
    for shape in _shapes(np.zeros(1, dtype=int), np.zeros(1, dtype=int)):
        print("%-22s %s" % (shape, "; ".join(found.get(shape, ["-"]))))
    missing = [s for s in _shapes(np.zeros(1, dtype=int), np.zeros(1, dtype=int)) if s not in found]
    assert not missing, "no tree of the table has a front with " + ", ".join(missing)


@pytest.mark.parametrize("leaf", [None, "8"])
@pytest.mark.parametrize("kind,L", [("fem2d", 5), ("fem2d", 6), ("fem3d", 3)])
def test_host_cholesky_meets_the_reference(monkeypatch, kind, L, leaf):
    import ctypes as C
    from mgb_amd import _lib
    if leaf is None:
        monkeypatch.delenv("MGB_LEAF", raising=False)
    else:
        monkeypatch.setenv("MGB_LEAF", leaf)
    h, p, dim, N, nz = R.plan(kind, L)
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
                print("%s L=%d leaf=%s (%s) rhs %d: eta %.2e (base %.2e)  phi %.2e (base %.2e, ratio %.2f)  refined eta %.1e" %
                      (kind, L, leaf or "default", name, k, m["eta"], m["eta_base"], m["phi"], m["phi_base"], m["phi_ratio"],
                       r["refine_eta"]))
                if not (m["exact"] and m["eta_ok"] and m["phi_ok"]):
                    bad.append((name, k, m))
        assert not bad, bad
    finally:
        if ch.value:
            _lib.call("mgb_hostchol_destroy", ch)
        R.free_plan(h, p)
