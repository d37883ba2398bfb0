"""Host-only checks of the plan of the device Cholesky chain (csrc/chol_plan.hpp) through mgb_plan_chol_schedule: which
launches run over which jobs, without a GPU.  Over the trees and knob variants of chol_reference.CASES, the MGB_LEAF trees of
chol_reference.SHAPE_TREES and the two trees of chol_reference.LARGE (one analysis of fem2d L=8 takes 0.45 s, of fem3d L=4
0.12 s; their cases 0.7 - 2.6 s each), every rule below is recomputed in Python from ns, nf and parent alone (children of a
node in ascending index are its two slots):

  * kinds: the must-contain / must-not sets of CASES and LARGE hold on the host plan (what test_gpu_chol_kinds asserts on
    the device);
  * order: forward launches by ascending height; one first launch (Leaf, Single*, Start) per non-empty height (with zero
    workgroups where no front of the height has a row: the root of a disconnected domain), followed --
    Start heights only -- by panel launches with ascending p that cover panels 0 .. ceil(max_ns / 32) - 1 exactly once
    (Step one, Step2 and Panel2 + Update2 two); backward launches by descending height, none for heights <= h_top of the
    fused plan, BwdFused last;
  * first launches: workgroups, consumer flag and producers equal hwg, hconsumer and the per-height sum of producer of
    mgb_plan_chol_premap under the same knobs, and the workgroups equal the count recomputed here;
  * tiles: every Step / Step2 / Update2 launch holds, per front with ns > 32 p, exactly the lower triangle of the trailing
    matrix from row k = min(ns, 32 (p + np)), each tile once, behind npiv leading pivot jobs, one per front with k < ns; a
    Panel2 launch one pivot job per front and one job per 64-row block below the pivot block;
  * start jobs: leading rb = -1 jobs for the fronts with ns > 0 (pivot knob on), then per front, chunk-major,
    ceil((nf + 1 - 32 chunk) / 256) row blocks whose [a0, a1) ranges tile the front's assembly range; every apos of a job
    lies in the job's 32 columns and 256 rows, on or below the diagonal; asrc names every pattern entry exactly once;
  * backward: rect jobs are the 64-column chunks of the fronts with a boundary on heights with max_nf > bwd_split_nf;
    h_top, workgroups and LDS bytes of BwdFused equal those of mgb_plan_chol_bwd_fused;
  * split (fem2d L=6, world 2 and 4): every node is in exactly one rank's own list or in the top list, no launch is a
    consumer, no fused launch exists."""
import ctypes as C

import numpy as np
import pytest

import chol_reference as R

PB, TS, TB = 32, 64, 256
FIRST = ("Leaf", "Single", "SingleNarrow", "SingleDense", "SingleDenseNarrow", "Start")
PANEL = ("Step", "Step2", "Panel2", "Update2")


def _cases():
    out = []
    for table in (R.CASES, R.LARGE):
        for (kind, L, mesh), variants in table.items():
            out += [(kind, L, mesh, v) for v in variants]
    for kind, L, mesh, leaf in R.SHAPE_TREES:
        if leaf is not None and (kind, L, mesh, "MGB_LEAF=" + leaf) not in out:
            out.append((kind, L, mesh, "MGB_LEAF=" + leaf))
    return out


_TREES = {}


def _tree(monkeypatch, kind, L, leaf, mesh=None):
    """plan handle and the tree with everything derived from ns / nf / parent, once per (workload, MGB_LEAF)"""
    if leaf is None:
        monkeypatch.delenv("MGB_LEAF", raising=False)      # read on every analysis
    else:
        monkeypatch.setenv("MGB_LEAF", leaf)
    if (kind, L, mesh, leaf) not in _TREES:
        h, p, dim, N, nz = R.plan(kind, L, mesh)
        ns, nf, par = (a.astype(np.int64) for a in R.plan_tree(p, dim))
        n = len(ns)
        height, kids = np.zeros(n, dtype=np.int64), [[] for _ in range(n)]
        for t in range(n):
            if par[t] >= 0:
                assert par[t] > t
                height[par[t]] = max(height[par[t]], height[t] + 1)
                kids[par[t]].append(t)
        fronts = [np.flatnonzero(height == hh) for hh in range(int(height.max()) + 1)]
        _TREES[(kind, L, mesh, leaf)] = dict(p=p, dim=dim, nz=nz, ns=ns, nf=nf, par=par, height=height, kids=kids, fronts=fronts)
    return _TREES[(kind, L, mesh, leaf)]


def _premap(T, kn):
    from mgb_amd import _lib
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    nn, nh = len(T["ns"]), len(T["fronts"])
    info = np.zeros(5, dtype=np.int64)
    producer, hkind, hwg, hcons = np.zeros(nn, dtype=np.int32), *(np.zeros(nh, dtype=np.int32) for _ in range(3))
    _lib.call("mgb_plan_chol_premap", T["p"], T["dim"], kn["MGB_CHOL_LEAF"], kn["MGB_CHOL_SINGLE"], kn["MGB_CHOL_PREMAP"],
              kn["MGB_CHOL_PREMAP_TILES"], info.ctypes.data_as(C.POINTER(C.c_longlong)), nn, None, ip(producer), None, None, None,
              None, nh, ip(hkind), ip(hwg), ip(hcons), 0, None, 0, None)
    assert (int(info[0]), int(info[1])) == (nn, nh)
    return producer, hkind, hwg, hcons


def _fused(T, kn):
    from mgb_amd import _lib
    info = np.zeros(12, dtype=np.int32)
    _lib.call("mgb_plan_chol_bwd_fused", T["p"], T["dim"], kn["MGB_CHOL_BWD_CUT"], kn["MGB_CHOL_BWD_FUSED_NF"],
              kn["MGB_CHOL_BWD_FUSED_THREADS"], info.ctypes.data_as(C.POINTER(C.c_int)), 0, None, 0, None, None, 0, None, None)
    return dict(h_top=int(info[0]), nwg=int(info[2]), lds=int(info[8]))


def _ceil(a, b):
    return -(-a // b)


def _tile_set(nf, k):
    """(ti, tj) of the lower triangle of the trailing matrix of a front from row k on (the right-hand-side row included)"""
    Tr, Tc = _ceil(nf + 1 - k, TS), max(1, _ceil(nf - k, TS))
    return [(ti, tj) for ti in range(Tr) for tj in range(min(ti, Tc - 1) + 1)]


def _start_jobs(nf):
    return [(ch, rb) for ch in range(_ceil(nf, PB)) for rb in range(_ceil(nf + 1 - ch * PB, TB))]


def _launch_nodes(S, i):
    """the fronts of launch i, one entry per job"""
    k, o, c = S["kinds"][i], S["ofs"][i], S["cnt"][i]
    if k in ("Leaf", "Bwd256", "Bwd1024"):
        return S["lists"][o:o + c]
    if k in FIRST[1:5]:
        return S["singles"][o:o + c, 0]
    if k == "Start":
        return S["starts"][o:o + c, 0]
    if k in PANEL:
        return S["tiles"][o:o + c, 0]
    if k == "BwdRect":
        return S["rects"][o:o + c, 0]
    raise AssertionError(k)


def _check_forward(T, S, kn, begin, end, fronts, premap):
    """launches [begin, end): the forward sweep over the node set `fronts` (per height); premap: the pre-map plan or None"""
    ns, nf, height = T["ns"], T["nf"], T["height"]
    pivot = bool(kn["MGB_CHOL_START_PIVOT"])
    i = begin
    for hh, mine in enumerate(fronts):
        if len(mine) == 0:
            continue
        assert i < end and S["kinds"][i] in FIRST, (hh, i)
        kind, cnt, nodes = S["kinds"][i], int(S["cnt"][i]), _launch_nodes(S, i)
        # (a front without rows, the empty-separator root of a disconnected domain, has no job in its Start launch: the
        # launch is planned with zero workgroups, which GpuChol::run passes over)
        jobless = [t for t in mine if kind == "Start" and nf[t] == 0]
        assert set(height[nodes]) <= {hh} and set(nodes) == set(mine) - set(jobless)
        assert len(nodes) > 0 or (cnt == 0 and len(jobless) == len(mine))
        # the first launch: its workgroups, recomputed
        if kind == "Leaf":
            want, npanel = len(mine), 0
            assert list(nodes) == list(mine)
        elif kind == "Start":
            want = sum(len(_start_jobs(nf[t])) + (pivot and ns[t] > 0) for t in mine)
            npanel = _ceil(int(ns[mine].max()), PB)
            _check_start(T, S, i, mine, pivot)
        else:
            assert ns[mine].max() <= PB and ns[mine].min() >= 1
            want, npanel = sum(len(_tile_set(nf[t], ns[t])) for t in mine), 0
            jobs = S["singles"][S["ofs"][i]:S["ofs"][i] + cnt]
            assert [tuple(j) for j in jobs] == [(t, ti, tj) for t in mine for ti, tj in _tile_set(nf[t], ns[t])]
        assert cnt == want, (hh, kind, cnt, want)
        if premap is not None:
            producer, hkind, hwg, hcons = premap
            # mgb_plan_chol_premap reads the pivot knob from the environment (on): without pivot jobs a Start launch is
            # smaller by one job per front with own columns
            adjust = int(np.sum(ns[mine] > 0)) if (kind == "Start" and not pivot) else 0
            assert hkind[hh] == {"Leaf": 0, "Start": 2}.get(kind, 1)
            assert cnt == hwg[hh] - adjust and bool(S["consumer"][i]) == bool(hcons[hh])
            assert S["producers"][i] == producer[mine].sum()
        else:
            assert not S["consumer"][i] and S["producers"][i] == 0
        i += 1
        # the panel launches of the height
        covered = []
        while i < end and S["kinds"][i] in PANEL:
            kind, p = S["kinds"][i], int(S["p"][i])
            assert set(height[_launch_nodes(S, i)]) <= {hh}
            if kind == "Panel2":
                assert i + 1 < end and S["kinds"][i + 1] == "Update2" and S["p"][i + 1] == p
                _check_panel2(T, S, i, mine, p)
            else:
                _check_tiles(T, S, i, mine, p, 1 if kind == "Step" else 2)
                if kind == "Update2":
                    assert S["kinds"][i - 1] == "Panel2" and S["npiv"][i] == 0
            if kind != "Panel2":
                covered += [p] if kind == "Step" else [p, p + 1]
            i += 1
        assert covered == list(range(npanel)), (hh, covered, npanel)
    assert i == end


def _check_tiles(T, S, i, mine, p, np_):
    ns, nf = T["ns"], T["nf"]
    jobs = [tuple(j) for j in S["tiles"][S["ofs"][i]:S["ofs"][i] + S["cnt"][i]]]
    npiv = int(S["npiv"][i])
    active = [t for t in mine if ns[t] > PB * p]
    k = {t: min(int(ns[t]), PB * (p + np_)) for t in active}
    if S["kinds"][i] != "Update2":      # the leading pivot jobs: one per front that still has a pivot block to factor
        assert jobs[:npiv] == [(t, 0, 0) for t in active if k[t] < ns[t]]
    want = [(t, ti, tj) for t in active for ti, tj in _tile_set(nf[t], k[t])]
    assert sorted(jobs[npiv:]) == sorted(want) and len(set(want)) == len(want)


def _check_panel2(T, S, i, mine, p):
    ns, nf = T["ns"], T["nf"]
    jobs = [tuple(j) for j in S["tiles"][S["ofs"][i]:S["ofs"][i] + S["cnt"][i]]]
    npiv = int(S["npiv"][i])
    active = [t for t in mine if ns[t] > PB * p]
    assert jobs[:npiv] == [(t, 0, 0) for t in active]
    want = [(t, b, b) for t in active for b in range(max(0, _ceil(int(nf[t]) + 1 - min(int(ns[t]), PB * (p + 2)) - PB, TS)))]
    assert jobs[npiv:] == want


def _check_start(T, S, i, mine, pivot):
    ns, nf = T["ns"], T["nf"]
    jobs = S["starts"][S["ofs"][i]:S["ofs"][i] + S["cnt"][i]]
    lead = [t for t in mine if ns[t] > 0] if pivot else []
    q = len(lead)
    assert list(jobs[:q, 0]) == lead and np.all(jobs[:q, 1] == 0) and np.all(jobs[:q, 2] == -1)
    assert np.all(jobs[q:, 2] >= 0)
    first = {}
    for t in mine:
        want = _start_jobs(nf[t])
        mineq = jobs[q:q + len(want)]
        assert [tuple(j[:3]) for j in mineq] == [(t, ch, rb) for ch, rb in want]
        assert np.array_equal(mineq[1:, 3], mineq[:-1, 4]) and np.all(mineq[:, 3] <= mineq[:, 4])      # no gap
        first[t] = tuple(mineq[0, 3:5]) if len(want) else None
        ld = int(nf[t]) + 1
        for node, ch, rb, a0, a1 in mineq:
            col, row = np.divmod(S["apos"][a0:a1].astype(np.int64), ld)
            assert np.all((col >= PB * ch) & (col < PB * ch + PB) & (row >= PB * ch + TB * rb) & (row < PB * ch + TB * rb + TB))
            assert np.all((row >= col) & (row < nf[t]))
        q += len(want)
    assert q == len(jobs)
    for j in jobs[:len(lead)]:      # a pivot job carries the assembly range of the front's chunk 0, row block 0
        assert tuple(j[3:5]) == first[int(j[0])]


def _check_backward(T, S, kn, begin, end, fronts, fused):
    ns, nf, height = T["ns"], T["nf"], T["height"]
    h_top = fused["h_top"] if fused else -1
    i = begin
    for hh in range(len(fronts) - 1, h_top, -1):
        mine = fronts[hh]
        if len(mine) == 0:
            continue
        rect = [(t, ch) for t in mine if nf[t] > ns[t] for ch in range(_ceil(int(ns[t]), 64))] if nf[mine].max() > kn["MGB_BWD_SPLIT_NF"] else []
        if rect:
            assert S["kinds"][i] == "BwdRect" and S["block"][i] == 1024
            assert [tuple(j) for j in S["rects"][S["ofs"][i]:S["ofs"][i] + S["cnt"][i]]] == rect
            i += 1
        assert i < end and S["kinds"][i] == ("Bwd1024" if nf[mine].max() > 384 else "Bwd256"), (hh, i)
        assert list(_launch_nodes(S, i)) == list(mine) and bool(S["rect"][i]) == bool(rect)
        i += 1
    if fused:
        assert S["kinds"][i] == "BwdFused"
        assert (S["cnt"][i], S["lds"][i], S["block"][i]) == (fused["nwg"], fused["lds"], kn["MGB_CHOL_BWD_FUSED_THREADS"])
        i += 1
    assert i == end and "BwdFused" not in S["kinds"][:end - 1]


@pytest.mark.parametrize("kind,L,mesh,variant", _cases(), ids=[R.case_id(*c) for c in _cases()])
def test_chain_plan(monkeypatch, kind, L, mesh, variant):
    T = _tree(monkeypatch, kind, L, R.VARIANTS[variant].get("MGB_LEAF"), mesh)
    kn = R.variant_knobs(variant)
    S = R.plan_schedule(T["p"], T["dim"], kn)
    assert S["world"] == 1 and S["top_fwd"] == len(S["kinds"])
    for table in (R.CASES, R.LARGE):
        if variant in table.get((kind, L, mesh), {}):
            must, never = table[(kind, L, mesh)][variant]
            assert set(must) <= set(S["kinds"]) and not set(never) & set(S["kinds"]), sorted(set(S["kinds"]))
    fused = _fused(T, kn) if kn["MGB_CHOL_BWD_FUSED"] else None
    if fused and (fused["nwg"] == 0 or fused["lds"] > 150 * 1024):
        fused = None
    _check_forward(T, S, kn, 0, S["own_bwd"], T["fronts"], _premap(T, kn))
    _check_backward(T, S, kn, S["own_bwd"], S["top_fwd"], T["fronts"], fused)
    assert len(S["rects"]) == sum(int(c) for k, c in zip(S["kinds"], S["cnt"]) if k == "BwdRect")
    assert np.array_equal(np.sort(S["asrc"]), np.arange(T["nz"]))      # every pattern entry once


@pytest.mark.parametrize("world", [2, 4])
def test_split_plan(monkeypatch, world):
    T = _tree(monkeypatch, "fem2d", 6, None)
    kn = R.variant_knobs("default")
    n, height = len(T["ns"]), T["height"]
    by_height = lambda nodes: [np.array(sorted(t for t in nodes if height[t] == hh), dtype=np.int64) for hh in range(len(T["fronts"]))]
    owner, tops = np.full(n, -2), []
    for rank in range(world):
        S = R.plan_schedule(T["p"], T["dim"], kn, world, rank)
        assert S["world"] == world and "BwdFused" not in S["kinds"] and not S["consumer"].any() and not S["producers"].any()
        nl, ob, tf = len(S["kinds"]), S["own_bwd"], S["top_fwd"]
        own = set(int(t) for i in range(ob, tf) if S["kinds"][i] != "BwdRect" for t in _launch_nodes(S, i))
        tb = next(i for i in range(tf, nl) if S["kinds"][i].startswith("Bwd"))
        top = set(int(t) for i in range(tb, nl) if S["kinds"][i] != "BwdRect" for t in _launch_nodes(S, i))
        assert own and top and not own & top and np.all(owner[list(own)] == -2)
        owner[list(own)] = rank
        tops.append(top)
        _check_forward(T, S, kn, 0, ob, by_height(own), None)
        _check_backward(T, S, kn, ob, tf, by_height(own), None)
        _check_forward(T, S, kn, tf, tb, by_height(top), None)
        _check_backward(T, S, kn, tb, nl, by_height(top), None)
    assert all(t == tops[0] for t in tops)
    owner[list(tops[0])] = -1
    assert np.all(owner >= -1)      # every node: one rank's own list or the top list
