"""Host-only checks of the tables behind the fused backward sweep of the device Cholesky (csrc/bwd_fused.hpp), through
mgb_plan_chol_bwd_fused: no GPU needed.  For the trees of fem1d / fem2d / fem3d at several L, of fem2d on the coarse meshes of
mesh_cases.py, and several cuts (and a front-size threshold that puts h_top below the root):

  * every front at or below h_top is stored by exactly one workgroup, nothing above h_top is stored;
  * a workgroup's ancestors come in top-down order: the fronts above h_top first (read, not solved), then its path, one
    front per level, then its own subtree parents before children;
  * every boundary entry's LDS slot is the slot of that very unknown, computed (or read) at an earlier level of the same
    workgroup;
  * every slot, slot list and reduction scratch stays inside the LDS allocation the plan asks for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from mesh_cases import MESHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HDR, LEVEL_INTS, JOB_INTS = 8, 4, 16
OFF, LOFF, FIRST, NF, NS, SOFS, BASE, LSOFS, NSL, NT, FLAGS, NODE = 0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13


def _plan_handles(kind, L, mesh=None):
    """(geometry handle, plan handle, dim) of the finest level, as tools/tree_stats.py builds them; mesh: a name of
    mesh_cases.MESHES, the coarse mesh of fem2d"""
    import scipy.sparse as sp
    import mgb_amd as M
    from mgb_amd import _lib
    call, dptr, iptr, f64, i32 = _lib.call, _lib.dptr, _lib.iptr, _lib.f64, _lib.i32
    g = M.fem3d(L, 3) if kind == "fem3d" else (M.fem2d(L, MESHES[mesh]) if mesh is not None else getattr(M, kind)(L))
    dim = {"fem1d": 1, "fem2d": 2, "fem3d": 3}[kind]
    x = f64(np.asarray(g.x).reshape(np.asarray(g.x).shape[0], -1))
    w = f64(g.w)
    Lv = len(g.refine)
    h = C.c_void_p()
    call("mgb_geo_create", x.shape[0], x.shape[1], Lv, 1, dptr(x), dptr(w), C.byref(h))
    for name, S in [("op:" + k, S) for k, S in g.operators.items()] + \
                   [("sub:%s:%d" % (k, l), S) for k, v in g.subspaces.items() for l, S in enumerate(v)]:
        S = sp.csr_matrix(S)
        S.sort_indices()
        rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
        call("mgb_geo_set_matrix", h, name.encode(), S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va))
    state = (("u", "dirichlet"), ("s", "full"))
    D = M.DEFAULT_D[dim]
    K = len(D)
    idx = list(range(K - dim - 1, K))
    iq = (C.c_int * (len(idx) - 1))(*idx[:-1])
    p = C.c_void_p()
    call("mgb_plan_create", h, len(state), _lib.str_array(state), K, _lib.str_array(D), len(idx) - 1, iq, idx[-1], Lv - 1, C.byref(p))
    return h, p, dim


_TREES = {}


def _tree(kind, L, mesh=None):
    if (kind, L, mesh) not in _TREES:
        from mgb_amd import _lib
        h, p, dim = _plan_handles(kind, L, mesh)
        nn = C.c_int()
        _lib.call("mgb_plan_chol_tree", p, dim, 0, C.byref(nn), None, None, None)
        ns, nf, par = (np.zeros(nn.value, dtype=np.int32) for _ in range(3))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _lib.call("mgb_plan_chol_tree", p, dim, nn.value, C.byref(nn), ip(ns), ip(nf), ip(par))
        _TREES[(kind, L, mesh)] = (h, p, dim, ns, nf, par)
    return _TREES[(kind, L, mesh)]


def _fused(kind, L, cut, top_nf, threads, mesh=None):
    from mgb_amd import _lib
    h, p, dim, ns, nf, par = _tree(kind, L, mesh)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    info = np.zeros(12, dtype=np.int32)
    _lib.call("mgb_plan_chol_bwd_fused", p, dim, cut, top_nf, threads, ip(info), 0, None, 0, None, None, 0, None, None)
    h_top, h_cut, nwg, wstride, max_levels, xs_cap, red_cap, sl_cap, lds, nbd, nn, nheights = (int(v) for v in info)
    wg = np.zeros(max(nwg * wstride, 1), dtype=np.int32)
    bdry, slots = np.zeros(max(nbd, 1), dtype=np.int32), np.zeros(max(nbd, 1), dtype=np.int32)
    bofs, first = np.zeros(nn, dtype=np.int32), np.zeros(nn, dtype=np.int32)
    _lib.call("mgb_plan_chol_bwd_fused", p, dim, cut, top_nf, threads, ip(info), nwg * wstride, ip(wg), nbd, ip(bdry), ip(slots),
              nn, ip(bofs), ip(first))
    return dict(h_top=h_top, h_cut=h_cut, nwg=nwg, wstride=wstride, max_levels=max_levels, xs_cap=xs_cap, red_cap=red_cap,
                sl_cap=sl_cap, lds=lds, nheights=nheights, wg=wg, bdry=bdry, slots=slots, bofs=bofs, first=first, ns=ns, nf=nf, par=par)


CASES = [("fem1d", 3), ("fem1d", 7), ("fem2d", 2), ("fem2d", 4), ("fem2d", 5), ("fem2d", 6), ("fem2d", 7), ("fem3d", 2), ("fem3d", 3)]
SETTINGS = [(4, 384, 512), (3, 384, 512), (2, 0, 256), (0, 0, 64), (4, 150, 512), (1, 100, 128), (9, 0, 512)]
# the trees of the coarse meshes of mesh_cases (chol_reference.NEW_TREES): fronts above the default threshold of 384 on top of
# a fused launch (graded4 and graded7 at L = 4), and a root without own columns (two_squares)
MESH_CASES = [("fem2d", 4, "graded4"), ("fem2d", 3, "graded4"), ("fem2d", 4, "graded7"), ("fem2d", 5, "lshape"),
              ("fem2d", 4, "two_squares")]


@pytest.mark.parametrize("kind,L", CASES)
@pytest.mark.parametrize("cut,top_nf,threads", SETTINGS)
def test_fused_backward_tables(kind, L, cut, top_nf, threads):
    _check(_fused(kind, L, cut, top_nf, threads), cut, top_nf, threads)


@pytest.mark.parametrize("kind,L,mesh", MESH_CASES, ids=["%s-%d-%s" % c for c in MESH_CASES])
@pytest.mark.parametrize("cut,top_nf,threads", SETTINGS)
def test_fused_backward_tables_of_coarse_meshes(kind, L, mesh, cut, top_nf, threads):
    _check(_fused(kind, L, cut, top_nf, threads, mesh), cut, top_nf, threads)


def test_default_plans_of_the_graded_meshes_stop_below_the_large_fronts():
    """graded4 and graded7 at L = 4: the heights with a front above 384 rows stay with the per-height launches (Bwd1024), the
    fused launch takes the heights below; the other coarse-mesh trees are fused up to the root"""
    for (kind, L, mesh), above in zip(MESH_CASES, (1, 0, 5, 0, 0)):
        P = _fused(kind, L, 2, 384, 512, mesh)
        assert P["nwg"] >= 1 and P["nheights"] - 1 - P["h_top"] >= above and (above > 0) == (P["h_top"] < P["nheights"] - 1), (mesh, L)


def _check(P, cut, top_nf, threads):
    ns, nf, par, first = P["ns"], P["nf"], P["par"], P["first"]
    n = len(ns)
    height = np.zeros(n, dtype=int)
    for t in range(n):
        if par[t] >= 0:
            assert par[t] > t
            height[par[t]] = max(height[par[t]], height[t] + 1)
    hmax = [int(nf[height == h].max()) for h in range(height.max() + 1)]
    # h_top: the heights below the first one with a front above the threshold
    want_top = -1
    while want_top + 1 < len(hmax) and (top_nf <= 0 or hmax[want_top + 1] <= top_nf):
        want_top += 1
    if want_top < 0:
        assert P["nwg"] == 0
        return
    # h_cut: the knob, raised by at most two heights until there are at most 256 subtrees (one workgroup per CU); a tree
    # that needs more gets no fused launch
    want_cut = min(cut, want_top)
    nroots = lambda c: sum(1 for t in range(n) if height[t] <= c and (par[t] < 0 or height[par[t]] > c))
    raised = 0
    while raised < 2 and want_cut < want_top and nroots(want_cut) > 256:
        want_cut += 1
        raised += 1
    if nroots(want_cut) > 256:
        assert P["nwg"] == 0
        return
    assert P["h_top"] == want_top and P["h_cut"] == want_cut and P["nwg"] == nroots(want_cut) >= 1
    assert P["lds"] == 4 * P["wstride"] + 8 * (P["xs_cap"] + P["red_cap"]) + 4 * P["sl_cap"] and P["wstride"] % 2 == 0
    stored = np.zeros(n, dtype=int)
    W = threads // 64
    jo = HDR + LEVEL_INTS * P["max_levels"]
    for w in range(P["nwg"]):
        rec = P["wg"][w * P["wstride"]:(w + 1) * P["wstride"]]
        nlevels, njobs, first_lv, xs_len, sl_len, sub_lv = (int(v) for v in rec[:6])
        assert 1 <= nlevels <= P["max_levels"] and jo + JOB_INTS * njobs <= P["wstride"]
        assert xs_len <= P["xs_cap"] and sl_len <= P["sl_cap"] and first_lv in (0, 1) and first_lv <= sub_lv < nlevels
        slot_of = {}       # unknown (new ordering) -> (LDS slot, level it becomes available at)
        used = np.zeros(xs_len, dtype=bool)
        seen_jobs, sl_seen = 0, 0
        level_of = {}
        for lv in range(nlevels):
            lofs, cnt, maxp, items = (int(v) for v in rec[HDR + LEVEL_INTS * lv:HDR + LEVEL_INTS * lv + 4])
            assert lofs == seen_jobs and cnt >= 1
            seen_jobs += cnt
            G = W
            while G > 1 and W // G < cnt:
                G //= 2
            if lv >= first_lv:
                assert (W // G) * items <= P["red_cap"]
            for k in range(cnt):
                j = rec[jo + JOB_INTS * (lofs + k):jo + JOB_INTS * (lofs + k + 1)]
                t = int(j[NODE])
                level_of[t] = lv
                assert j[NF] == nf[t] and j[NS] == ns[t] and j[FIRST] == first[t] and j[SOFS] == P["bofs"][t]
                assert 0 <= j[BASE] and j[BASE] + ns[t] <= xs_len
                assert not used[j[BASE]:j[BASE] + ns[t]].any()       # nobody else's slots
                used[j[BASE]:j[BASE] + ns[t]] = True
                above = bool(j[FLAGS] & 2)
                assert above == (height[t] > P["h_top"]) == (lv < first_lv)
                if above:
                    assert not (j[FLAGS] & 1)
                else:
                    nb = nf[t] - ns[t]
                    assert j[LSOFS] == sl_seen and j[LSOFS] + nb <= sl_len
                    sl_seen += nb
                    assert -(-int(ns[t]) // 32) <= maxp and j[NSL] * ns[t] <= items
                    assert (j[NSL] > 0) == (nb > 0 and ns[t] > 0) and j[NT] in (256, 1024)
                    if j[FLAGS] & 1:
                        stored[t] += 1
                    # every boundary entry: the slot of that unknown, available at an earlier level
                    for i in range(nb):
                        g = int(P["bdry"][P["bofs"][t] + i])
                        s = int(P["slots"][P["bofs"][t] + i])
                        assert g in slot_of, (t, g)
                        assert slot_of[g][0] == s and slot_of[g][1] < lv and 0 <= s < xs_len
                    if lv < sub_lv:
                        assert cnt == 1
                for i in range(int(ns[t])):
                    slot_of[int(first[t]) + i] = (int(j[BASE]) + i, lv)
        assert seen_jobs == njobs and sl_seen == sl_len and used.all()
        # levels before sub_lv: the ancestors of the subtree root, top down; behind: the subtree, parents before children
        root = int(rec[jo + JOB_INTS * int(rec[HDR + LEVEL_INTS * sub_lv]) + NODE])
        assert int(rec[HDR + LEVEL_INTS * sub_lv + 1]) == 1 and height[root] <= P["h_cut"]
        assert par[root] < 0 or height[par[root]] > P["h_cut"]
        anc = []
        a = par[root]
        while a >= 0:
            anc.append(int(a))
            a = par[a]
        anc.reverse()
        order = [int(rec[jo + JOB_INTS * q + NODE]) for q in range(int(rec[HDR + LEVEL_INTS * sub_lv]))]
        assert order == anc
        for t, lv in level_of.items():
            if lv > sub_lv:
                assert level_of[int(par[t])] == lv - 1
        sub = [t for t, lv in level_of.items() if lv >= sub_lv]
        assert sorted(sub) == list(range(min(sub), root + 1))      # a contiguous postorder run ending at the root
    want = (height <= P["h_top"]).astype(int)
    assert (stored == want).all()


def test_default_plan_of_the_benchmark_tree_is_one_launch():
    """fem2d L=7: the root is below the default threshold, 256 subtrees of 7 fronts, paths of 8 fronts; a cut of 0 is
    raised to 2 (1 024 leaves, 256 CUs)"""
    P = _fused("fem2d", 7, 2, 384, 512)
    assert P["h_top"] == P["nheights"] - 1 == 10 and P["nwg"] == 256 and P["h_cut"] == 2
    assert _fused("fem2d", 7, 0, 384, 512)["h_cut"] == 2
    for w in range(256):
        rec = P["wg"][w * P["wstride"]:(w + 1) * P["wstride"]]
        assert rec[1] == 8 + 7 and rec[2] == 0 and rec[5] == 8
    assert P["lds"] <= 64 * 1024


def test_trees_too_wide_for_one_round_keep_the_per_height_launches():
    """fem2d L=8 at cut 0: 4 096 leaves, two raises give 1 024 subtrees for 256 CUs: no fused launch; at the default cut
    the same tree gets 256 subtrees of height 4 below h_top = 6"""
    assert _fused("fem2d", 8, 0, 384, 512)["nwg"] == 0
    P = _fused("fem2d", 8, 2, 384, 512)
    assert (P["nwg"], P["h_cut"], P["h_top"]) == (256, 4, 6)
