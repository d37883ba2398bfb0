"""Host-only checks of the tables behind the pre-mapped child contributions of the device Cholesky (csrc/chol_premap.hpp),
through mgb_plan_chol_premap: no GPU needed.  Over the trees of fem1d L=8, fem2d L=4 / 6 / 7 and fem3d L=2 / 3, and of the
coarse meshes of mesh_cases.py (chol_reference.NEW_TREES: graded and L-shaped meshes, a domain of two components), with the
leaf and single kinds on and off, both consumer modes and a tile limit that bites:

  * for every consumer front and slot the positions (fwd[i], fwd[j]), i >= j, over the child's boundary including its
    right-hand-side row are distinct, lie in the lower part including row nf and inside the slab;
  * the forward map composed with the inverse map (pinv) is the identity, and pinv maps nothing else;
  * slabs of different (front, slot) do not overlap and fill the allocation exactly;
  * a front is a producer iff its parent's launch is a consumer, and stores into its own slot's slab;
  * every consumer launch has only Leaf / Single* children, at least one, and at most `tiles` workgroups;
  * fem1d L=8: parents whose two children sit at different heights (heights 2-4: {0,1}, {1,2}, {2,3}) are consumers."""
import ctypes as C

import numpy as np
import pytest

import chol_reference as R

LEAF, SINGLE, START = 0, 1, 2
TREES = [("fem1d", 8), ("fem2d", 4), ("fem2d", 6), ("fem2d", 7), ("fem3d", 2), ("fem3d", 3)]
MESH_TREES = list(R.NEW_TREES)      # the trees of the coarse meshes of mesh_cases: (kind, L, mesh)
# (leaf, single, mode, tiles)
SETTINGS = [(1, 1, 2, 512), (1, 1, 1, 512), (0, 1, 2, 512), (1, 0, 2, 512), (0, 0, 2, 512), (1, 1, 2, 40), (1, 1, 0, 512),
            (1, 1, 2, 1 << 30)]

_PLANS = {}


def _handles(kind, L, mesh=None):
    if (kind, L, mesh) not in _PLANS:
        h, p, dim, N, nz = R.plan(kind, L, mesh)
        ns, nf, par = R.plan_tree(p, dim)
        _PLANS[(kind, L, mesh)] = (h, p, dim, ns, nf, par)
    return _PLANS[(kind, L, mesh)]


def _premap(kind, L, leaf, single, mode, tiles, mesh=None):
    from mgb_amd import _lib
    h, p, dim, ns, nf, par = _handles(kind, L, mesh)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    info = np.zeros(5, dtype=np.int64)
    args = (p, dim, leaf, single, mode, tiles, lp(info))
    _lib.call("mgb_plan_chol_premap", *args, 0, None, None, None, None, None, None, 0, None, None, None, 0, None, 0, None)
    nn, nh, nfwd, npinv, slab = (int(v) for v in info)
    assert nn == len(ns)
    height, producer, fofs, iofs = (np.zeros(nn, dtype=np.int32) for _ in range(4))
    soff, eoff = np.zeros(2 * nn, dtype=np.int64), np.zeros(nn, dtype=np.int64)
    hkind, hwg, hcons = (np.zeros(nh, dtype=np.int32) for _ in range(3))
    fwd, pinv = np.zeros(max(nfwd, 1), dtype=np.int32), np.zeros(max(npinv, 1), dtype=np.int32)
    _lib.call("mgb_plan_chol_premap", *args, nn, ip(height), ip(producer), lp(soff), lp(eoff), ip(fofs), ip(iofs), nh, ip(hkind),
              ip(hwg), ip(hcons), nfwd, ip(fwd), npinv, ip(pinv))
    return dict(ns=ns, nf=nf, par=par, height=height, producer=producer, soff=soff.reshape(nn, 2), eoff=eoff, fofs=fofs, iofs=iofs,
                hkind=hkind, hwg=hwg, hcons=hcons, fwd=fwd, pinv=pinv, slab=slab)


def _children(par):
    """child slots in the order of the symbolic analysis: children of a node in ascending (postorder) index"""
    ch = [[] for _ in par]
    for t, q in enumerate(par):
        if q >= 0:
            ch[q].append(t)
    return ch


def _check(P, mode, tiles):
    ns, nf, par, height = P["ns"], P["nf"], P["par"], P["height"]
    n, ch = len(ns), _children(par)
    want_h = np.zeros(n, dtype=int)
    for t in range(n):
        if par[t] >= 0:
            assert par[t] > t
            want_h[par[t]] = max(want_h[par[t]], want_h[t] + 1)
    assert np.array_equal(height, want_h)
    hkind, hcons, hwg = P["hkind"], P["hcons"], P["hwg"]
    # the rule, recomputed
    for h in range(len(hkind)):
        fronts = np.flatnonzero(height == h)
        kids = [c for t in fronts for c in ch[t]]
        ok_kind = (hkind[h] == SINGLE and mode >= 1) or (hkind[h] == START and mode >= 2)
        want = ok_kind and len(kids) > 0 and all(hkind[height[c]] in (LEAF, SINGLE) for c in kids) and hwg[h] <= tiles
        assert bool(hcons[h]) == bool(want), (h, hkind[h], hwg[h], want)
        if hkind[h] == LEAF:
            assert hwg[h] == len(fronts) and not kids
    slabs = []
    for t in range(n):
        cons = bool(hcons[height[t]])
        assert len(ch[t]) <= 2
        # producer iff the parent's launch is a consumer; it stores into its own slot's slab of the parent
        if par[t] >= 0:
            pc = bool(hcons[height[par[t]]])
            assert bool(P["producer"][t]) == pc
            slot = ch[par[t]].index(t)
            assert P["eoff"][t] == (P["soff"][par[t], slot] if pc else -1)
        else:
            assert not P["producer"][t] and P["eoff"][t] == -1 and P["fofs"][t] == -1
        for s in range(2):
            if not cons or s >= len(ch[t]):
                assert P["soff"][t, s] == -1
                continue
            c = ch[t][s]
            off, ld, size = int(P["soff"][t, s]), int(nf[t]) + 1, (int(nf[t]) + 1) * int(nf[t])
            assert off >= 0 and off + size <= P["slab"]
            slabs.append((off, off + size))
            nb = int(nf[c] - ns[c])
            fw = P["fwd"][P["fofs"][c]:P["fofs"][c] + nb + 1].astype(np.int64)
            assert fw[nb] == nf[t] and np.all(np.diff(fw) > 0) and fw[0] >= 0      # ascending: i >= j stays i >= j
            a, q = np.meshgrid(np.arange(nb + 1), np.arange(nb), indexing="ij")    # rows incl. the rhs row, columns
            keep = a >= q
            i, j = fw[a[keep]], fw[q[keep]]
            assert np.all(i >= j) and np.all(j < nf[t]) and np.all(i <= nf[t])     # lower part, row nf included
            pos = ld * j + i
            assert len(pos) == 0 or (pos.min() >= 0 and pos.max() < size)          # inside the slab (a child without a
                                                                                   # boundary stores nothing: two_squares' root)
            assert len(np.unique(pos)) == len(pos)                                 # distinct
    # forward o inverse = identity, and the inverse maps nothing else
    for t in range(n):
        if not ch[t]:
            assert P["iofs"][t] == -1
            continue
        ld = int(nf[t]) + 1
        for s in range(2):
            iv = P["pinv"][P["iofs"][t] + s * ld:P["iofs"][t] + (s + 1) * ld]
            if s >= len(ch[t]):
                assert np.all(iv == -1)
                continue
            c = ch[t][s]
            nb = int(nf[c] - ns[c])
            fw = P["fwd"][P["fofs"][c]:P["fofs"][c] + nb + 1]
            assert np.array_equal(iv[fw], np.arange(nb + 1))
            assert np.count_nonzero(iv >= 0) == nb + 1
    # slabs are disjoint and fill the allocation
    slabs.sort()
    end = 0
    for a, b in slabs:
        assert a == end
        end = b
    assert end == P["slab"]


@pytest.mark.parametrize("kind,L", TREES)
@pytest.mark.parametrize("leaf,single,mode,tiles", SETTINGS)
def test_premap_tables(kind, L, leaf, single, mode, tiles):
    P = _premap(kind, L, leaf, single, mode, tiles)
    _check(P, mode, tiles)
    if mode == 0 or (not single and mode < 2):
        assert P["slab"] == 0 and not P["hcons"].any() and not P["producer"].any()
    if not leaf and P["hkind"][0] == START and len(P["hkind"]) > 1:
        assert not P["hcons"][1]      # children from front_start + panel launches: the gather stays


@pytest.mark.parametrize("kind,L,mesh", MESH_TREES, ids=[R.case_id(*c) for c in MESH_TREES])
@pytest.mark.parametrize("leaf,single,mode,tiles", SETTINGS)
def test_premap_tables_of_coarse_meshes(kind, L, mesh, leaf, single, mode, tiles):
    P = _premap(kind, L, leaf, single, mode, tiles, mesh)
    _check(P, mode, tiles)
    if mode == 0 or (not single and mode < 2):
        assert P["slab"] == 0 and not P["hcons"].any() and not P["producer"].any()
    if not leaf and P["hkind"][0] == START and len(P["hkind"]) > 1:
        assert not P["hcons"][1]


def test_expected_consumers_of_the_default_schedules():
    """the launches the GPU cases rely on (tests/test_gpu_chol_premap.py) are consumers in the host plan too"""
    P = _premap("fem2d", 4, 1, 1, 2, 512)
    assert list(P["hkind"]) == [LEAF] + [SINGLE] * 4 and list(P["hcons"]) == [0, 1, 1, 1, 1]
    P = _premap("fem2d", 6, 1, 1, 2, 512)
    assert list(P["hkind"]) == [LEAF] + [SINGLE] * 5 + [START] * 3 and list(P["hcons"]) == [0, 1, 1, 1, 1, 1, 1, 0, 0]
    assert list(_premap("fem2d", 6, 1, 1, 1, 512)["hcons"]) == [0, 1, 1, 1, 1, 1, 0, 0, 0]
    P = _premap("fem2d", 6, 0, 1, 2, 512)
    assert P["hkind"][0] == START and list(P["hcons"][:6]) == [0, 0, 1, 1, 1, 1]
    P = _premap("fem2d", 7, 1, 1, 2, 512)
    assert list(P["hcons"][:7]) == [0, 1, 1, 1, 1, 1, 1] and not P["hcons"][7:].any()
    # the coarse meshes: graded4 has no Leaf height and one Single height above a Start height, so nothing is pre-mapped; the L
    # shape is the square's picture; the two squares' root (no row at all) is a consumer of two children without a boundary
    P = _premap("fem2d", 4, 1, 1, 2, 512, "graded4")
    assert list(P["hkind"]) == [START, SINGLE] + [START] * 7 and not P["hcons"].any() and P["slab"] == 0
    P = _premap("fem2d", 5, 1, 1, 2, 512, "lshape")
    assert list(P["hkind"]) == [LEAF] + [SINGLE] * 4 + [START] * 4 and list(P["hcons"]) == [0, 1, 1, 1, 1, 1, 0, 0, 0]
    P = _premap("fem2d", 4, 1, 1, 2, 512, "two_squares")
    assert list(P["hkind"]) == [LEAF] + [SINGLE] * 4 + [START] and list(P["hcons"]) == [0, 1, 1, 1, 1, 1]
    assert P["ns"][-1] == 0 and P["nf"][-1] == 0 and P["hwg"][-1] == 0
    for L in (2, 3):      # no Leaf / Single* launch at all: nothing is pre-mapped
        P = _premap("fem3d", L, 0, 0, 2, 512)
        assert not (P["hkind"] != START).any() and P["slab"] == 0 and not P["hcons"].any()


def test_children_of_mixed_heights_fem1d():
    """fem1d L=8: heights 2, 3, 4 hold parents whose children sit at heights {0,1}, {1,2}, {2,3}: consumers all the same, and
    the lower child's launch stores pre-mapped for them while its other fronts may have a parent elsewhere"""
    P = _premap("fem1d", 8, 1, 1, 2, 512)
    height, par = P["height"], P["par"]
    ch = _children(par)
    assert list(P["hkind"][:5]) == [LEAF, SINGLE, SINGLE, SINGLE, SINGLE] and list(P["hcons"][:5]) == [0, 1, 1, 1, 1]
    for h, want in ((2, {0, 1}), (3, {1, 2}), (4, {2, 3})):
        mixed = [t for t in np.flatnonzero(height == h) if {int(height[c]) for c in ch[t]} == want]
        assert mixed, (h, want)
        for t in mixed:
            for s, c in enumerate(ch[t]):
                assert P["producer"][c] and P["eoff"][c] == P["soff"][t, s] >= 0
