"""CPU checks of shard_reference.py, the helper of test_gpu_shard_step.py: the rank shares add up exactly and put nothing on a
foreign rank, the dot bound contains what fp64 gives, and the figures the GPU test's shapes were chosen from come out of the host
plan (geometric tree: mgb_plan_chol_tree + mgb_hostchol_partition; ranked tree: mgb_plan_hostchol_create_ranked +
mgb_hostchol_rank_aligned)."""
import numpy as np
import pytest

import chol_reference as CR
import shard_reference as SR
from test_shard import _full_plan

BLOCK = {"fem1d": 2, "fem2d": 7}
DIM = {"fem1d": 1, "fem2d": 2}


def _pattern(lib, kind, L):
    from mgb_amd import _lib
    h, p, n, S, K, block, N, nz = _full_plan(kind, L, L - 1)
    rp, ci = CR.plan_pattern(p, N, nz)
    _lib.call("mgb_plan_destroy", p)
    _lib.call("mgb_geo_destroy", h)
    return rp, ci, N


def _synthetic_owner(rp, ci, world, ntop, seed):
    """an owner table that is no tree's: regions grown breadth-first over the pattern's graph from `world` random unknowns, ntop
    random top unknowns, and the row of every entry that would still couple two ranks made top as well (a separator)"""
    N = len(rp) - 1
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(N), np.diff(rp))
    nbrs = [[] for _ in range(N)]
    for i, j in zip(rows, ci):
        nbrs[i].append(j)
        nbrs[j].append(i)
    owner = np.full(N, -1)
    front = [int(u) for u in rng.choice(N, world, replace=False)]
    owner[front] = np.arange(world)
    while front:
        nxt = []
        for u in front:
            for v in nbrs[u]:
                if owner[v] < 0:
                    owner[v] = owner[u]
                    nxt.append(v)
        front = nxt
    assert np.all(owner >= 0)
    owner[rng.choice(N, ntop, replace=False)] = -1
    for i, j in zip(rows, ci):
        if owner[i] >= 0 and owner[j] >= 0 and owner[i] != owner[j]:
            owner[i] = -1
    assert all((owner == r).any() for r in range(world))
    return owner


@pytest.mark.parametrize("world", [2, 4, 8])
def test_shares_sum_back_exactly_and_stay_off_foreign_ranks(lib, world):
    rp, ci, N = _pattern(lib, "fem2d", 4)
    a = SR.dyadic(rp, ci, CR.random_spd(rp, ci, seed=5))
    H = CR.full_matrix(rp, ci, a, N)
    off = abs(H).sum(axis=1).A1 - H.diagonal()
    assert np.all(H.diagonal() - off >= 0.25)                      # still diagonally dominant: SPD
    assert np.linalg.eigvalsh(H.toarray()).min() > 0
    owner = _synthetic_owner(rp, ci, world, 10, seed=world)
    sh = SR.split_shares(rp, ci, a, owner, world, seed=3)
    assert sh.shape == (world, len(ci)) and SR.shares_exact(sh, a)
    assert SR.foreign_weight(rp, ci, sh, owner) == 0.0
    rows = np.repeat(np.arange(N), np.diff(rp))
    top = (owner[rows] < 0) & (owner[ci] < 0)
    assert top.any() and np.all(np.count_nonzero(sh[:, top], axis=0) == world)      # every rank holds a part of every top entry
    assert np.all(np.count_nonzero(sh[:, ~top], axis=0) == 1)
    w = np.sort(np.abs(sh[:, top] / a[top]), axis=0)[::-1]
    assert np.array_equal(w, np.repeat(SR.weights(world)[:, None], w.shape[1], axis=1))
    # the permutation varies from entry to entry (two equal halves show none)
    assert world == 2 or len({tuple(np.argsort(-np.abs(sh[:, k]), kind="stable")) for k in np.flatnonzero(top)}) > 1
    # a diagonal entry moved into one rank's share
    u = int(np.flatnonzero(owner < 0)[0])
    sh2, pos = SR.set_diagonal_share(rp, ci, sh, owner, u, -1.0, world - 1)
    assert sh2[:, pos].sum() == -1.0 and sh2[world - 1, pos] == -1.0 and np.array_equal(np.delete(sh2, pos, 1), np.delete(sh, pos, 1))


def test_owner_of_rejects_inconsistent_kind_tables():
    k = np.array([[1, 0, 2, 0], [0, 1, 2, 1]])
    assert SR.owner_of(k).tolist() == [0, 1, -1, 1]
    for bad in ([[1, 0, 2, 0], [0, 1, 0, 1]], [[1, 0, 2, 0], [1, 1, 2, 1]], [[0, 0, 2, 0], [0, 1, 2, 1]]):
        with pytest.raises(ValueError):
            SR.owner_of(np.array(bad))


def test_nodes_without_unknowns_inherit_their_owner():
    """a subtree root may be an empty node that only joins its children; the top starts above it"""
    #        6 (top, 2 unknowns)
    #      2 (empty)    5 (empty, children of two ranks: top)
    #     0   1        3   4
    ns, nf = np.array([2, 2, 0, 1, 1, 0, 2]), np.array([4, 4, 3, 2, 2, 2, 2])
    parent = np.array([2, 2, 6, 5, 5, 6, -1])
    unknown_node = np.array([0, 0, 1, 1, 3, 4, 6, 6])
    owner = np.array([0, 0, 0, 0, 1, 2, -1, -1])
    no = SR.node_owner(ns, parent, unknown_node, owner)
    assert no.tolist() == [0, 0, 0, 1, 2, -1, -1]
    assert SR.subtree_roots(nf, ns, parent, no) == [(2, 0, 3), (3, 1, 1), (4, 2, 1)]
    assert SR.exchange_doubles(SR.subtree_roots(nf, ns, parent, no), 5) == 9 + 2 + 2 + 5
    with pytest.raises(ValueError):
        SR.node_owner(ns, parent, unknown_node, np.array([0, 1, 0, 0, 1, 2, -1, -1]))


@pytest.mark.parametrize("n,scale", [(1, 1.0), (33, 1.0), (770, 1e-3), (12290, 1e6)])
def test_dot_bound_contains_fp64_dots(n, scale):
    rng = np.random.default_rng(n)
    x = scale * rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    y = rng.standard_normal(n)
    for world in (2, 8):
        for got in (np.dot(x, y), float(np.sum(x * y)), float(np.sum((x * y)[::-1])), sum(float(np.dot(a, b)) for a, b in
                    zip(np.array_split(x, world), np.array_split(y, world)))):
            assert SR.dot_ratio(got, x, y, world) <= 1.0
        assert SR.dot_ratio(np.dot(x, x), x, x, world) <= 1.0
    exact, mag = SR.exact_dot(x, y)
    assert SR.dot_ratio(float(exact) + 4 * (n + 10) * SR.U * mag, x, y, 2) > 1.0        # and it is a bound, not a blanket
    ints = np.arange(1.0, n + 1)
    assert SR.exact_dot(ints, ints)[0] == n * (n + 1) * (2 * n + 1) // 6
    assert SR.dot_ratio(1.0, np.array([np.nan, 1.0]), np.ones(2), 2) == np.inf and SR.dot_ratio(np.nan, np.ones(2), np.ones(2), 2) == np.inf
    assert SR.dot_ratio(0.0, np.zeros(3), np.ones(3), 2) == 0.0 and SR.dot_ratio(1e-300, np.zeros(3), np.ones(3), 2) == np.inf


@pytest.mark.parametrize("kind,L", sorted(SR.GEOMETRIC))
def test_shape_table_is_what_the_host_plan_gives(lib, kind, L):
    """Records the figures the shapes of test_gpu_shard_step.py were chosen from and guards that choice."""
    from mgb_amd import _lib
    h, p, n, S, K, block, N, nz = _full_plan(kind, L, L - 1)
    try:
        want_N, geo = SR.GEOMETRIC[(kind, L)]
        assert N == want_N and block == BLOCK[kind]
        for world, want in geo.items():
            got = SR.host_split(p, DIM[kind], world)
            print("%s L=%d world %d geometric: split %d nb %s top unknowns %s" % (kind, L, world, got["split"], got.get("nb"),
                                                                                got.get("top_unknowns")))
            if want is None:
                assert got["split"] == 1
                continue
            assert got["split"] == world and len(got["nb"]) == world
            assert tuple(sorted(set(got["nb"]))) == want[0] or (len(want[0]) == 2 and want[0][0] <= min(got["nb"]) and
                                                                max(got["nb"]) <= want[0][1] and
                                                                {min(got["nb"]), max(got["nb"])} == set(want[0]))
            if want[1] is not None:
                assert got["top_unknowns"] == want[1]
            # how the GPU test finds the subtrees of the geometric tree, where the device hands out no kind table
            assert np.array_equal(SR.geometric_node_owner(got["parent"], world), got["owner"])
        for world, want in zip((2, 4, 8), SR.RANKED_TOP_VALUES[(kind, L)]):
            got = SR.host_split(p, DIM[kind], world, ranked=(K, block))
            print("%s L=%d world %d ranked: split %d aligned %d top values %d" % (kind, L, world, got["split"], got["aligned"],
                                                                                 got["top_values"]))
            assert got["split"] == world and got["aligned"] == 1 and got["top_values"] == want
    finally:
        _lib.call("mgb_plan_destroy", p)
        _lib.call("mgb_geo_destroy", h)
