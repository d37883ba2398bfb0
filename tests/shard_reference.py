"""Helpers for the checks of the sharded Newton step (test_gpu_shard_step.py, test_shard_reference.py): plain numpy on the CPU.
A helper module, not a test module.

  * matrices whose rank shares add up exactly: dyadic() rounds the values of chol_reference.random_spd to multiples of 2^-20
    and recomputes the diagonal from the rounded values (still SPD by Gershgorin); split_shares() hands an entry with an
    endpoint inside a rank's subtree wholly to that rank and splits an entry among top (separator) unknowns by power-of-two
    weights that sum to one.  The weights are multiples of 2^-7, the values multiples of 2^-20 below 2^6: every share and every
    partial sum of shares is a multiple of 2^-27 below 2^6, 33 bits, so it is exact in fp64 in any order of summation;
  * dots: exact_dot() in rational arithmetic (linesearch_reference.exact_dot is the same idea for integer data; a gradient is not
    integer-valued), dot_bound() = (N + world + 2) u sum |x_i y_i|: N roundings of products and at most N - 1 additions on the
    ranks in any order, world - 1 additions in the collective and one more for the top part, first order in u with the usual
    slack of two;
  * the split of an elimination tree as the exchange kernels see it: subtree roots, their boundary sizes nb, the doubles one
    factorisation exchanges (sum over the roots of nb (nb + 3) / 2 for the packed lower triangle plus the right-hand-side row, and
    the matrix entries among top unknowns that ride along);
  * the shapes the GPU test was planned from (GEOMETRIC, RANKED_TOP_VALUES), reproduced from the host plan by
    test_shard_reference.py."""
import ctypes as C
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
GRID = 2.0 ** -20


def _rows(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


# ---------------------------------------------------------------------------------------------------------- matrices
def dyadic(rp, ci, lower):
    """(a'): the off-diagonal values rounded to multiples of 2^-20, every diagonal entry the absolute sum of the FULL rounded row
    plus the rounded surplus the input had: diagonally dominant, hence SPD, and every value a multiple of 2^-20."""
    rows = _rows(rp)
    N = len(rp) - 1
    off = rows != ci
    v = np.round(np.asarray(lower, dtype=np.float64) / GRID) * GRID
    rowsum0 = np.bincount(rows[off], np.abs(lower[off]), N) + np.bincount(ci[off], np.abs(lower[off]), N)
    surplus = np.round((lower[~off] - rowsum0[rows[~off]]) / GRID) * GRID
    assert np.all(surplus >= 0.25)
    rowsum = np.bincount(rows[off], np.abs(v[off]), N) + np.bincount(ci[off], np.abs(v[off]), N)
    v[~off] = rowsum[rows[~off]] + surplus
    assert np.array_equal(np.round(v / GRID) * GRID, v) and np.abs(v).max() < 64.0
    return v


def owner_of(kinds):
    """kinds: world x N table of the per-rank kind tables (0 = another rank's, 1 = own, 2 = top).  Returns per unknown the rank
    whose kind is 1, or -1 for a top unknown; raises where the tables do not say that."""
    kinds = np.asarray(kinds)
    top = kinds[0] == 2
    if not np.all((kinds == 2) == top[None, :]):
        raise ValueError("the top set differs between the ranks")
    ones = (kinds == 1).sum(axis=0)
    if not np.all(ones[~top] == 1) or not np.all((kinds[:, ~top] == 0).sum(axis=0) == kinds.shape[0] - 1):
        raise ValueError("an unknown outside the top is not owned by exactly one rank")
    return np.where(top, -1, np.argmax(kinds == 1, axis=0))


def weights(world):
    """power-of-two weights that sum to one: (1/2, 1/2), (1/2, 1/4, 1/8, 1/8), ..., the last one doubled"""
    w = [2.0 ** -(k + 1) for k in range(world)]
    w[-1] *= 2
    assert sum(w) == 1.0
    return np.array(w)


def split_shares(rp, ci, lower, owner, world, seed):
    """world x nnz shares of lower-triangle values: an entry with an endpoint owned by a rank goes wholly to that rank (the row's
    owner if both are owned), an entry among top unknowns is split by a per-entry permutation of weights(world)."""
    rng = np.random.default_rng(seed)
    rows = _rows(rp)
    lower = np.asarray(lower, dtype=np.float64)
    shares = np.zeros((world, len(ci)))
    to = np.where(owner[rows] >= 0, owner[rows], owner[ci])
    idx = np.arange(len(ci))
    own = to >= 0
    shares[to[own], idx[own]] = lower[own]
    top = np.flatnonzero(~own)
    w = weights(world)
    perm = np.argsort(rng.random((len(top), world)), axis=1)      # a permutation per entry
    shares[:, top] = (w[perm] * lower[top, None]).T
    return shares


def shares_exact(shares, lower):
    """the shares add up to the values exactly, forwards, backwards and pairwise"""
    fwd = np.zeros(shares.shape[1])
    for s in shares:
        fwd = fwd + s
    bwd = np.zeros(shares.shape[1])
    for s in shares[::-1]:
        bwd = bwd + s
    return np.array_equal(fwd, lower) and np.array_equal(bwd, lower) and np.array_equal(shares.sum(axis=0), lower)


def foreign_weight(rp, ci, shares, owner):
    """largest |share| a rank holds on an entry with an endpoint owned by ANOTHER rank (must be zero)"""
    rows = _rows(rp)
    worst = 0.0
    for r in range(shares.shape[0]):
        foreign = ((owner[rows] >= 0) & (owner[rows] != r)) | ((owner[ci] >= 0) & (owner[ci] != r))
        worst = max(worst, float(np.abs(shares[r, foreign]).max(initial=0.0)))
    return worst


def set_diagonal_share(rp, ci, shares, owner, unknown, value, rank):
    """copies of the shares with the diagonal entry of `unknown` summing to `value`: the whole of it in `rank`'s share, zero in
    the others (for an owned unknown `rank` has to be its owner)"""
    pos = int(np.flatnonzero((ci == unknown) & (_rows(rp) == unknown))[0])
    assert owner[unknown] in (-1, rank)
    out = shares.copy()
    out[:, pos] = 0.0
    out[rank, pos] = value
    return out, pos


# ---------------------------------------------------------------------------------------------------------- dots
def exact_dot(x, y):
    """(sum_i x_i y_i rounded once to long double, sum_i |x_i y_i| in fp64 rounded up a little), in rational arithmetic"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    acc, mag = Fraction(0), Fraction(0)
    for a, b in zip(x.tolist(), y.tolist()):
        p = Fraction(a) * Fraction(b)
        acc += p
        mag += abs(p)
    hi = float(acc)
    return LD(hi) + LD(float(acc - Fraction(hi))), float(mag) * (1 + 2 * U)


def dot_bound(x, y, world):
    return (len(x) + world + 2) * U * exact_dot(x, y)[1]


def dot_ratio(got, x, y, world):
    """|got - <x, y>| / ((N + world + 2) u sum |x_i y_i|); an all-zero dot has to be met exactly"""
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y)) and np.isfinite(got)):
        return np.inf
    exact, mag = exact_dot(x, y)
    err = abs(float(LD(got) - exact))
    if err == 0:
        return 0.0
    return err / ((len(x) + world + 2) * U * mag) if mag > 0 else np.inf


# ---------------------------------------------------------------------------------------------------------- trees
def node_owner(ns, parent, unknown_node, owner):
    """owner per tree node from the owner per unknown (every node's unknowns must agree); a node without unknowns of its own
    belongs to the rank all its children belong to, and to the top otherwise"""
    out = np.full(len(ns), -2)
    for i, t in enumerate(unknown_node):
        if out[t] == -2:
            out[t] = owner[i]
        elif out[t] != owner[i]:
            raise ValueError("tree node %d holds unknowns of different owners" % t)
    assert np.all(out[np.asarray(ns) > 0] != -2)
    for t in range(len(ns)):      # postorder: children first
        if out[t] == -2:
            kids = {int(out[c]) for c in np.flatnonzero(np.asarray(parent) == t)}
            out[t] = kids.pop() if len(kids) == 1 and min(kids) >= 0 else -1
    return out


def geometric_node_owner(parent, world):
    """owner per tree node (postorder) of the geometric split: the nodes log2(world) levels below the root are the subtree roots
    (rank = their order in the postorder), everything above them is top (-1)"""
    nn = len(parent)
    depth = np.zeros(nn, dtype=np.int64)
    for t in range(nn - 1, -1, -1):      # postorder: parents after children
        depth[t] = 0 if parent[t] < 0 else depth[parent[t]] + 1
    cut = int(np.log2(world))
    roots = [t for t in range(nn) if depth[t] == cut]
    out = np.full(nn, -1)
    for t in range(nn):
        a = t
        while depth[a] > cut:
            a = parent[a]
        if depth[a] == cut:
            out[t] = roots.index(a)
    return out


def subtree_roots(nf, ns, parent, nodeown):
    """[(node, rank, nb)] of the subtree roots: owned nodes whose parent is top, nb = nf - ns rows in its Schur complement"""
    return [(t, int(nodeown[t]), int(nf[t] - ns[t])) for t in range(len(ns))
            if nodeown[t] >= 0 and parent[t] >= 0 and nodeown[parent[t]] == -1]


def top_value_count(rp, ci, owner):
    return int(np.count_nonzero((owner[_rows(rp)] < 0) & (owner[ci] < 0)))


def exchange_doubles(roots, ntop_vals):
    return sum(nb * (nb + 3) // 2 for _, _, nb in roots) + ntop_vals


# The shapes the GPU test was planned from, per (kind, L): N, and per world of the GEOMETRIC tree (MGB_RANK_ALIGNED=0) either None
# (the tree does not split) or (sorted set of the subtree roots' nb, top unknowns); per world of the RANKED tree the number of matrix
# entries among top unknowns.  test_shard_reference.py reproduces every figure from the host plan.
GEOMETRIC = {
    ("fem1d", 4): (32, {2: None, 4: None, 8: None}),
    ("fem1d", 7): (256, {2: ((2,), None), 4: ((2, 4), None), 8: None}),
    ("fem2d", 2): (50, {2: None, 4: None, 8: None}),
    ("fem2d", 3): (194, {2: ((16,), 16), 4: ((16,), 30)}),
    ("fem2d", 4): (770, {2: ((32,), None), 4: ((32,), None), 8: ((24, 40), 122)}),
    ("fem2d", 5): (3074, {2: ((64,), 64), 4: ((64,), 126), 8: ((48, 80), 250)}),
    ("fem2d", 6): (12290, {2: ((128,), 128), 4: ((128,), 254), 8: ((96, 160), 506)}),
}
RANKED_TOP_VALUES = {
    ("fem1d", 4): (3, 9, 21), ("fem1d", 7): (3, 9, 21), ("fem2d", 2): (21, 79, 115), ("fem2d", 3): (51, 187, 305),
    ("fem2d", 4): (111, 367, 545), ("fem2d", 5): (231, 727, 1025), ("fem2d", 6): (471, 1447, 1985),
}


def host_split(plan, dim, world, ranked=None):
    """The split of a level's elimination tree from the host plan alone.  ranked = None: the geometric tree; (K, block): the tree
    whose top follows the row partition.  Returns dict(split, nb (per subtree root), top_unknowns, aligned, top_values)."""
    from mgb_amd import _lib
    call = _lib.call
    ch = C.c_void_p()
    if ranked is None:
        call("mgb_plan_hostchol_create", plan, dim, C.byref(ch))
    else:
        call("mgb_plan_hostchol_create_ranked", plan, dim, ranked[0], world, ranked[1], C.byref(ch))
    try:
        sw, nn = C.c_int(), C.c_int()
        call("mgb_hostchol_partition", ch, world, C.byref(sw), 0, C.byref(nn), None)
        owner = np.empty(nn.value, dtype=np.int32)
        call("mgb_hostchol_partition", ch, world, C.byref(sw), nn.value, C.byref(nn), owner.ctypes.data_as(_lib.c_int_p))
        out = dict(split=sw.value, owner=owner)
        if ranked is not None:
            al, ntop = C.c_int(), C.c_int()
            call("mgb_hostchol_rank_aligned", ch, world, C.byref(al), C.byref(ntop))
            out.update(aligned=al.value, top_values=ntop.value)
        else:      # the geometric tree is the plan's own (mgb_plan_chol_tree, same postorder)
            n = C.c_int()
            call("mgb_plan_chol_tree", plan, dim, 0, C.byref(n), None, None, None)
            ns, nf, par = (np.zeros(n.value, dtype=np.int32) for _ in range(3))
            call("mgb_plan_chol_tree", plan, dim, n.value, C.byref(n), _lib.iptr(ns), _lib.iptr(nf), _lib.iptr(par))
            assert n.value == nn.value
            if sw.value > 1:
                roots = subtree_roots(nf, ns, par, owner)
                out.update(nb=[nb for _, _, nb in roots], top_unknowns=int(ns[owner < 0].sum()), parent=par)
        return out
    finally:
        call("mgb_hostchol_destroy", ch)
