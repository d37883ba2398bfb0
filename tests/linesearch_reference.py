"""Reference helpers for the line search's objective kernels and the grid reductions (test_linesearch_reference.py,
test_gpu_linesearch.py, test_gpu_reductions.py): plain numpy with long double on top of barrier_reference.py.  A helper
module, not a test module.

Launch shapes, restated from csrc/devutil.hpp and csrc/kernels.hip (kBlock = 256 threads = 4 waves of 64, at most kMaxBlocks =
2048 blocks, kTrialNodes = 64 nodes per chunk of trial_f0_kernel):

  grid_for(m)    = clamp(ceil(m / 256), 1, 2048)      barrier_f0_kernel, dot_kernel, sum_kernel: thread t of block b takes the
                                                      items b 256 + t, + grid 256, ...
  trial_grid(n)  = clamp(ceil(n / 64), 1, 2048)       trial_f0_kernel: the block with slot c (its place in the summation order,
                                                      xcd_block of its index) takes the chunks c, c + grid, ...; lane j of
                                                      wave a adds node j of every such chunk for point a

Every sum then goes through the same tree (block_sum / block_sum_n, grid_finish):

  per thread    the thread's items one after the other              `serial` additions (the first one, to zero, is exact)
  wave_sum      six shuffle steps, lane i += lane i + o, o = 32..1  6
  block_sum     the four waves' values one after the other          3 (the first, to zero, is exact; in trial_f0_kernel three
                                                                      of the four are zero, which only makes additions exact)
  grid_finish   thread i of the last block adds the partials of the
                slots i, i + 256, ... one after the other           ceil(grid / 256)
                wave_sum, block_sum of those                        6 + 3

so no term passes through more than depth = serial + 6 + 3 + ceil(grid / 256) + 6 + 3 rounded additions, and to first order

  |fl(sum) - sum| <= u (sum_q bound(term_q) + depth sum_q |term_q|)

whatever the order inside the tree and whether or not a product is fused into its addition.  At most 27 for the fused kernel
up to 131 072 nodes (2048 blocks, one chunk each) against the n - 1 of an any-order bound.

Threshold rows of the fraction-to-the-boundary rule !(phi >= frac * phi_ref): `threshold(phi, frac)` gives for a device value
phi the largest double r_le with fl(frac * r_le) <= phi and its successor r_gt.  One fp64 multiplication and one comparison
cannot be contracted or reassociated, so numpy and the device agree on both sides exactly.

Exactly summable data: non-zero integers below 2^15 in magnitude and fewer than 2^21 of them per sum keep every partial sum
of products below 2^51 < 2^53: every summation order and every fma contraction gives the exact integer, and a dropped,
doubled or stale element changes it."""
import numpy as np
import scipy.sparse as sp

import barrier_reference as BR

LD = BR.LD
KBLOCK, KMAXBLOCKS, KTRIALNODES = 256, 2048, 64
FRAC = 0.1                    # csrc/amg.hpp kFracToBoundary
INT_MAX = 2 ** 15             # integer data: 0 < |x| < INT_MAX
INT_MAX_TERMS = 2 ** 21


def _cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------- launch shapes
def grid_for(items):
    return min(max(_cdiv(items, KBLOCK), 1), KMAXBLOCKS)


def trial_grid(n):
    return min(max(_cdiv(n, KTRIALNODES), 1), KMAXBLOCKS)


def xcd_block(b, nb):
    """csrc/devutil.hpp: the position block b of nb works on."""
    if nb < 16:
        return b
    per = nb >> 3
    return (b & 7) * per + (b >> 3) if b < (per << 3) else b


def _finish_depth(grid):
    return 6 + 3 + _cdiv(grid, KBLOCK) + 6 + 3


def depth_grid_for(m):
    """Longest chain of additions of a sum over m items launched with grid_for(m) blocks (barrier_f0_kernel over the nodes,
    dot_kernel / sum_kernel over the entries): serial = ceil(m / (grid 256)) items per thread, then the tree above."""
    grid = grid_for(m)
    return _cdiv(max(m, 1), grid * KBLOCK) + _finish_depth(grid)


def depth_trial(n):
    """The same for trial_f0_kernel over n nodes: serial = ceil(chunks / grid) chunks per block, one node of each per lane."""
    grid = trial_grid(n)
    return _cdiv(_cdiv(max(n, 1), KTRIALNODES), grid) + _finish_depth(grid)


# ---------------------------------------------------------------------------------------------------------- fp64 restatements
def _wave_sum(v):
    """v: (..., 64) -> lane 0 after the six shuffle steps (lanes past the end read their own value; they never reach lane 0)."""
    v = np.array(v, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :64 - o] = v[..., :64 - o] + v[..., o:]
    return v[..., 0]


def _block_sum(v):
    """v: (..., 256) per-thread values -> thread 0's block sum."""
    w = _wave_sum(v.reshape(v.shape[:-1] + (4, 64)))
    r = np.zeros(w.shape[:-1])
    for i in range(4):
        r = r + w[..., i]
    return r


def _finish(partials, drop_slot=None):
    """grid_finish: partials in slot order -> the launch's result."""
    grid = len(partials)
    p = np.zeros(_cdiv(grid, KBLOCK) * KBLOCK)
    p[:grid] = partials
    if drop_slot is not None:
        p[drop_slot] = 0.0
    acc = np.zeros(KBLOCK)
    for row in p.reshape(-1, KBLOCK):
        acc = acc + row
    return float(_block_sum(acc))


def restate_grid_for_sum(terms, drop_slot=None):
    """fp64 sum of `terms` in the order of barrier_f0_kernel / dot_kernel / sum_kernel.  drop_slot: leave that block's partial
    out (a wrong restatement, for the test of the bound)."""
    terms = np.asarray(terms, dtype=np.float64)
    grid = grid_for(len(terms))
    serial = _cdiv(max(len(terms), 1), grid * KBLOCK)
    t = np.zeros(serial * grid * KBLOCK)
    t[:len(terms)] = terms
    acc = np.zeros((grid, KBLOCK))
    for row in t.reshape(serial, grid, KBLOCK):
        acc = acc + row
    return _finish(_block_sum(acc), drop_slot)


def restate_trial_sum(terms, drop_slot=None):
    """fp64 sum of per-node `terms` in the order of trial_f0_kernel (one point)."""
    terms = np.asarray(terms, dtype=np.float64)
    grid = trial_grid(len(terms))
    serial = _cdiv(_cdiv(max(len(terms), 1), KTRIALNODES), grid)
    t = np.zeros(serial * grid * KTRIALNODES)
    t[:len(terms)] = terms
    lane = np.zeros((grid, KTRIALNODES))
    for row in t.reshape(serial, grid, KTRIALNODES):
        lane = lane + row
    return _finish(_wave_sum(lane), drop_slot)       # the point's wave holds the only non-zero values of its block


# ---------------------------------------------------------------------------------------------------------- objective sums
class Sums:
    pass


def f0_sums(rows, w, c, Dz, depth):
    """Exact (sum_q w_q F_q, sum_q w_q <c_q, Dz_q>) at the rows Dz with the depth-aware bounds of the module docstring.  `rows`:
    BR.reference(terms, Dz, ...) (or the .rows of a BR.level_reference at the same Dz).  Term bounds as in
    BR.level_reference: w (bF + |F|) for w F and w ((K + 1) sum_k |c_k Dz_k| + |<c, Dz>|) for w <c, Dz>."""
    Dz = np.ascontiguousarray(Dz, dtype=np.float64)
    K = Dz.shape[1]
    wl, cl, Dl = np.asarray(w, dtype=LD), np.asarray(c, dtype=LD), Dz.astype(LD)
    S = Sums()
    wF = wl * rows.F
    S.f0F = wF.sum()
    S.b_f0F = float((wl * (rows.bF + np.abs(rows.F))).sum() + depth * np.abs(wF).sum())
    lin = (cl * Dl).sum(axis=1)
    S.f0C = (wl * lin).sum()
    S.b_f0C = float((wl * ((K + 1) * np.abs(cl * Dl).sum(axis=1) + np.abs(lin))).sum() + depth * np.abs(wl * lin).sum())
    S.depth = depth
    return S


def f0_total(S, t=1.0):
    """(f0F + t f0C, its bound), as BR.f0_total."""
    y = S.f0F + LD(t) * S.f0C
    return y, S.b_f0F + abs(t) * S.b_f0C + abs(float(LD(t) * S.f0C)) + abs(float(y))


def oracle_f0(terms, x, w, c, Dz, mask=None):
    """The oracle's fp64 objective (oracle/mgb_oracle.py Barrier.f0, t = 1) at the rows Dz: the yardstick of the sums."""
    import mgb_oracle as O
    n, K = Dz.shape
    Bo = O.Barrier(BR.oracle_set(terms, None, mask))
    with np.errstate(all="ignore"):
        return Bo.f0(np.zeros(1), x, w, c, None, [None] * K, None, pre=(Dz, [sp.csr_matrix((n, 1))] * K))


# ---------------------------------------------------------------------------------------------------------- the rule
def threshold(phi, frac=FRAC):
    """(r_le, r_gt, hit): r_le the largest double with fl(frac * r_le) <= phi, r_gt its successor, hit = fl(frac * r_le) == phi.
    phi finite, frac in (0, 1]."""
    phi = np.asarray(phi, dtype=np.float64)
    frac = np.float64(frac)
    with np.errstate(all="ignore"):
        r = phi / frac
        for _ in range(64):
            high = frac * r > phi
            if not high.any():
                break
            r = np.where(high, np.nextafter(r, -np.inf), r)
        assert not (frac * r > phi).any()
        for _ in range(64):
            up = np.nextafter(r, np.inf)
            more = frac * up <= phi
            if not more.any():
                break
            r = np.where(more, up, r)
        r_gt = np.nextafter(r, np.inf)
        assert not (frac * r_gt <= phi).any()
    return r, r_gt, frac * r == phi


# ---------------------------------------------------------------------------------------------------------- integer data
def int_vector(n, seed):
    """n non-zero integers with |x| < 2^15 as doubles."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, INT_MAX, n) * rng.choice([-1, 1], n)).astype(np.float64)


REDUCTION_GROUPS = (1, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048)
REDUCTION_SIZES = sorted({KBLOCK * g + r for g in REDUCTION_GROUPS for r in (-1, 0, 1)} | {2 * KMAXBLOCKS * KBLOCK + 3})


def exact_dot(x, y):
    """The integer sum_i x_i y_i of integer-valued doubles (int64 cannot overflow: below 2^51 by construction)."""
    xi, yi = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    assert np.array_equal(xi, x) and np.array_equal(yi, y) and int(np.abs(xi).max(initial=0)) * int(np.abs(yi).max(initial=0)) * len(xi) < 2 ** 62
    return int(np.dot(xi, yi))


def pick_group(A):
    """csrc/amg.cpp pick_group: lanes per row, the first power of two that is at least the mean row length (at most 64)."""
    A = sp.csr_matrix(A)
    if A.shape[0] == 0:
        return 1
    avg = A.nnz / A.shape[0]
    g = 1
    while g < 64 and g < avg:
        g <<= 1
    return g


def int_csr(rows, cols, row_lengths, seed):
    """Integer-valued CSR: row i has row_lengths[i] distinct columns, values non-zero with |a| < 2^15."""
    rng = np.random.default_rng(seed)
    row_lengths = np.asarray(row_lengths, dtype=np.int64)
    assert row_lengths.shape == (rows,) and row_lengths.max(initial=0) <= cols
    indptr = np.r_[0, np.cumsum(row_lengths)]
    indices = np.concatenate([np.sort(rng.choice(cols, m, replace=False)) for m in row_lengths] + [np.zeros(0, dtype=np.int64)])
    data = int_vector(int(indptr[-1]), seed + 1)
    return sp.csr_matrix((data, indices.astype(np.int32), indptr.astype(np.int32)), shape=(rows, cols))


def spmv_cases():
    """(name, A, lanes per row the library must pick) for the SpMV test: every width, and the shapes of the issue."""
    out = []
    for G in (1, 2, 4, 8, 16, 32, 64):       # every row exactly G long (G = 64: 64 and 65): the mean is what pick_group stops at
        rows = 300 + G
        out.append(("width %d" % G, int_csr(rows, 97 + 2 * G, np.full(rows, G) + (np.arange(rows) % 2 if G == 64 else 0), 100 + G), G))
    lens = np.ones(2000, dtype=np.int64)
    lens[1234] = 1000
    out.append(("one row of 1000 in a width-2 matrix", int_csr(2000, 1500, lens, 201), 2))
    out.append(("empty rows between full ones", int_csr(513, 64, np.where(np.arange(513) % 2 == 0, 14, 0), 202), 8))
    out.append(("rows = 1", int_csr(1, 300, [100], 203), 64))
    out.append(("rows = 1, one nonzero", int_csr(1, 3, [1], 204), 1))
    out.append(("9000 rows at width 64", int_csr(9000, 257, 33 + np.arange(9000) % 9, 205), 64))
    out.append(("cols = 1", int_csr(700, 1, np.arange(700) % 3 != 0, 206), 1))
    return out


def spmv_max_sum(A, x, y0=None):
    """Largest sum of magnitudes any row's sum can pass through."""
    A = sp.csr_matrix(A)
    m = abs(A) @ np.abs(x)
    if y0 is not None:
        m = m + np.abs(y0)
    return float(m.max(initial=0.0))
