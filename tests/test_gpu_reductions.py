"""The grid reductions (dot_kernel, sum_kernel through grid_finish) and spmv_kernel_t<G, double> through the raw types
(HPCVector, HPCSparseMatrix) on exactly summable integer data (linesearch_reference.py): every summation order and every fma
contraction gives the exact integer, and a dropped, doubled or stale element changes it.  So the checks are equalities.

Sizes n = 256 g + r walk the block count g over the edges of grid_finish: one block, the eight ticket shards (7, 8, 9), the
first read-back batch of 4 x 256 partials with its clamped indices (255, 256, 257; 1023, 1024, 1025: the second round), the
block limit (2047, 2048) and the grid-stride loop beyond it (2 * 2048 * 256 + 3)."""
import math

import numpy as np
import pytest

import linesearch_reference as LR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


@pytest.mark.parametrize("g", LR.REDUCTION_GROUPS + (2 * LR.KMAXBLOCKS,))
def test_dot_norm_and_sum_of_integers_are_exact(M, g):
    sizes = [2 * LR.KMAXBLOCKS * LR.KBLOCK + 3] if g == 2 * LR.KMAXBLOCKS else [LR.KBLOCK * g + r for r in (-1, 0, 1)]
    for n in sizes:
        assert n in LR.REDUCTION_SIZES and LR.grid_for(n) == min(g + (n > LR.KBLOCK * g), LR.KMAXBLOCKS)
        x, y = LR.int_vector(n, n), LR.int_vector(n, n + 1)
        hx, hy = M.HPCVector(x), M.HPCVector(y)
        d = hx.dot(hy)
        assert d == LR.exact_dot(x, y), (n, d - LR.exact_dot(x, y))
        assert hy.dot(hx) == d
        s = hx.sum()
        assert s == int(x.astype(np.int64).sum()), n
        nn = LR.exact_dot(x, x)
        assert hx.dot(hx) == nn
        # norm = sqrt of the exact integer, correctly rounded by the host's sqrt: 1 ulp covers a sqrt that is not
        assert abs(hx.norm() - math.sqrt(nn)) <= math.ulp(math.sqrt(nn)), n
        # the last element counts, and only once
        x2 = x.copy()
        x2[-1] += 1.0
        assert M.HPCVector(x2).sum() == s + 1


@pytest.mark.parametrize("n", [257, 1024 * 256 + 1, 2 * 2048 * 256 + 3])
def test_non_finite_values_propagate(M, n):
    x = LR.int_vector(n, 5)
    one = M.HPCVector(np.ones(n))

    def put(**at):
        v = x.copy()
        for i, val in at.items():
            v[int(i)] = val
        return M.HPCVector(v)

    v = put(**{str(n - 1): np.inf})
    assert v.sum() == np.inf and v.dot(one) == np.inf and v.norm() == np.inf
    i = (LR.grid_for(n) - 1) * LR.KBLOCK             # the first entry of the last block
    assert i < n
    v = put(**{str(i): np.nan})
    assert math.isnan(v.sum()) and math.isnan(v.dot(one)) and math.isnan(v.norm())
    v = put(**{"1": np.inf, str(LR.KBLOCK): -np.inf})      # blocks 0 and 1: the partials meet in grid_finish
    assert math.isnan(v.sum()) and math.isnan(v.dot(one)) and v.norm() == np.inf
    v = put(**{"0": -np.inf})
    assert v.sum() == -np.inf and v.norm() == np.inf


@pytest.fixture(scope="module")
def spmv_cases():
    return LR.spmv_cases()


def _spmv_add(M, hA, hx, hy0, hy):
    from mgb_amd import _lib
    _lib.call("mgb_spmv_add", hA.handle, hx.handle, hy0.handle, hy.handle)
    return hy.to_numpy()


@pytest.mark.parametrize("i", range(13))
def test_spmv_on_integer_matrices_is_exact(M, spmv_cases, i):
    assert len(spmv_cases) == 13
    name, A, G = spmv_cases[i]
    assert LR.pick_group(A) == G, name                    # the width this matrix runs at (csrc/amg.cpp pick_group, restated)
    rows, cols = A.shape
    x, y0, v = LR.int_vector(cols, 1), LR.int_vector(rows, 2), LR.int_vector(rows, 3)
    assert LR.spmv_max_sum(A, x, y0) < 2.0 ** 53 and LR.spmv_max_sum(A.T, v) < 2.0 ** 53
    Ai = A.astype(np.int64)
    want = Ai @ x.astype(np.int64)
    hA, hx = M.HPCSparseMatrix(A), M.HPCVector(x)
    assert (hA.host != A).nnz == 0
    y = (hA @ hx).to_numpy()
    assert np.array_equal(y, want), (name, np.flatnonzero(y != want)[:5])
    # y = y0 + A x into a third vector, then with y aliasing y0
    out = _spmv_add(M, hA, hx, M.HPCVector(y0), M.HPCVector(np.full(rows, np.nan)))
    assert np.array_equal(out, want + y0.astype(np.int64)), name
    hy = M.HPCVector(y0)
    out = _spmv_add(M, hA, hx, hy, hy)
    assert np.array_equal(out, want + y0.astype(np.int64)), name
    # the transpose product on the same matrix (the library's own transpose, its own width)
    hT = hA.T
    assert hT.shape == (cols, rows)
    yt = (hT @ M.HPCVector(v)).to_numpy()
    assert np.array_equal(yt, Ai.T @ v.astype(np.int64)), (name, LR.pick_group(A.T))
