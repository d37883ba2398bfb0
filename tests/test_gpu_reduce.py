"""The finish launch of the two-stage field reductions (csrc/reduce.hpp, csrc/reduce.hip) alone, through
the test hook mgb_reduce_selftest, bit for bit against a numpy replay of its fixed order:
  1. thread t of 256 folds its run of ceil(nwg / 256) consecutive partials in ascending order, starting from the identity
     (0, 0, 0, 0, -inf);
  2. per wave of 64, level o = 32, 16, .., 1 folds lane t + o into lane t for t < o;
  3. waves 1, 2, 3 are folded into wave 0 in that order.
A fold adds the three sum columns and takes the NaN-sticky maximum of the other two.

The meshes of the module tests give at most 4 workgroups; here nwg = 1, 2 (one partial, a partial wave), 255, 256, 257 (the run
length goes from 1 to 2), 513 and 1000 (runs of 3 and 4; at 513 the last 85 threads have empty runs), each with one row and with a
grid of three rows.  The sum columns carry mixed signs over twelve decades, so that another order shows in the last bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
THREADS, COLS = 256, 5
NWG = (1, 2, 255, 256, 257, 513, 1000)


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


def finish(M, partials):
    from mgb_amd._lib import call, dptr
    rows, nwg, cols = partials.shape
    assert cols == COLS and partials.flags.c_contiguous and partials.dtype == np.float64
    out = np.full((rows, COLS), 123.0)
    call("mgb_reduce_selftest", M.backend_hip().handle, rows, nwg, dptr(partials), dptr(out))
    return out


def fold(acc, c):
    """acc, c: (..., 5); combine of reduce.hpp"""
    out = acc.copy()
    out[..., :3] = acc[..., :3] + c[..., :3]
    m, v = acc[..., 3:], c[..., 3:]
    out[..., 3:] = np.where((v > m) | (v != v), v, m)
    return out


def replay(partials):
    rows, nwg, _ = partials.shape
    chunk = (nwg + THREADS - 1) // THREADS
    out = np.empty((rows, COLS))
    with np.errstate(invalid="ignore"):
        for r in range(rows):
            acc = np.zeros((THREADS, COLS))
            acc[:, 4] = -np.inf
            for j in range(chunk):
                g = np.arange(THREADS) * chunk + j
                live = g < nwg
                acc[live] = fold(acc[live], partials[r, g[live]])
            acc = acc.reshape(THREADS // 64, 64, COLS)
            o = 32
            while o > 0:
                acc[:, :o] = fold(acc[:, :o], acc[:, o:2 * o])
                o //= 2
            res = acc[0, 0]
            for w in range(1, THREADS // 64):
                res = fold(res, acc[w, 0])
            out[r] = res
    return out


def partials_of(rows, nwg, seed, negative=False):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((rows, nwg, COLS)) * 10.0 ** rng.uniform(-6.0, 6.0, (rows, nwg, COLS))
    p[..., 3] = np.abs(p[..., 3])
    p[..., 4] = -np.abs(p[..., 4]) - 1e-300 if negative else np.abs(p[..., 4])
    return p


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("rows", (1, 3))
@pytest.mark.parametrize("nwg", NWG)
def test_finish_is_the_replay_bit_for_bit(M, nwg, rows):
    p = partials_of(rows, nwg, 1000 * rows + nwg)
    out, ref = finish(M, p), replay(p)
    assert np.array_equal(bits(out), bits(ref)), (out, ref)


@pytest.mark.parametrize("nwg", (1, 257, 513))
def test_a_negative_second_maximum_survives(M, nwg):
    """every value of column 4 is strictly negative: a zero seed in any thread, empty runs included, would come out as 0"""
    p = partials_of(3, nwg, 77 + nwg, negative=True)
    out = finish(M, p)
    assert np.array_equal(bits(out), bits(replay(p)))
    assert np.array_equal(out[:, 4], p[..., 4].max(axis=1)) and (out[:, 4] < 0.0).all()
    assert np.array_equal(out[:, 3], p[..., 3].max(axis=1))


@pytest.mark.parametrize("col", range(COLS))
def test_a_nan_in_the_last_partial_stays_in_its_column_and_row(M, col):
    nwg, rows, row = 513, 3, 1
    p = partials_of(rows, nwg, 5)
    clean = finish(M, p)
    p[row, nwg - 1, col] = np.nan
    out = finish(M, p)
    assert np.isnan(out[row, col])
    keep = np.ones((rows, COLS), dtype=bool)
    keep[row, col] = False
    assert np.array_equal(bits(out)[keep], bits(clean)[keep])


def test_bad_arguments_are_refused(M):
    from mgb_amd._lib import MGBError, call, dptr
    p, out = np.zeros((1, 1, COLS)), np.zeros((1, COLS))
    for rows, nwg in ((0, 1), (1, 0)):
        with pytest.raises(MGBError):
            call("mgb_reduce_selftest", M.backend_hip().handle, rows, nwg, dptr(p), dptr(out))
