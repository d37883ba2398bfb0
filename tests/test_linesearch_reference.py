"""CPU checks of linesearch_reference.py itself: the depth-aware bound of the objective sums, the threshold rows of the
fraction-to-the-boundary rule, the exactly summable integer data and the restated pick_group (no GPU)."""
import numpy as np
import pytest

import barrier_reference as BR
import linesearch_reference as LR

LD = BR.LD


def test_launch_shapes_and_depths():
    assert [LR.grid_for(m) for m in (0, 1, 256, 257, 2048 * 256, 2048 * 256 + 1)] == [1, 1, 1, 2, 2048, 2048]
    assert [LR.trial_grid(n) for n in (1, 64, 65, 224, 3584, 131072, 229376)] == [1, 1, 2, 4, 56, 2048, 2048]
    # serial + 6 + 3 + ceil(grid / 256) + 6 + 3
    assert LR.depth_trial(224) == 1 + 9 + 1 + 9 and LR.depth_trial(131072) == 1 + 9 + 8 + 9 == 27
    assert LR.depth_trial(229376) == 2 + 9 + 8 + 9           # 3584 chunks on 2048 blocks: the grid-stride loop
    assert LR.depth_grid_for(224) == 1 + 9 + 1 + 9 and LR.depth_grid_for(2048 * 256 + 1) == 2 + 9 + 8 + 9
    # the block order is a permutation that leaves fewer than 16 blocks and the remainder beyond a multiple of 8 alone
    for nb in (1, 4, 14, 15, 16, 27, 56, 2048):
        slots = [LR.xcd_block(b, nb) for b in range(nb)]
        assert sorted(slots) == list(range(nb))
        assert nb >= 16 or slots == list(range(nb))
        assert slots[nb - nb % 8:] == list(range(nb - nb % 8, nb))
    assert LR.xcd_block(8, 27) == 1 and LR.xcd_block(1, 27) == 3


@pytest.mark.parametrize("n", [1, 63, 224, 896, 1728, 3584, 131072 + 64, 229376])
def test_depth_bound_holds_for_the_documented_order_and_not_without_a_block(n):
    """An fp64 restatement of the kernels' summation order stays inside u depth sum |term| of the long-double sum on random
    terms of mixed sign and size (exact terms: their own bound is zero); the same restatement without one block's partial does
    not."""
    rng = np.random.default_rng(n)
    terms = rng.standard_normal(n) * np.power(10.0, rng.uniform(-3, 3, n))
    exact = terms.astype(LD).sum()
    mag = float(np.abs(terms).astype(LD).sum())
    for restate, depth, grid in ((LR.restate_trial_sum, LR.depth_trial(n), LR.trial_grid(n)),
                                 (LR.restate_grid_for_sum, LR.depth_grid_for(n), LR.grid_for(n))):
        r = BR.ratio(restate(terms), exact, depth * mag)
        assert r <= 1.0, (restate.__name__, n, r)
        # and the any-order bound (n - 1) sum |term| of BR.level_reference is looser by the factor the depth bound removes
        assert n < 64 or (n - 1) / depth > 2.0
        slot = grid // 2
        bad = BR.ratio(restate(terms, drop_slot=slot), exact, depth * mag)
        assert bad > 1e6, (restate.__name__, n, bad)


def test_f0_sums_carry_the_rows_bounds_and_the_depth():
    K, terms = 4, [([1, 2, 3], 1.5), ("linear", [0, 3], [1.0, 0.5], 0.2)]
    Y = BR.generate(terms, K, 0, 1e-4, 3, 300, 5)
    n = len(Y)
    rng = np.random.default_rng(3)
    w, c = rng.uniform(0.1, 1.0, n), rng.standard_normal((n, K))
    R = BR.reference(terms, Y)
    assert R.bphi.shape == (n, 2) and np.all(R.bphi > 0) and np.all(R.bphi >= np.abs(R.phi))      # at least the last rounding
    S1, S9 = LR.f0_sums(R, w, c, Y, 1), LR.f0_sums(R, w, c, Y, 9)
    wl = w.astype(LD)
    assert S1.f0F == (wl * R.F).sum() and S9.f0F == S1.f0F
    assert np.isclose(S9.b_f0F - S1.b_f0F, 8 * float(np.abs(wl * R.F).sum()), rtol=1e-12)
    lin = (c.astype(LD) * Y.astype(LD)).sum(axis=1)
    assert np.isclose(S9.b_f0C - S1.b_f0C, 8 * float(np.abs(wl * lin).sum()), rtol=1e-12)
    # a plain fp64 evaluation in the kernels' order is inside the bound, rows and sums together
    Q = BR.oracle_set(terms)
    F64 = Q.F(None, Y)
    S = LR.f0_sums(R, w, c, Y, LR.depth_trial(n))
    assert BR.ratio(LR.restate_trial_sum(w * F64), S.f0F, S.b_f0F) <= BR.MARGIN
    assert BR.ratio(LR.restate_trial_sum(w * (c * Y).sum(axis=1)), S.f0C, S.b_f0C) <= 1.0
    y, b = LR.f0_total(S, 2.0)
    assert y == S.f0F + 2 * S.f0C and b > S.b_f0F + 2 * S.b_f0C
    assert BR.ratio(LR.oracle_f0(terms, None, w, c, Y), *LR.f0_total(S)) <= BR.MARGIN


def test_threshold_rows_satisfy_their_definition():
    rng = np.random.default_rng(8)
    phi = np.concatenate([rng.uniform(0.0, 1.0, 5000) * np.power(10.0, rng.uniform(-12, 6, 5000)),
                          np.ldexp(1.0, rng.integers(-40, 40, 2500)),                          # powers of two: the spacing changes there
                          np.nextafter(np.ldexp(1.0, rng.integers(-40, 40, 2500)), 0.0)])
    assert len(phi) == 10 ** 4
    for frac in (LR.FRAC, 0.5, 1.0):
        r_le, r_gt, hit = LR.threshold(phi, frac)
        f = np.float64(frac)
        assert np.all(f * r_le <= phi) and np.all(f * r_gt > phi)
        assert np.array_equal(r_gt, np.nextafter(r_le, np.inf))
        assert np.array_equal(hit, f * r_le == phi)
        # the rule itself, as the kernels write it
        assert np.all(phi >= f * r_le) and not np.any(phi >= f * r_gt)
    # frac = 0.1: the products are denser than the doubles around phi only on part of every binade, so not every phi is hit
    hit = LR.threshold(phi, LR.FRAC)[2]
    assert 0.3 < hit.mean() <= 1.0
    assert LR.threshold(phi, 1.0)[2].all() and np.array_equal(LR.threshold(phi, 1.0)[0], phi)


def test_integer_data_is_exactly_summable_at_every_size_in_use():
    assert LR.REDUCTION_SIZES[0] == 255 and LR.REDUCTION_SIZES[-1] == 2 * 2048 * 256 + 3 and len(LR.REDUCTION_SIZES) == 37
    assert max(LR.REDUCTION_SIZES) < LR.INT_MAX_TERMS
    for n in LR.REDUCTION_SIZES:
        x, y = LR.int_vector(n, n), LR.int_vector(n, n + 1)
        for v in (x, y):
            assert np.array_equal(v, np.rint(v)) and np.all(v != 0) and np.abs(v).max() < LR.INT_MAX
        assert float(np.abs(x) @ np.abs(y)) < 2.0 ** 53 and n * LR.INT_MAX ** 2 <= 2 ** 53
        assert LR.exact_dot(x, y) == int((x.astype(LD) * y.astype(LD)).sum())
    for name, A, G in LR.spmv_cases():
        x, y0 = LR.int_vector(A.shape[1], 1), LR.int_vector(A.shape[0], 2)
        v = LR.int_vector(A.shape[0], 3)
        assert np.array_equal(A.data, np.rint(A.data)) and np.all(A.data != 0) and np.abs(A.data).max(initial=0) < LR.INT_MAX
        assert LR.spmv_max_sum(A, x, y0) < 2.0 ** 53 and LR.spmv_max_sum(A.T, v) < 2.0 ** 53, name
        assert np.diff(A.indptr).max() < LR.INT_MAX_TERMS


def test_restated_pick_group_gives_every_width():
    cases = LR.spmv_cases()
    assert [LR.pick_group(A) for _, A, _ in cases[:7]] == [1, 2, 4, 8, 16, 32, 64]
    for name, A, G in cases:
        assert LR.pick_group(A) == G, name
        lens = np.diff(A.indptr)
        assert A.shape[0] == 1 or G == 1 or lens.max() > G // 2, name      # lanes beyond G / 2 hold terms
    by = {name: A for name, A, _ in cases}
    assert np.diff(by["one row of 1000 in a width-2 matrix"].indptr).max() == 1000
    assert (np.diff(by["empty rows between full ones"].indptr) == 0).sum() == 256
    assert by["9000 rows at width 64"].shape[0] * 64 > 2048 * 256
    assert by["cols = 1"].shape[1] == 1 and by["rows = 1"].shape[0] == 1
