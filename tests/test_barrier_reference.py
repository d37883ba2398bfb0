"""The reference machinery of the barrier-row check (barrier_reference.py) on the CPU, on every run:

  * the long-double rows against a 60-digit evaluation (mpmath; the only place it is imported): ratio <= 2^-8 -- long
    double's unit roundoff is 2^-11 u, the factor 8 is for the few operations behind an entry;
  * the fp64 baseline: the oracle's F / F1 / F2 on every class of the sweep; its worst ratio per class is rho_base, the
    yardstick the device kernels are held to in test_gpu_barrier_rows.py.  A correctly rounded fp64 evaluation has ratio
    <= 1 to first order; numpy's pow / log are within an ulp, so rho_base <= 4 pins the bound model (measured: 0.0 .. 1.2);
  * the case table covers what the issue of the check lists;
  * the level propagation on the committed goldens: oracle f0 / f1 / f2 in fp64 at the golden z against the exact values;
  * the matrix-free H v reference (three keyed sums, for levels too large for a dense H) against the dense one on small levels:
    both are long-double sums of the same products in another order, so they differ by long-double roundings of terms the
    bound already counts at fp64's u = 2^11 long-double ulps: held to 4 long-double ulps of the bound, a ratio of 2^-9;
  * the float working precision (prec = BR.F32, the yardstick of test_gpu_barrier_rows_f32.py): the conditions of the float
    sweep (floats inside RANGE32, kappa 8 u32 < 1, every class keeps 40 % of its rows), the float baseline rows_f32 against the
    float bound (ratio <= 2; measured 0.0 .. 1.30), three planted errors in rows_f32 far outside it, and the hand-made rows
    whose class is decided by the rounding to float."""
import os

import numpy as np
import pytest

import barrier_reference as BR
import mgb_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
RHO_BASE_MAX = 4.0
MP_ROWS = 24          # rows of every class that go through mpmath (more than 200 per case of the table)


# ---------------------------------------------------------------------------------------------------------- 60 digits
def _mp_rows(terms, Y, a_node=None, mu_node=None, mask=None):
    """F, F1, F2 of every row at 60 digits, written separately from barrier_reference (scalar code, one row at a time)."""
    import mpmath as mp
    mp.mp.dps = 60
    n, K = Y.shape
    outF, outG, outH = [], [], []
    for r in range(n):
        y = [mp.mpf(float(v)) for v in Y[r]]
        F, G, H = mp.mpf(0), [mp.mpf(0)] * K, [[mp.mpf(0)] * K for _ in range(K)]
        G = list(G)
        inside = True
        for ti, term in enumerate(terms):
            if mask is not None and not mask[r, ti]:
                continue
            if term[0] == "linear":
                _, idx, coef, off = term
                phi = mp.mpf(float(off)) + sum(mp.mpf(float(c)) * y[i] for i, c in zip(idx, coef))
                if not phi > 0:
                    inside = False
                    continue
                F -= mp.log(phi)
                for i, ci in zip(idx, coef):
                    G[i] -= mp.mpf(float(ci)) / phi
                    for j, cj in zip(idx, coef):
                        H[i][j] += mp.mpf(float(ci)) * mp.mpf(float(cj)) / phi ** 2
                continue
            idx, p = term[0], term[1]
            a = mp.mpf(float(BR.a_of(p))) if a_node is None else mp.mpf(float(a_node[r, ti]))
            mu = mp.mpf(float(BR.mu_of(p))) if mu_node is None else mp.mpf(float(mu_node[r, ti]))
            qi, scols = list(idx[:-1]), [idx[-1]] + ([term[2]] if len(term) > 2 else [])
            s = sum(y[c] for c in scols)
            if not s > 0:
                inside = False
                continue
            phi = s ** a - sum(y[c] ** 2 for c in qi)
            if not phi > 0:
                inside = False
                continue
            F -= mp.log(phi) + mu * mp.log(s)
            ds, dds = a * s ** (a - 1), a * (a - 1) * s ** (a - 2)
            gs = -ds / phi - mu / s
            hss = -dds / phi + ds ** 2 / phi ** 2 + mu / s ** 2
            for c in qi:
                G[c] += 2 * y[c] / phi
                for c2 in qi:
                    H[c][c2] += 4 * y[c] * y[c2] / phi ** 2 + (2 / phi if c == c2 else 0)
                for cs in scols:
                    H[c][cs] -= 2 * y[c] * ds / phi ** 2
                    H[cs][c] -= 2 * y[c] * ds / phi ** 2
            for cs in scols:
                G[cs] += gs
                for cs2 in scols:
                    H[cs][cs2] += hss
        outF.append(F if inside else mp.inf)
        outG.append(G)
        outH.append(H)
    return outF, outG, outH


def _ld(x):
    """An mpmath number as a long double (head + tail of two doubles)."""
    import mpmath as mp
    if mp.isinf(x):
        return BR.LD(np.inf)
    hi = float(x)
    return BR.LD(hi) + BR.LD(float(x - mp.mpf(hi)))


def _mp_ratio(terms, Y, R, **kw):
    mF, mG, mH = _mp_rows(terms, Y, **kw)
    n, K = Y.shape
    F = np.array([_ld(v) for v in mF], dtype=BR.LD)
    G = np.array([[_ld(v) for v in row] for row in mG], dtype=BR.LD).reshape(n, K)
    H = np.array([[[_ld(v) for v in r2] for r2 in row] for row in mH], dtype=BR.LD).reshape(n, K, K)
    assert np.array_equal(np.isinf(F), np.isinf(R.F))
    fin = np.isfinite(F)
    return max(BR.ratio(R.F, F, R.bF, fin), BR.ratio(R.F1, G, R.bF1, fin), BR.ratio(R.F2, H, R.bF2, fin))


@pytest.fixture(scope="module")
def sweep():
    return list(BR.classes())


def test_case_table_covers_the_menu():
    terms = [BR.parse(t) for _, _, ts in BR.CASES for t in ts]
    cones = [t for t in terms if t["kind"] == 0]
    halves = [t for t in terms if t["kind"] == 1]
    assert {len(t["q"]) for t in cones} == {1, 2, 3} and {len(t["q"]) for t in halves} == {1, 2, 3}
    assert {len(t["q"]) for t in cones if t["s2"] >= 0} == {1, 2, 3}                   # is2 set, with every nq
    assert {len(ts) for _, _, ts in BR.CASES} == {1, 2, 3}
    assert {K for _, K, _ in BR.CASES} == {2, 4, 5, 8}
    assert {t["p"] for t in cones} == {1.0, BR.P_NEAR_ONE, 1.5, 2.0, 3.0, 8.0}
    assert any(t["cols"] != sorted(t["cols"]) for t in cones) and any(t["cols"] != sorted(t["cols"]) for t in halves)
    assert any(np.any(np.diff(sorted(t["cols"])) > 1) for t in cones)                  # non-contiguous
    assert any(min(t["coef"]) < 0 < max(t["coef"]) for t in halves)                    # mixed signs
    shared = [ts for _, _, ts in BR.CASES if len(ts) > 1 and
              sum(len(BR.parse(t)["cols"]) for t in ts) > len({c for t in ts for c in BR.parse(t)["cols"]})]
    assert len(shared) >= 3
    assert any(K != len(BR.parse(ts[0])["cols"]) + 1 for _, K, ts in BR.CASES)         # K other than dim + 2
    assert [r[0] for r in BR.REGIMES[:4]] == ["1e0", "1e-4", "1e-8", "1e-11"]


def test_generated_rows_are_inside_at_the_asked_distance(sweep):
    for label, K, terms, Y in sweep:
        assert len(Y) >= 40, label
        R = BR.reference(terms, Y)
        assert R.feasible.all() and R.in_range.all() and np.isfinite(R.F).all(), label
        assert float(R.dist.min()) >= BR.MIN_DIST, label


def test_long_double_rows_match_60_digits(sweep):
    worst = 0.0
    for label, K, terms, Y in sweep:
        Y = Y[:MP_ROWS]
        worst = max(worst, _mp_ratio(terms, Y, BR.reference(terms, Y)))
        assert worst <= 2.0 ** -8, label
    K, terms, Y, pn = BR.node_exponent_rows()
    Y, pn = Y[::4], pn[::4]
    an, mn = BR.a_of(pn), BR.mu_of(pn)
    assert set(mn.ravel()) == {0.0, 1.0, 2.0}
    worst = max(worst, _mp_ratio(terms, Y, BR.reference(terms, Y, a_node=an, mu_node=mn), a_node=an, mu_node=mn))
    K, terms, Y, mask = BR.piecewise_rows()
    worst = max(worst, _mp_ratio(terms, Y[::3], BR.reference(terms, Y[::3], mask=mask[::3]), mask=mask[::3]))
    for K, terms, Y, what in BR.hand_made():
        Y = np.array(Y, dtype=np.float64)
        mF = _mp_rows(terms, Y)[0]
        assert all(np.isinf(float(v)) for v in mF) and np.all(np.isposinf(BR.reference(terms, Y).F)), what
    print("long double rows against 60 digits: worst ratio %.2e (allowed 2^-8 = %.2e)" % (worst, 2.0 ** -8))
    assert worst <= 2.0 ** -8


def test_fp64_baseline_rows(sweep):
    """rho_base of every class: the oracle's fp64 rows against the reference."""
    worst = [0.0, 0.0, 0.0]
    for label, K, terms, Y in sweep:
        r = BR.rho_base(terms, Y, BR.reference(terms, Y))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= RHO_BASE_MAX, (label, r)
    K, terms, Y, pn = BR.node_exponent_rows()
    r = BR.rho_base(terms, Y, BR.reference(terms, Y, a_node=BR.a_of(pn), mu_node=BR.mu_of(pn)), p_node=pn)
    assert max(r) <= RHO_BASE_MAX, ("per-node p", r)
    worst = [max(a, b) for a, b in zip(worst, r)]
    K, terms, Y, mask = BR.piecewise_rows()
    R = BR.reference(terms, Y, mask=mask)
    assert np.isfinite(R.F).all()                                    # the violated half space is masked out on those rows
    r = BR.rho_base(terms, Y, R, mask=mask)
    assert max(r) <= RHO_BASE_MAX, ("piecewise", r)
    worst = [max(a, b) for a, b in zip(worst, r)]
    print("fp64 baseline (oracle rows): worst ratio F %.2f  F1 %.2f  F2 %.2f" % tuple(worst))


def test_a_wrong_formula_is_far_outside_the_bound():
    """The check has teeth on the CPU too: the q-s slot with the wrong sign is a ratio of 1e6 and more in every regime of a
    p = 1.5 cone.  Dropping mu / s^2 from hss is one at order-one distances and still far outside at 1e-4; closer to the
    boundary that term sinks below the rounding of ds^2 / phi^2 next to it (its share is about (phi / s^a)^3 / u bounds), so
    only the order-one regime can see it -- which is why the sweep keeps that regime for every case."""
    terms = [([1, 2, 3], 1.5)]
    for target in (None, 1e-4, 1e-8):
        Y = BR.generate(terms, 4, 0, target, 3, 100, 5)
        R = BR.reference(terms, Y)
        H = BR.oracle_set(terms).F2(None, Y)
        bad = H.copy()
        bad[:, 3, 3] -= 1.0 / Y[:, 3] ** 2
        assert BR.ratio(H, R.F2, R.bF2) <= RHO_BASE_MAX
        if target is None or target >= 1e-4:
            assert BR.ratio(bad, R.F2, R.bF2) > (1e6 if target is None else 16 * RHO_BASE_MAX)
        bad = H.copy()
        bad[:, 1, 3] *= -1
        assert BR.ratio(bad, R.F2, R.bF2) > 1e6


@pytest.mark.parametrize("kind,L,p", BR.SMALL_GOLDENS)
def test_level_baseline_on_the_goldens(kind, L, p):
    """Oracle f0 / f1 / f2 in fp64 at the golden z, t = ts[-1] and ts[len // 2], every level, against the exact values: the
    level baseline.  Measured 0.05 .. 1.1; the any-order summation bound is pessimistic by design, 4 pins it."""
    gold = np.load(os.path.join(HERE, "golden", BR.golden_name(kind, L, p)))
    go = getattr(O, kind)(L)
    Mo = O.amg(go)
    dim = go.discretization["dim"]
    c = O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), Mo.x)
    terms = BR.default_terms(dim, p)
    ts = gold["ts"]
    for t in (float(ts[-1]), float(ts[len(ts) // 2])):
        for l in range(L):
            r0, r1, r2, Lv = BR.oracle_level_baseline(Mo, l, gold["z"], c, t, terms)
            kap = float(Lv.rows.kappa.max())
            print("%s L=%d p=%g t=%.0e level %d: kappa_max %.1e  baseline ratio f0 %.2f f1 %.2f f2 %.2f" % (kind, L, p, t, l, kap, r0, r1, r2))
            assert Lv.rows.feasible.all()
            assert max(r0, r1, r2) <= RHO_BASE_MAX


# ---------------------------------------------------------------------------------------------------------- float
RHO_BASE32_MAX = 2.0      # rows_f32 against the float bound: the same kind of constant as RHO_BASE_MAX (measured: 0.0 .. 1.30)
P32 = BR.F32


@pytest.fixture(scope="module")
def sweep32():
    return list(BR.classes(prec=P32))


def test_float_sweep_rows_are_floats_inside_at_the_asked_distance(sweep32):
    """The conditions of the float sweep, none of them a measurement: the regimes are the stated ones, every row is a float32
    inside every term and inside RANGE32, no closer than MIN_DIST32, with kappa 8 u32 < 1 (the first-order bound means
    something), and every class keeps at least 40 % of the 200 rows asked for (measured: 63.5 % in the worst class)."""
    assert BR.U32 == 2.0 ** -24 and BR.RANGE32 == (2.0 ** -100, 2.0 ** 100) and BR.MIN_DIST32 == 1e-5
    assert BR.REGIMES32 == [("1e0", None, 3), ("1e-2", 1e-2, 3), ("1e-4", 1e-4, 3), ("1e0 wide", None, 8), ("1e-3 wide", 1e-3, 8)]
    singles = sum(1 for _, _, ts in BR.CASES if len(ts) == 1)
    assert len(sweep32) == 5 * singles + 3 * sum(len(ts) for _, _, ts in BR.CASES if len(ts) > 1)
    share = 1.0
    for label, K, terms, Y in sweep32:
        assert np.array_equal(Y, Y.astype(np.float32).astype(np.float64)), label
        assert len(Y) >= 0.4 * 200, (label, len(Y))
        share = min(share, len(Y) / 200.0)
        R = BR.reference(terms, Y, prec=P32)
        assert R.feasible.all() and R.in_range.all() and np.isfinite(R.F).all(), label
        assert float(R.dist.min()) >= BR.MIN_DIST32, label
        assert float(R.kappa.max()) * 8 * BR.U32 < 1.0, label
        for x in (R.F1, R.F2):
            ax = np.abs(x[x != 0]).astype(np.float64)
            assert ax.size == 0 or (ax.min() >= BR.RANGE32[0] and ax.max() <= BR.RANGE32[1]), label
    print("float sweep: %d classes, %d rows, smallest share of a class %.1f %%"
          % (len(sweep32), sum(len(s[3]) for s in sweep32), 100 * share))


def test_float_reference_reads_what_the_kernels_read():
    """The float reference rounds its inputs itself: doubles and their float roundings give the same rows, bit for bit; a is
    float32(fl(2 / p)), and a - 2 carries float's rounding where float rounds it (p = 8: a = 0.25 is exact, p = 3: a = 2/3 is
    not and a - 2 loses a bit)."""
    terms = [([1, 2, 3], 3.0), ("linear", [0, 3], [0.1, 0.7], 0.3)]
    rng = np.random.default_rng(1)
    Y = np.column_stack([rng.uniform(0.5, 1.0, 50), rng.uniform(-0.3, 0.3, (50, 2)), rng.uniform(1.0, 2.0, 50)])
    R = BR.reference(terms, Y, prec=P32)
    R32 = BR.reference(terms, Y.astype(np.float32).astype(np.float64), prec=P32)
    for k in ("F", "bF", "F1", "bF1", "F2", "bF2"):
        assert np.array_equal(getattr(R, k), getattr(R32, k)), k
    assert R.feasible.all() and not np.array_equal(R.F, BR.reference(terms, Y).F)
    a = np.array([np.float32(BR.a_of(3.0))], dtype=np.float64)
    assert float(BR.a_minus(a, 2, P32).e[0]) > 0 and float(BR.a_minus(a, 2).e[0]) == 0
    assert float(BR.a_minus(np.array([0.25]), 2, P32).e[0]) == 0 and float(BR.a_minus(np.array([0.25]), 1, P32).e[0]) == 0
    # the coefficients 0.1 and 0.7 and the offset 0.3 are rounded as the kernels cast them
    h = BR.reference([("linear", [0], [0.1], 0.3)], np.array([[1.0]]), prec=P32)
    assert h.phi[0, 0] == BR.LD(np.float32(0.1)) + BR.LD(np.float32(0.3))


def test_float_baseline_rows(sweep32):
    """rho_base32 of every class: the plain numpy float32 restatement of the kernels' formulas against the float reference."""
    worst = [0.0, 0.0, 0.0]
    for label, K, terms, Y in sweep32:
        r = BR.rho_base32(terms, Y, BR.reference(terms, Y, prec=P32))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= RHO_BASE32_MAX, (label, r)
    K, terms, Y, pn = BR.node_exponent_rows(prec=P32)
    an, mn = BR.a_of(pn), BR.mu_of(pn)
    assert set(mn.ravel()) == {0.0, 1.0, 2.0} and len(Y) >= 0.4 * 7 * 60
    R = BR.reference(terms, Y, a_node=an, mu_node=mn, prec=P32)
    assert R.feasible.all() and R.in_range.all() and float(R.kappa.max()) * 8 * BR.U32 < 1.0
    r = BR.rho_base32(terms, Y, R, a_node=an, mu_node=mn)
    assert max(r) <= RHO_BASE32_MAX, ("per-node p", r)
    worst = [max(a, b) for a, b in zip(worst, r)]
    K, terms, Y, mask = BR.piecewise_rows(prec=P32)
    R = BR.reference(terms, Y, mask=mask, prec=P32)
    assert np.isfinite(R.F).all() and len(Y) >= 0.4 * 240 and (Y[~mask[:, 1], 0] < 0.25).any()
    assert float(np.where(np.isfinite(R.kappa), R.kappa, 0).max()) * 8 * BR.U32 < 1.0
    r = BR.rho_base32(terms, Y, R, mask=mask)
    assert max(r) <= RHO_BASE32_MAX, ("piecewise", r)
    worst = [max(a, b) for a, b in zip(worst, r)]
    print("float baseline (rows_f32): worst ratio F %.2f  F1 %.2f  F2 %.2f" % tuple(worst))


def test_mutated_float_restatements_are_far_outside_the_float_bound(sweep32):
    """Teeth of the float check: rows_f32 with one planted error -- the output slots of a term's first q column and its last
    column swapped, mu off by one, the exponent a - 1 where a - 2 belongs (in dds) -- against the float bound.  A mutation
    applies to a class if it changes a formula there: the slot swap everywhere, mu where there is a power cone, a - 1 where
    there is a power cone with a != 1 (for p = 2 the kernels set dds = 0).  Every mutation that applies has a ratio of at least
    1e3 in every order-one class (measured: 1.3e6 and more); in every 1e-4 class the slot swap and mu are beyond BR.MARGIN
    (measured: 8.4e2 and more), and so is the worst of the three.

    The exponent in dds alone cannot be held to that at 1e-4 where its own cone is the near-active term: dds / phi is
    (a - 1) / a dist times ds^2 / phi^2, the term beside it in hss, whose own bound is about 2 kappa u = 4 u / dist of it; a
    relative error e in dds is a ratio of about e |a - 1| / a dist^2 / (4 u), i.e. 0.04 e |a - 1| / a at dist = 1e-4 and
    u = 2^-24, with e = |1 - s| up to 1e3 on these rows.  Measured there: 4.4 .. 1.1e2 (printed below), and 0.88 where a half
    space on the cone's slack column is the near-active term (its coef^2 / phi^2 sits in the same entry) -- the same effect as
    for mu / s^2 in test_a_wrong_formula_is_far_outside_the_bound, and the reason why every case keeps its order-one and 1e-2
    regimes, where this mutation is a ratio of 1.7e3 and more."""
    near_dds = []
    for label, K, terms, Y in sweep32:
        regime = label.split(" | ")[1]
        if regime not in ("1e0", "1e0 wide", "1e-4"):
            continue
        R = BR.reference(terms, Y, prec=P32)
        cones = [BR.parse(t) for t in terms if t[0] != "linear"]
        applies = {"slot": True, "mu": bool(cones), "a-1": any(np.float32(BR.a_of(T["p"])) != 1 for T in cones)}
        r = {m: max(BR.rho_base32(terms, Y, R, mutate=m)) for m in applies}
        for m, on in applies.items():
            if not on:
                assert r[m] <= RHO_BASE32_MAX, (label, m)                 # nothing to mutate: the restatement itself
            elif regime != "1e-4":
                assert r[m] >= 1e3, (label, m, r[m])
            elif m != "a-1":
                assert r[m] > BR.MARGIN, (label, m, r[m])
            else:
                near_dds.append((label, r[m]))
        if regime == "1e-4":
            assert max(r.values()) > BR.MARGIN, (label, r)
    print("a - 1 for a - 2 at 1e-4: " + "; ".join("%s: %.1e" % lr for lr in near_dds))


def test_rows_decided_by_the_rounding_to_float_classify_as_stated():
    """The hand-made rows of the float classification check: what is exactly outside stays outside, rows that are strictly
    inside in double but on or outside the boundary after the rounding to float are +inf in float and finite in double, rows
    inside by more than the float bound of phi are finite -- in the reference and in rows_f32 alike."""
    n = 0
    for K, terms, Y, what in BR.hand_made():
        Y = np.array(Y, dtype=np.float64)
        Y = Y[BR.float_representable(Y)]
        n += len(Y)
        assert np.all(np.isposinf(BR.reference(terms, Y, prec=P32).F)) and np.all(np.isposinf(BR.rows_f32(terms, Y)[0])), what
    assert n >= 13                                                         # only the rows with a 0.1 are not floats
    for K, terms, row, outside, what in BR.rounding_rows():
        Y = np.array([row], dtype=np.float64)
        assert not BR.float_representable(Y)[0], what
        R64, R32 = BR.reference(terms, Y), BR.reference(terms, Y, prec=P32)
        assert R64.feasible[0] and np.isfinite(R64.F[0]), what
        f32 = BR.rows_f32(terms, Y)[0][0]
        if outside:
            assert not R32.feasible[0] and float(R32.phi.min()) <= 0 and np.isposinf(R32.F[0]) and np.isposinf(f32), what
        else:
            assert R32.feasible[0] and np.all(np.abs(R32.phi[0]) > BR.U32 * R32.bphi[0]) and np.isfinite(f32), what


MATRIX_FREE_ULPS = 4.0 * 2.0 ** -11      # 4 long-double ulps (2^-64) in units of u = 2^-53, relative to the bound


@pytest.mark.parametrize("kind,L,p", [("fem1d", 4, 2.0), ("fem2d", 2, 1.5), ("fem3d", 2, 1.0)])
def test_matrix_free_hessian_apply_matches_the_dense_reference(kind, L, p):
    """hessian_apply_matrix_free against hessian_apply_reference at a golden state, every level, for a random vector and a unit
    vector: values to 4 long-double ulps of the bound, and the two bounds equal up to the fp64 rounding of their own sums."""
    import scipy.sparse as sp
    gold = np.load(os.path.join(HERE, "golden", BR.golden_name(kind, L, p)))
    go = getattr(O, kind)(L)
    Mo = O.amg(go)
    dim = go.discretization["dim"]
    K = len(Mo.D)
    c = O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), Mo.x)
    terms = BR.default_terms(dim, p)
    t = float(gold["ts"][len(gold["ts"]) // 2])
    rng = np.random.default_rng(3)
    worst = 0.0
    for l in range(L):
        _, _, _, Lv = BR.oracle_level_baseline(Mo, l, gold["z"], c, t, terms)
        B = BR.interleave([sp.csr_matrix(Dk @ Mo.R[l]) for Dk in Mo.D])
        N = B.shape[1]
        e = np.zeros(N)
        e[N // 2] = 1.0
        for v in (rng.standard_normal(N), e):
            hv, bhv = BR.hessian_apply_reference(Lv, v)
            hm, bhm = BR.hessian_apply_matrix_free(B, K, Mo.w, Lv.rows, v)
            assert hm.dtype == BR.LD and np.all(bhv[hv != 0] > 0)
            worst = max(worst, BR.ratio(hm, hv, bhv))
            assert np.allclose(bhm, bhv, rtol=1e-12, atol=0.0)
            he, bhe = BR.hessian_apply_matrix_free(B, K, Mo.w, Lv.rows, v, rows_per_el=K * go.discretization["block"])
            assert BR.ratio(he, hv, bhv) <= MATRIX_FREE_ULPS and np.all(bhe >= bhm)      # r from the elements: never smaller
        # teeth: one nonzero of B dropped (a lost element entry, a wrong slot) is far outside the bound, pessimistic as it is
        Bd = B.copy()
        in_cone = np.repeat(np.arange(B.shape[0]) % K == K - 1, np.diff(B.indptr))      # the slack row of D: in every default cone
        Bd.data[int(np.argmax(np.abs(Bd.data) * in_cone))] = 0.0
        hd, _ = BR.hessian_apply_matrix_free(Bd, K, Mo.w, Lv.rows, np.ones(N))
        teeth = BR.ratio(hd, *BR.hessian_apply_reference(Lv, np.ones(N)))
        print("level %d: one dropped nonzero of B: ratio %.1e" % (l, teeth))
        assert teeth > 1e3 * BR.MARGIN * RHO_BASE_MAX
        d, bd = BR.diag_reference(Lv)
        assert np.array_equal(d, np.diagonal(Lv.H)) and np.all(d > 0) and np.all(bd >= (K + 2) * d)
    print("%s L=%d: matrix-free against dense H v, worst ratio %.2e (allowed %.2e)" % (kind, L, worst, MATRIX_FREE_ULPS))
    assert worst <= MATRIX_FREE_ULPS
