"""The per-node barrier kernels (barrier_f0_kernel, trial_f0_kernel, barrier_rows_F_kernel, barrier_f1_kernel_t,
barrier_f2_kernel_t, expand_hessian_rows_kernel) against exact rows (barrier_reference.py), near the cone boundary and over
the whole barrier menu.  Run with -m gpu -s on an MI355X; profiles/barrier_rows_reference.txt is the output of such a run.

Every figure is a ratio |device - exact| / (u bound) with the reference's own first-order fp64 bound, held to
MARGIN * max(baseline, 1), the baseline being the oracle's fp64 ratio on the same rows (rho_base) or at the same state (level
baseline).  MARGIN is measured, not chosen: worst device ratio over max(baseline, 1) in the first run on
the device, times 4, rounded up to a power of two, capped at 16 (chol_reference.MARGIN: same arithmetic, other operation order --
here the device's pow / log and fma contraction).

First run on an MI355X (MARGIN still at the cap), device ratio / baseline ratio, worst over the classes:

  row sweep, 170 classes (23 cases x 6 regimes x near-active term, 200 rows each, kappa up to 2e11):
      device F, F1 and F2 each 0.00 .. 1.21 against rho_base 0.00 .. 0.91; worst device / max(rho_base, 1) = 1.21
      (cone nq1 K4 p = 1 + 2^-20 at distance 1e-11: device 1.21, oracle 0.86), the same for F, F1 and F2
  golden end points, 7 cases, every level, t = 1e8 and 1e4 (kappa_max 3.5e8 .. 2.4e9):
      f0 and f0_trial <= 0.21, f1 <= 0.75, f2 and the plan path <= 0.75, H v <= 0.60; level baselines f0 <= 0.20, f1 and f2 <= 0.68
  states with an obstacle in contact / term mask / p(x) / slack column: f1 <= 0.72, f2 <= 0.91 (baseline 0.77), H v <= 0.56
  fem2d L = 7 end point and centre (kappa_max 9.9e8): f1 0.79 / 0.81 (baseline 0.76 / 0.83), f0 <= 0.01
  fem2d L = 8 after a device solve (229 376 rows, the separate apply_D + barrier_f0_kernel path; kappa_max 1.1e9): f1 0.85 (baseline 0.86)
  apply_D against the long-double D z: <= 0.25 of the SpMV bound

so MARGIN = 4 x 1.21 rounded up to a power of two = 8.

Row sweep (map_rows of barrier_functions(cones, K), i.e. mgb_map_rows_barrier: the production kernels with unit weights) over
barrier_reference.CASES x REGIMES x near-active term; positions (grid-stride loop past kMaxBlocks, n = 0 included -- the
Python types accept an empty matrix); argument errors for repeated columns inside a power cone; states of the Newton path
through AMG.apply_D / f0 / f0_trial / f1 / f2 / f2_template_f64 / hessian_apply at the golden end points (t = 1e8, kappa up to
2.4e9), at states with a term mask, per-node exponents, an obstacle in contact and the feasibility slack column, and at scale
(fem2d L = 7 and 8).  The Float32 instantiation of the same templates is held to exact rows at float precision, in the range
the float solve works in (t up to 1e4, kappa 8 u32 < 1), by test_gpu_barrier_rows_f32.py."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import barrier_reference as BR
import mgb_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 8.0             # see above; never more than BR.MARGIN = 16
assert MARGIN <= BR.MARGIN
MGB_E_ARG = -1            # include/mgb_hip.h
LD = BR.LD


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


def _device_rows(M, terms, K, Y):
    F, F1, F2 = M.barrier_functions(terms, K)
    hY = M.HPCMatrix(Y)
    n = Y.shape[0]
    f = M.map_rows(F, None, hY).to_numpy()
    f1 = M.map_rows(F1, None, hY).to_numpy().reshape(n, K)
    f2 = M.map_rows(F2, None, hY).to_numpy().reshape(n, K, K)
    return f, f1, f2


# ---------------------------------------------------------------------------------------------------------- row sweep
def test_row_sweep_against_exact_rows(M):
    sweep = list(BR.classes())
    worst = {"F": 0.0, "F1": 0.0, "F2": 0.0}
    failures = []
    print()
    i = 0
    while i < len(sweep):
        K, terms = sweep[i][1], sweep[i][2]
        j = i
        while j < len(sweep) and sweep[j][2] is terms:
            j += 1
        Yall = np.vstack([s[3] for s in sweep[i:j]])
        f, f1, f2 = _device_rows(M, terms, K, Yall)                   # one launch of each kernel for the whole case
        active = sorted({c for t in terms for c in BR.parse(t)["cols"]})
        idle = [c for c in range(K) if c not in active]
        assert np.array_equal(f2, f2.transpose(0, 2, 1)), "F2 rows are symmetric bit for bit"
        assert not f1[:, idle].any() and not f2[:, idle, :].any() and not f2[:, :, idle].any()
        r0 = 0
        for label, _, _, Y in sweep[i:j]:
            sl = slice(r0, r0 + len(Y))
            r0 += len(Y)
            R = BR.reference(terms, Y)
            # classification: no generated row may be left out -- every one is further than 8 u (s^a + |q|^2) from the boundary
            assert float(R.kappa.max()) * 8 * BR.U < 1.0 and np.isfinite(f[sl]).all(), label
            base = BR.rho_base(terms, Y, R)
            dev = (BR.ratio(f[sl], R.F, R.bF), BR.ratio(f1[sl], R.F1, R.bF1), BR.ratio(f2[sl], R.F2, R.bF2))
            print("%-72s n=%3d kappa<=%.1e  device/base  F %5.2f/%4.2f  F1 %5.2f/%4.2f  F2 %5.2f/%4.2f"
                  % (label, len(Y), float(R.kappa.max()), dev[0], base[0], dev[1], base[1], dev[2], base[2]))
            for k, d, b in zip(("F", "F1", "F2"), dev, base):
                worst[k] = max(worst[k], d / max(b, 1.0))
                if not d <= MARGIN * max(b, 1.0):
                    failures.append((label, k, d, b))
        i = j
    print("row sweep: worst device ratio / max(rho_base, 1):  F %.2f  F1 %.2f  F2 %.2f   (MARGIN %g)"
          % (worst["F"], worst["F1"], worst["F2"], MARGIN))
    assert not failures, failures


def test_hand_made_rows_are_outside_exactly(M):
    """Classification: F = +inf exactly on the hand-made rows (phi = 0 exactly, s = 0, s < 0, phi < 0, NaN, half space on and
    past its boundary)."""
    for K, terms, Y, what in BR.hand_made():
        Y = np.array(Y, dtype=np.float64)
        f = M.map_rows(M.barrier_functions(terms, K)[0], None, M.HPCMatrix(Y)).to_numpy()
        assert np.all(np.isposinf(f)), (what, f)
        assert np.all(np.isposinf(BR.reference(terms, Y).F))


# ---------------------------------------------------------------------------------------------------------- positions
def test_every_position_of_the_grid_gives_the_row_of_the_checked_batch(M):
    """Rows are independent: a matrix tiled from a checked batch of m rows must give row q mod m at row q, bit for bit --
    block edges (255, 256, 257), the grid-stride loop past kMaxBlocks = 2048 blocks of 256, and the empty matrix."""
    K, terms = 4, [([1, 2, 3], 1.5), ("linear", [0, 3], [1.0, 0.5], 0.2)]
    Yb = np.vstack([BR.generate(terms, K, near, target, 3, 17, 77 + 10 * near + j)
                    for near in (0, 1) for j, target in enumerate((None, 1e-4, 1e-9))])[:97]
    m = len(Yb)
    assert m == 97
    R = BR.reference(terms, Yb)
    fb, f1b, f2b = _device_rows(M, terms, K, Yb)
    base = BR.rho_base(terms, Yb, R)
    for d, b in zip((BR.ratio(fb, R.F, R.bF), BR.ratio(f1b, R.F1, R.bF1), BR.ratio(f2b, R.F2, R.bF2)), base):
        assert d <= MARGIN * max(b, 1.0)
    for n in (0, 1, 255, 256, 257, 2048 * 256 + 257):
        idx = np.arange(n) % m
        f, f1, f2 = _device_rows(M, terms, K, Yb[idx].reshape(n, K))
        assert f.shape == (n,) and f1.shape == (n, K) and f2.shape == (n, K, K)
        assert np.array_equal(f, fb[idx]) and np.array_equal(f1, f1b[idx]) and np.array_equal(f2, f2b[idx]), n
    print("\npositions: n = 0, 1, 255, 256, 257, %d reproduce the %d checked rows bit for bit" % (2048 * 256 + 257, m))


# ---------------------------------------------------------------------------------------------------------- arguments
@pytest.mark.parametrize("term,what", [(([1, 1, 3], 1.5), "a q column twice"), (([1, 3, 3], 1.5), "s among the q"),
                                       (([1, 2, 3], 1.5, 3), "is2 == is"), (([1, 2, 3], 1.5, 1), "is2 among the q"),
                                       (([2, 0, 2, 3], 2.0), "first and third q equal")])
def test_repeated_columns_in_a_power_cone_are_argument_errors(M, term, what):
    Y = M.HPCMatrix(np.array([[0.5, 0.1, 0.1, 2.0]]))
    for fn in M.barrier_functions([term], 4):
        with pytest.raises(M.MGBError) as e:
            M.map_rows(fn, None, Y)
        assert e.value.code == MGB_E_ARG and "repeated column" in str(e.value), what
    with pytest.raises(M.MGBError) as e:
        M.AMG(M.fem2d_mpi(2), p=1.5, cones=[term])
    assert e.value.code == MGB_E_ARG and "repeated column" in str(e.value), what
    # the same columns in DIFFERENT terms are fine (the intersections of the sweep share columns)
    M.map_rows(M.barrier_functions([([1, 3], 1.5), ([1, 2, 3], 1.5)], 4)[0], None, Y)


# ---------------------------------------------------------------------------------------------------------- states of the path
def _check_state(M, A, gm, Mo, terms, z, c, ts, label, worst, p_node=None, mask=None, levels=None, hessian=True):
    """Every objective / gradient / Hessian entry point of `A` at the state z (n x S), s = 0, against the exact level values at
    the DEVICE's Dz; the level baseline is the oracle's fp64 code at the same state."""
    n, K = A.n, A.K
    zv = np.asarray(z, dtype=np.float64).reshape(-1, order="F")
    A.set_c(c)
    A.set_z(zv)
    ops = {k: v.host for k, v in gm.operators.items()}
    subs = {k: [m.host for m in v] for k, v in gm.subspaces.items()}
    w = gm.w.to_numpy()
    an = None if p_node is None else BR.a_of(p_node)
    mn = None if p_node is None else BR.mu_of(p_node)
    rng = np.random.default_rng(5)
    failures = []
    for l in (range(A.L) if levels is None else levels):
        N = A.level_size(l)[0]
        s0 = np.zeros(N)
        Dfull, B = BR.level_matrices(ops, subs, A.state_variables, A.D, l, n)
        assert B.shape == (n * K, N)
        Dz = A.apply_D(l, s0)
        dz_exact, dz_bound = BR.spmv_reference(Dfull, zv)
        r_dz = BR.ratio(Dz.reshape(-1), dz_exact, dz_bound)
        assert r_dz <= MARGIN, (label, l, "apply_D", r_dz)
        for t in ts:
            rb0, rb1, rb2, Lo = BR.oracle_level_baseline(Mo, l, z, c, t, terms, p_node=p_node, mask=mask, hessian=hessian)
            Lv = BR.level_reference(B, K, w, c, t, Dz, terms, a_node=an, mu_node=mn, mask=mask, hessian=hessian)
            assert Lv.rows.feasible.all(), (label, l)
            y, parts = A.f0(l, s0, t, parts=True)
            res = {"f0F": (BR.ratio(parts[0], Lv.f0F, Lv.b_f0F), rb0), "f0C": (BR.ratio(parts[1], Lv.f0C, Lv.b_f0C), rb0),
                   "f0": (BR.ratio(y, *BR.f0_total(Lv, t)), rb0),
                   "f0_trial": (BR.ratio(A.f0_trial(l, s0, s0, t), *BR.f0_total(Lv, t)), rb0),
                   "f1": (BR.ratio(A.f1(l, s0, t), Lv.g, Lv.b_g), rb1)}
            if hessian:
                Hd, lower = A.f2(l, s0, t)
                Hd = Hd.toarray()
                assert np.array_equal(Hd, Hd.T)
                res["f2"] = (BR.ratio(Hd, Lv.H, Lv.b_H), rb2)
                rp, ci = A.hessian_pattern(l)
                Lo_ = sp.csr_matrix((A.f2_template_f64(l, s0, t), ci, rp), shape=(N, N))
                res["f2 plan"] = (BR.ratio((Lo_ + sp.tril(Lo_, -1).T).toarray(), Lv.H, Lv.b_H), rb2)
                v = rng.standard_normal(N)
                hv, bhv = BR.hessian_apply_reference(Lv, v)
                res["Hv free"] = (BR.ratio(A.hessian_apply(l, s0, v, matrix_free=True), hv, bhv), rb2)
                res["Hv asm"] = (BR.ratio(A.hessian_apply(l, s0, v, matrix_free=False), hv, bhv), rb2)
            kap = np.where(np.isfinite(Lv.rows.kappa), Lv.rows.kappa, 0).max(axis=0)
            print("%-34s l=%d t=%.0e kappa_max %s Dz %.2f | " % (label, l, t, "/".join("%.1e" % float(k) for k in kap), r_dz)
                  + "  ".join("%s %.2f/%.2f" % (k, d, b) for k, (d, b) in res.items()))
            for k, (d, b) in res.items():
                worst[k] = max(worst.get(k, 0.0), d / max(b, 1.0))
                if not d <= MARGIN * max(b, 1.0):
                    failures.append((label, l, t, k, d, b))
    assert not failures, failures


def _default_problem(M, kind, L, p):
    gm = getattr(M, kind + "_mpi")(L)
    go = getattr(O, kind)(L)
    Mo = O.amg(go)
    dim = go.discretization["dim"]
    c = O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), Mo.x)
    return gm, Mo, dim, c


@pytest.mark.parametrize("kind,L,p", BR.SMALL_GOLDENS)
def test_golden_end_points_every_level(M, kind, L, p):
    gold = np.load(os.path.join(HERE, "golden", BR.golden_name(kind, L, p)))
    gm, Mo, dim, c = _default_problem(M, kind, L, p)
    A = M.AMG(gm, p=p)
    ts = gold["ts"]
    worst = {}
    print()
    _check_state(M, A, gm, Mo, BR.default_terms(dim, p), gold["z"], c, (float(ts[-1]), float(ts[len(ts) // 2])),
                 "%s L=%d p=%g" % (kind, L, p), worst)
    print("worst device ratio / max(level baseline, 1): " + "  ".join("%s %.2f" % kv for kv in worst.items()))


def _solved_state(A, c, z0):
    A.set_c(c)
    A.set_z(np.asarray(z0).reshape(-1, order="F"))
    A.prepare()
    A.solve()
    return A.get_z().reshape(np.asarray(z0).shape, order="F")


OBST_G = lambda x: np.array([0.3 + 0.5 * (x[0] ** 2 + x[1] ** 2), 100.0])
OBST_F = lambda x: np.array([5.0, 0.0, 0.0, 1.0])


def test_states_with_mask_node_exponents_obstacle_and_slack_column(M):
    """One state each of the rest of the menu: get_z() after a device solve (it only has to be a state of the path; the check is
    the kernels' values at it)."""
    L = 3
    gm, Mo, dim, c = _default_problem(M, "fem2d", L, 1.0)
    x = Mo.x
    cone15, lin = ([1, 2, 3], 1.5), ("linear", [0], [1.0], -0.1)
    zg = O.map_rows(OBST_G, x)
    cf = O.map_rows(OBST_F, x)
    worst = {}
    print()
    # an obstacle in contact: the half space's kappa is large at the end point
    A = M.AMG(gm, p=1.5, cones=[cone15, lin])
    z = _solved_state(A, cf, zg)
    assert z[:, 0].min() - 0.1 < 1e-3
    _check_state(M, A, gm, Mo, [cone15, lin], z, cf, (1e8, 1e3), "obstacle in contact", worst, levels=(L - 1, 0))
    # a term mask: the obstacle only on x_1 > 0
    select = lambda xi: (True, xi[0] > 0.0)
    mask = np.array([select(xi) for xi in x], dtype=bool)
    A = M.AMG(gm, p=1.5, cones=[cone15, lin], select=select)
    z = _solved_state(A, cf, zg)
    assert z[x[:, 0] < 0, 0].min() < 0.1                               # the masked-out term is violated there
    _check_state(M, A, gm, Mo, [cone15, lin], z, cf, (1e8, 1e3), "term mask", worst, mask=mask, levels=(L - 1, 0))
    # per-node exponents crossing p = 2
    pfun = lambda xi: 1.6 + 0.5 * xi[0]
    pn = np.array([pfun(xi) for xi in x])
    assert set(BR.mu_of(pn)) == {0.0, 1.0, 2.0} or set(BR.mu_of(pn)) == {1.0, 2.0}
    A = M.AMG(gm, p=1.0, cones=[([1, 2, 3], pfun)])
    z = _solved_state(A, c, O.map_rows(lambda xi: O.DEFAULT_G[2](xi), x))
    _check_state(M, A, gm, Mo, [([1, 2, 3], 1.0)], z, c, (1e8, 1e3), "p(x) = 1.6 + 0.5 x", worst, p_node=pn[:, None],
                 levels=(L - 1, 0))
    # the feasibility phase's slack column: (q, s + sigma) in the cone, u + 0.2 + sigma > 0, sigma > -1
    state1 = tuple(M.DEFAULT_STATE) + (("sigma", "full"),)
    D1 = tuple(M.DEFAULT_D[2]) + (("sigma", "id"),)
    terms = [([1, 2, 3], 1.5, 4), ("linear", [0, 4], [1.0, 1.0], 0.2), ("linear", [4], [1.0], 1.0)]
    g = lambda xi: np.array([1.0 - 1.5 * (1.0 - float(np.sum(np.asarray(xi) ** 2)) / 2), 0.05])
    z0 = O.map_rows(g, x)
    Mo1 = O.amg(Mo.geometry, state1, D1)
    Dz0 = O.Barrier.apply_D(Mo.D, z0.reshape(-1, order="F"))
    sigma0 = 1.0 + max(0.0, float(np.max(np.sum(Dz0[:, 1:3] ** 2, axis=1) ** 0.75 - Dz0[:, 3])), float(np.max(-(Dz0[:, 0] + 0.2))))
    c1 = np.column_stack([c, np.full(len(x), 10.0)])
    A = M.AMG(gm, state1, D1, 1.5, cones=terms)
    z = _solved_state(A, c1, np.column_stack([z0, np.full(len(x), sigma0)]))
    _check_state(M, A, gm, Mo1, terms, z, c1, (1e8, 1e3), "slack column (is2), 3 terms", worst, levels=(L - 1, 0))
    print("worst device ratio / max(level baseline, 1): " + "  ".join("%s %.2f" % kv for kv in worst.items()))


def test_at_scale_fem2d_L7(M):
    """large_fem2d_L7_p1_0.npz, end point and polished centre, finest level, f0 and f1."""
    gold = np.load(os.path.join(HERE, "golden", BR.golden_name("fem2d", 7, 1.0, large=True)))
    gm, Mo, dim, c = _default_problem(M, "fem2d", 7, 1.0)
    A = M.AMG(gm, p=1.0)
    worst = {}
    print()
    for name in ("z", "z_centre"):
        _check_state(M, A, gm, Mo, BR.default_terms(dim, 1.0), gold[name], c, (float(gold["ts"][-1]),), "fem2d L=7 p=1 " + name,
                     worst, levels=(6,), hessian=False)
    print("worst device ratio / max(level baseline, 1): " + "  ".join("%s %.2f" % kv for kv in worst.items()))


def test_separate_objective_kernel_beyond_the_fused_range(M):
    """Up to 64 * 2048 rows f0 runs the fused trial_f0_kernel (all the states above); beyond, apply_D and barrier_f0_kernel run
    as separate launches.  fem2d L = 8 (229 376 rows): the state is get_z() after the device solve, finest level, f0 and f1."""
    L = 8
    gm, Mo, dim, c = _default_problem(M, "fem2d", L, 1.0)
    A = M.AMG(gm, p=1.0)
    assert A.n > 64 * 2048
    z = _solved_state(A, c, O.map_rows(lambda xi: O.DEFAULT_G[dim](xi), Mo.x))
    worst = {}
    print()
    _check_state(M, A, gm, Mo, BR.default_terms(dim, 1.0), z, c, (1e8, 1e3), "fem2d L=8 p=1 solved", worst, levels=(L - 1,),
                 hessian=False)
    print("worst device ratio / max(level baseline, 1): " + "  ".join("%s %.2f" % kv for kv in worst.items()))
