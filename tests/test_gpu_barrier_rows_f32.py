"""The Float32 instantiation of the Newton-path templates (csrc/kernels_f32.hip: spmv_t<float>, barrier_f0_rows_kernel_t<float>,
barrier_f1_kernel_t<float>, barrier_f2_kernel_t<float>, convert_kernel) against exact rows at float precision, through the
production entry points AMG.f0_f32 / f1_f32 / f2_f32 that drive amgb(..., T=np.float32).  Run with -m gpu -s on an MI355X;
profiles/barrier_rows_f32_reference.txt is the output of such a run.

Every figure is a ratio |device - exact| / (u32 bound), u32 = 2^-24, with barrier_reference's first-order bound for the floats
the kernels read (prec = BR.F32), held to MARGIN32 * max(baseline, 1).  The baseline is BR.rows_f32 / BR.level_f32 -- the
kernels' formulas in plain numpy float32 -- on the same rows or at the same state.  MARGIN32 is measured, not chosen: worst
device ratio over max(baseline, 1) in the first run on the device, times 4, rounded up to a power of two, capped at
BR.MARGIN = 16.

First run on an MI355X (MARGIN32 still at the cap), device ratio / baseline ratio, worst over the classes:

  row sweep, 135 classes (23 cases x 5 float regimes x near-active term, 200 rows each but 127 .. 175 in two, kappa up to 2e4),
  both deliveries, t = 1 and 1e4:
      f1 0.00 .. 1.15 and f2 0.00 .. 1.14 against baselines up to 1.19 / 1.18; f0F <= 0.13, f0C <= 0.02 (their bounds carry
      the any-order sum over 64 rows); worst device / max(baseline, 1) = 1.15 (cone nq1 K4 p = 1 + 2^-20 at distance 1e-2:
      device 1.15, numpy float32 0.92)
  per-node exponents crossing p = 2 and a per-row term mask: f1 and f2 <= 0.68 (baseline 0.70), f0F <= 0.18
  positions, fem2d L = 4 (896 nodes, levels 3 and 0) and fem1d L = 2 (8 nodes): f1 and f2 <= 0.48 (baseline 0.79), f0F <= 0.19
  end states of the five float solves, every level, t = 1e4 and 1e2 (kappa_max 3.5e4 .. 1.6e5, kappa 8 u32 <= 0.077):
      f1 <= 0.73, f2 <= 0.72, f0F <= 0.06, the baselines the same within 0.1
  states with an obstacle in contact / term mask / p(x) / slack column at tol = sqrt(eps32) (kappa_max 1.6e5 .. 2.2e5,
  kappa 8 u32 <= 0.104): f1 <= 0.77, f2 <= 0.69 (baselines up to 0.97)

so MARGIN32 = 4 x 1.15 rounded up to a power of two = 8.

The identity layout.  The "id" operator of every geometry is the identity, and on fem3d L = 1 the "full" subspace is the 64 x 64
identity.  An AMG with K state variables ("v0", "full") .. and D = (("v0", "id"), ..) therefore has Dz0 = exactly the n x K state
given to set_z, B = a 0/1 matrix (the identity on the cube), f1_f32 = w (F1 + t c) row by row, f2_f32 = the node blocks of
w F2 through the Hessian plan and f0_f32 = the two row sums.  Every batch of the row sweep is delivered twice -- through z with
s = 0 (the convert kernel and the Dz0_32 base of the float SpMV) and through s with z = 0 (the float SpMV with unit entries,
exact) -- and both deliveries must agree bit for bit.

f0_f32 returns f0F + t f0C only.  f0F is the value at t = 0; f0C is read off (f0_f32(t = 2^60) - f0F) / 2^60 in long double: the
product by 2^60 is exact and the one double rounding of the sum is 2^-53 (|f0C| + 2^-60 |f0F|), 2^-29 of the unit the ratio is
measured in.

What is not repeated here: the grid-stride loop past 2048 blocks needs more than 524 288 rows.  It is the template's loop,
test_gpu_barrier_rows.py covers it in double, and the bit-for-bit *_template_f64 checks of test_gpu_parity.py tie the two
instantiations together.  Symmetry of the f2 node blocks holds by construction here: f2_f32 returns one triangle.  Where a batch
holds an infeasible row nothing is asserted about f1_f32 or f2_f32: their content there is unspecified.  The limits of the
float path (RANGE32, kappa 8 u32 < 1) are barrier_reference's; the float solve menu (obstacle, mask or p(x) problems under
T = float32) is not part of this check, only the float kernels at such states."""
import numpy as np
import pytest
import scipy.sparse as sp

import barrier_reference as BR
import mgb_oracle as O

pytestmark = pytest.mark.gpu

P32, U32, LD = BR.F32, BR.U32, BR.LD
MARGIN32 = 8.0            # see above; never more than BR.MARGIN = 16
assert MARGIN32 <= BR.MARGIN
T_PART = 2.0 ** 60        # f0C = (f0_f32(t = 2^60) - f0_f32(t = 0)) / 2^60
TS = (1.0, 1e4)
TOL32 = float(np.sqrt(np.finfo(np.float32).eps))
BATCH = 64


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


@pytest.fixture(scope="module")
def cube(M):
    gm = M.fem3d_mpi(1)
    assert gm.x.shape[0] == BATCH
    return gm


def f32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


_HOST = {}


def _host(gm):
    """Host copies of a geometry's matrices and weights, once per geometry."""
    if id(gm) not in _HOST:
        _HOST[id(gm)] = (gm, {k: v.host for k, v in gm.operators.items()}, {k: [m.host for m in v] for k, v in gm.subspaces.items()},
                         gm.w.to_numpy())
    return _HOST[id(gm)][1:]


class Problem:
    """An AMG with the host side the reference needs: B of a level, the weights."""

    def __init__(self, A, gm):
        self.A, self.gm, self.n, self.K = A, gm, A.n, A.K
        self.ops, self.subs, self.w = _host(gm)
        self._B = {}

    def B(self, l):
        if l not in self._B:
            self._B[l] = BR.level_matrices(self.ops, self.subs, self.A.state_variables, self.A.D, l, self.n)[1]
        return self._B[l]


def identity_problem(M, gm, K, terms, **kw):
    state = tuple(("v%d" % k, "full") for k in range(K))
    D = tuple(("v%d" % k, "id") for k in range(K))
    return Problem(M.AMG(gm, state, D, 1.0, cones=terms, **kw), gm)


class Tally:
    def __init__(self):
        self.worst, self.failures = {}, []

    def add(self, label, dev, base):
        for k, d in dev.items():
            b = base[k]
            self.worst[k] = max(self.worst.get(k, 0.0), d / max(b, 1.0))
            if not d <= MARGIN32 * max(b, 1.0):
                self.failures.append((label, k, d, b))

    def done(self, what):
        print("%s: worst device ratio / max(baseline, 1): " % what + "  ".join("%s %.2f" % kv for kv in sorted(self.worst.items()))
              + "   (MARGIN32 %g)" % MARGIN32)
        assert not self.failures, self.failures


def device_level(A, l, s, ts=TS, hessian=True):
    """(f0F, f0C, {t: g}, dense float32 H) of the float entry points at level l and the float32 unknowns s."""
    s = np.ascontiguousarray(s, dtype=np.float32)
    yF, yT = A.f0_f32(l, s, 0.0), A.f0_f32(l, s, T_PART)
    yC = float((LD(yT) - LD(yF)) / LD(T_PART)) if np.isfinite(yF) and np.isfinite(yT) else float("nan")
    g = {t: A.f1_f32(l, s, t) for t in ts}
    H = None
    if hessian:
        N = A.level_size(l)[0]
        rp, ci = A.hessian_pattern(l)
        v = A.f2_f32(l, s, ts[0])
        assert v.dtype == np.float32 and all(x.dtype == np.float32 for x in g.values())
        Lo = sp.csr_matrix((v, ci, rp), shape=(N, N))
        H = (Lo + sp.tril(Lo, -1).T).toarray()
        assert H.dtype == np.float32
    return yF, yC, g, H


def same_device_results(a, b):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64)
    ok = np.float64(a[0]).tobytes() == np.float64(b[0]).tobytes() and np.float64(a[1]).tobytes() == np.float64(b[1]).tobytes()
    ok = ok and all(np.array_equal(bits(a[2][t]), bits(b[2][t])) for t in a[2])
    return ok and ((a[3] is None and b[3] is None) or np.array_equal(bits(a[3]), bits(b[3])))


def figures(f0F, f0C, g, H, Lv):
    r = {"f0F": BR.ratio(f0F, Lv.f0F, Lv.b_f0F, prec=P32), "f0C": BR.ratio(f0C, Lv.f0C, Lv.b_f0C, prec=P32),
         "f1": BR.ratio(g, Lv.g, Lv.b_g, prec=P32)}
    if H is not None:
        r["f2"] = BR.ratio(H, Lv.H, Lv.b_H, prec=P32)
    return r


def hold_level(pb, l, dev, Dz, c, terms, label, tally, ts=TS, a_node=None, mu_node=None, mask=None, hessian=True):
    """The device results `dev` of level l against the exact float level values at the rows Dz (doubles that are floats)."""
    B, kw = pb.B(l), dict(a_node=a_node, mu_node=mu_node, mask=mask)
    yF, yC, g, H = dev
    out = []
    for i, t in enumerate(ts):
        hs = hessian and i == 0                                   # f2 does not depend on t
        Lv = BR.level_reference(B, pb.K, pb.w, c, t, Dz, terms, hessian=hs, prec=P32, **kw)
        assert Lv.rows.feasible.all() and Lv.rows.in_range.all(), label
        kap = float(np.where(np.isfinite(Lv.rows.kappa), Lv.rows.kappa, 0).max())
        assert kap * 8 * U32 < 1.0, (label, kap)                  # the first-order bound means something
        assert np.isfinite(yF) and np.isfinite(yC), (label, yF, yC)
        bF, bC, bg, bH = BR.level_f32(B, pb.K, pb.w, c, t, Dz, terms, hessian=hs, **kw)
        d = figures(yF, yC, g[t], H if hs else None, Lv)
        b = figures(bF, bC, bg, bH, Lv)
        if i > 0:
            d, b = {"f1": d["f1"]}, {"f1": b["f1"]}               # f0F, f0C do not depend on t either
        tally.add((label, l, t), d, b)
        out.append((t, kap, d, b))
    return out


def fmt(out):
    return "  ".join("t=%.0e " % t + " ".join("%s %.2f/%.2f" % (k, d[k], b[k]) for k in d) for t, _, d, b in out)


# ---------------------------------------------------------------------------------------------------------- row sweep
def sweep_rows(pb, terms, Y, c, label, tally, p_node=None, mask=None, both_deliveries=True):
    """The rows Y in batches of 64 through the identity layout on the cube (the last batch wraps around): both deliveries
    agree bit for bit, idle columns and inactive slots are exact, f0 is finite, and f0 (both parts), f1 and f2 are within the
    margin of the float level reference.  p_node / mask: per-row exponents of term 0 / per-row term mask, set per batch."""
    A, n, K = pb.A, pb.n, pb.K
    N = A.level_size(0)[0]
    assert N == n * K and A.L == 1
    B = pb.B(0)
    w32, c32 = f32(pb.w), f32(c)
    active = sorted({col for t in terms for col in BR.parse(t)["cols"]})
    idle = [k for k in range(K) if k not in active]
    zero_s, zero_z = np.zeros(N, dtype=np.float32), np.zeros(N)
    worst = {}
    kap = 0.0
    for b0 in range(0, len(Y), BATCH):
        idx = (b0 + np.arange(BATCH)) % len(Y)
        Yb = Y[idx]
        zv = Yb.reshape(-1, order="F")
        assert np.array_equal((B @ zv).reshape(n, K), Yb)                      # the layout: B s is the batch, row by row
        an = mn = mk = None
        if p_node is not None:
            A.set_exponents(0, p_node[idx, 0])
            an, mn = BR.a_of(p_node[idx]), BR.mu_of(p_node[idx])
        if mask is not None:
            mk = mask[idx]
            A.set_term_mask(mk.astype(np.uint8))
        A.set_z(zv)
        dev = device_level(A, 0, zero_s)
        if both_deliveries:
            A.set_z(zero_z)
            assert same_device_results(dev, device_level(A, 0, zv.astype(np.float32))), (label, b0, "z and s deliveries differ")
        yF, yC, g, H = dev
        Hb = H.reshape(K, n, K, n)
        off_node = Hb.copy()
        off_node[:, np.arange(n), :, np.arange(n)] = 0
        assert not off_node.any(), (label, "f2 couples different nodes")
        assert np.array_equal(H, H.T)                                           # by construction: one triangle comes back
        assert not Hb[idle].any() and not Hb[:, :, idle].any(), (label, "f2 of an idle column")
        for t in TS:
            v = g[t].reshape(K, n).T
            with np.errstate(all="ignore"):
                plain = w32[:, None] * (np.float32(t) * c32)
            assert np.array_equal(v[:, idle], plain[:, idle]), (label, t, "f1 of an idle column is not w t c")
            if mk is not None:                                               # the half space alone owns column 0
                off = ~mk[:, 1]
                assert np.array_equal(v[off, 0], plain[off, 0]) and not Hb[0, off, 0, off].any(), (label, "slots of a masked-out term")
        out = hold_level(pb, 0, dev, Yb, c, terms, label, tally, a_node=an, mu_node=mn, mask=mk)
        for t, k_, d, b in out:
            kap = max(kap, k_)
            for k in d:
                key = "%s%s" % (k, "" if k != "f1" else "(t=%.0e)" % t)
                worst[key] = max(worst.get(key, (0.0, 0.0)), (d[k], b[k]))
    print("%-72s n=%3d kappa<=%.1e  device/base  " % (label, len(Y), kap) + "  ".join("%s %.2f/%.2f" % (k, d, b) for k, (d, b) in worst.items()))


@pytest.mark.parametrize("ci", range(len(BR.CASES)), ids=[c[0].replace(" ", "_") for c in BR.CASES])
def test_row_sweep_through_the_float_entry_points(M, cube, ci):
    name, K, terms = BR.CASES[ci]
    pb = identity_problem(M, cube, K, terms)
    rng = np.random.default_rng(500 + ci)
    c = f32(rng.standard_normal((pb.n, K))).astype(np.float64)
    pb.A.set_c(c)
    tally = Tally()
    print()
    for label, _, _, Y in BR.classes(prec=P32, only=(ci,)):
        assert len(Y) >= 0.4 * 200, label
        sweep_rows(pb, terms, Y, c, label, tally)
    tally.done("row sweep, " + name)


def test_per_node_exponents_and_term_masks_in_float(M, cube):
    """BR.node_exponent_rows and BR.piecewise_rows in the float regimes on the identity layout: the exponents and the mask are
    set per batch on one handle.  Rows that violate a masked-out term stay finite, and that term's slots are exact zeros."""
    tally = Tally()
    print()
    rng = np.random.default_rng(41)
    K, terms, Y, pn = BR.node_exponent_rows(prec=P32)
    assert set(BR.mu_of(pn).ravel()) == {0.0, 1.0, 2.0}
    pb = identity_problem(M, cube, K, terms)
    c = f32(rng.standard_normal((pb.n, K))).astype(np.float64)
    pb.A.set_c(c)
    order = rng.permutation(len(Y))                                           # every batch mixes the exponents
    sweep_rows(pb, terms, Y[order], c, "per-node p in {1, 1.1, 1.7, 2, 2.1, 2.6, 8}", tally, p_node=pn[order])
    K, terms, Y, mask = BR.piecewise_rows(prec=P32)
    violated = ~mask[:, 1] & (Y[:, 0] - 0.25 <= 0)
    assert violated.sum() >= 10
    pb = identity_problem(M, cube, K, terms)
    c = f32(rng.standard_normal((pb.n, K))).astype(np.float64)
    pb.A.set_c(c)
    order = rng.permutation(len(Y))
    sweep_rows(pb, terms, Y[order], c, "piecewise: cone everywhere, half space on some rows", tally, mask=mask[order])
    tally.done("per-node exponents and masks")


# ---------------------------------------------------------------------------------------------------------- positions
def test_positions_fem2d_L4_and_fem1d_L2(M):
    """A checked batch of 97 rows tiled over the 896 nodes of fem2d L = 4 (three and a half workgroups of 256; B is 0 / 1 with
    several nodes per unknown at the finest level, interpolation weights below), and 8 rows on fem1d L = 2, far below one wave:
    f0, f1 and f2 of the finest and the coarsest level against the float level reference."""
    tally = Tally()
    print()
    K, terms = 4, [([1, 2, 3], 1.5), ("linear", [0, 3], [1.0, 0.5], 0.2)]
    Yb = np.vstack([BR.generate(terms, K, near, target, 3, 20, 77 + 10 * near + j, P32)
                    for near in (0, 1) for j, target in enumerate((None, 1e-2, 1e-4))])
    assert len(Yb) >= 97
    Yb = Yb[np.random.default_rng(3).permutation(len(Yb))[:97]]
    gm = M.fem2d_mpi(4)
    pb = identity_problem(M, gm, K, terms)
    n = pb.n
    assert n == 896 and n % 256 == 128
    rng = np.random.default_rng(8)
    c = f32(rng.standard_normal((n, K))).astype(np.float64)
    Y = Yb[np.arange(n) % 97]
    pb.A.set_c(c)
    pb.A.set_z(Y.reshape(-1, order="F"))
    for l in (pb.A.L - 1, 0):
        N = pb.A.level_size(l)[0]
        Bl = pb.B(l)
        assert Bl.shape == (n * K, N) and int(np.bincount(Bl.indices, minlength=N).max()) > 1
        assert np.array_equal(pb.A.apply_D(l, np.zeros(N)), Y)
        out = hold_level(pb, l, device_level(pb.A, l, np.zeros(N, dtype=np.float32)), Y, c, terms, "fem2d L=4 identity layout", tally)
        print("fem2d L=4, 97 rows tiled over %d nodes, level %d (N = %d): device/base  %s" % (n, l, N, fmt(out)))
    K, terms = 2, [([0, 1], 1.0)]
    Y = np.vstack([BR.generate(terms, K, 0, target, 3, 3, 91 + j, P32) for j, target in enumerate((None, 1e-2, 1e-4))])[:8]
    gm = M.fem1d_mpi(2)
    pb = identity_problem(M, gm, K, terms)
    assert pb.n == 8 and len(Y) == 8
    c = f32(rng.standard_normal((8, K))).astype(np.float64)
    pb.A.set_c(c)
    pb.A.set_z(Y.reshape(-1, order="F"))
    for l in (1, 0):
        N = pb.A.level_size(l)[0]
        out = hold_level(pb, l, device_level(pb.A, l, np.zeros(N, dtype=np.float32)), Y, c, terms, "fem1d L=2 identity layout", tally)
        print("fem1d L=2, 8 rows, level %d (N = %d): device/base  %s" % (l, N, fmt(out)))
    tally.done("positions")


# ---------------------------------------------------------------------------------------------------------- states of the float path
def hold_state(M, pb, terms, z, c, ts, label, tally, p_node=None, mask=None, levels=None):
    """f0_f32 / f1_f32 / f2_f32 at the state z (n x S), s = 0, against the exact float level values at the floats of the
    device's own D z."""
    A = pb.A
    A.set_c(c)
    A.set_z(np.asarray(z, dtype=np.float64).reshape(-1, order="F"))
    an = None if p_node is None else BR.a_of(p_node)
    mn = None if p_node is None else BR.mu_of(p_node)
    for l in (range(A.L) if levels is None else levels):
        N = A.level_size(l)[0]
        Dz = f32(A.apply_D(l, np.zeros(N))).astype(np.float64)
        dev = device_level(A, l, np.zeros(N, dtype=np.float32), ts)
        out = hold_level(pb, l, dev, Dz, c, terms, label, tally, ts=ts, a_node=an, mu_node=mn, mask=mask)
        print("%-34s l=%d kappa_max %.1e (kappa 8 u32 = %.3f) | %s" % (label, l, out[0][1], out[0][1] * 8 * U32, fmt(out)))


@pytest.mark.parametrize("kind,L,p", [("fem1d", 3, 1.0), ("fem2d", 2, 2.0), ("fem2d", 3, 1.0), ("fem2d", 3, 1.5), ("fem3d", 2, 1.0)])
def test_end_states_of_the_float_solve_every_level(M, kind, L, p):
    """The configurations of test_float32_solve_at_the_reference_float32_tolerance: the state z of *_mpi_solve(T = float32), every
    level, t = ts[-1] = 1e4 and t = 1e2."""
    sol = getattr(M, kind + "_mpi_solve")(L=L, p=p, T=np.float32)
    gm = sol.geometry
    z = sol.z.to_numpy()
    assert sol.SOL_main["ts"][-1] == 1e4
    dim = gm.discretization["dim"]
    c = O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), gm.x.to_numpy())
    pb = Problem(M.AMG(gm, p=p), gm)
    tally = Tally()
    print()
    hold_state(M, pb, BR.default_terms(dim, p), z, c, (float(sol.SOL_main["ts"][-1]), 1e2), "%s L=%d p=%g float end state" % (kind, L, p), tally)
    tally.done("float end state")


def _solved_state(A, c, z0):
    A.set_c(c)
    A.set_z(np.asarray(z0).reshape(-1, order="F"))
    A.prepare()
    A.solve(tol=TOL32)
    return A.get_z().reshape(np.asarray(z0).shape, order="F")


OBST_G = lambda x: np.array([0.3 + 0.5 * (x[0] ** 2 + x[1] ** 2), 100.0])
OBST_F = lambda x: np.array([5.0, 0.0, 0.0, 1.0])


def test_float_kernels_at_states_with_obstacle_mask_node_exponents_and_slack_column(M):
    """One state each of the rest of the menu, the constructions of test_gpu_barrier_rows.py's
    test_states_with_mask_node_exponents_obstacle_and_slack_column, solved in double with tol = sqrt(eps32) so that the state
    sits near t = 1e4; finest and coarsest level."""
    L = 3
    gm = M.fem2d_mpi(L)
    x = gm.x.to_numpy()
    c = O.map_rows(lambda xi: O.DEFAULT_F[2](xi), x)
    cone15, lin = ([1, 2, 3], 1.5), ("linear", [0], [1.0], -0.1)
    zg = O.map_rows(OBST_G, x)
    cf = O.map_rows(OBST_F, x)
    tally = Tally()
    ts, lv = (1e4, 1e2), (L - 1, 0)
    print()
    pb = Problem(M.AMG(gm, p=1.5, cones=[cone15, lin]), gm)
    z = _solved_state(pb.A, cf, zg)
    assert z[:, 0].min() - 0.1 < 1e-2                                   # in contact, as far as t = 1e4 lets it
    hold_state(M, pb, [cone15, lin], z, cf, ts, "obstacle in contact", tally, levels=lv)
    select = lambda xi: (True, xi[0] > 0.0)
    mask = np.array([select(xi) for xi in x], dtype=bool)
    pb = Problem(M.AMG(gm, p=1.5, cones=[cone15, lin], select=select), gm)
    z = _solved_state(pb.A, cf, zg)
    assert z[x[:, 0] < 0, 0].min() < 0.1                               # the masked-out term is violated there
    hold_state(M, pb, [cone15, lin], z, cf, ts, "term mask", tally, mask=mask, levels=lv)
    pfun = lambda xi: 1.6 + 0.5 * xi[0]
    pn = np.array([pfun(xi) for xi in x])
    assert set(BR.mu_of(pn)) >= {1.0, 2.0}
    pb = Problem(M.AMG(gm, p=1.0, cones=[([1, 2, 3], pfun)]), gm)
    z = _solved_state(pb.A, c, O.map_rows(lambda xi: O.DEFAULT_G[2](xi), x))
    hold_state(M, pb, [([1, 2, 3], 1.0)], z, c, ts, "p(x) = 1.6 + 0.5 x", tally, p_node=pn[:, None], levels=lv)
    state1 = tuple(M.DEFAULT_STATE) + (("sigma", "full"),)
    D1 = tuple(M.DEFAULT_D[2]) + (("sigma", "id"),)
    terms = [([1, 2, 3], 1.5, 4), ("linear", [0, 4], [1.0, 1.0], 0.2), ("linear", [4], [1.0], 1.0)]
    g = lambda xi: np.array([1.0 - 1.5 * (1.0 - float(np.sum(np.asarray(xi) ** 2)) / 2), 0.05])
    z0 = O.map_rows(g, x)
    pb = Problem(M.AMG(gm, state1, D1, 1.5, cones=terms), gm)
    A0 = M.AMG(gm, p=1.5)
    A0.set_z(z0.reshape(-1, order="F"))
    Dz0 = A0.apply_D(L - 1, np.zeros(A0.level_size(L - 1)[0]))
    sigma0 = 1.0 + max(0.0, float(np.max(np.sum(Dz0[:, 1:3] ** 2, axis=1) ** 0.75 - Dz0[:, 3])), float(np.max(-(Dz0[:, 0] + 0.2))))
    c1 = np.column_stack([c, np.full(len(x), 10.0)])
    z = _solved_state(pb.A, c1, np.column_stack([z0, np.full(len(x), sigma0)]))
    hold_state(M, pb, terms, z, c1, ts, "slack column (is2), 3 terms", tally, levels=lv)
    tally.done("states of the menu")


# ---------------------------------------------------------------------------------------------------------- classification
def test_classification_after_the_rounding_to_float(M, cube):
    """Rows with an exact answer through f0_f32 on the identity layout, one bad row among 63 good ones, at several node
    positions: +inf for the hand-made rows that are floats (phi = 0 exactly, s <= 0, phi < 0, a NaN entry, the half space on
    and past its boundary) and for rows strictly inside in double whose float rounding lies on or outside the boundary, while
    A.f0 stays finite there; finite for rows whose float rounding is inside by more than the float bound of phi.  Nothing is
    asserted about f1_f32 / f2_f32 of a batch with an infeasible row: their content there is unspecified."""
    rows = []
    for K, terms, Y, what in BR.hand_made():
        Y = np.array(Y, dtype=np.float64)
        rows += [(K, terms, y, True, None, what) for y in Y[BR.float_representable(Y)]]
    rows += [(K, terms, np.array(y), out, True, what) for K, terms, y, out, what in BR.rounding_rows()]
    assert sum(1 for r in rows if np.isnan(r[2]).any()) == 2
    problems = {}
    rng = np.random.default_rng(17)
    for K, terms, y, outside, double_finite, what in rows:
        key = repr((K, terms))
        if key not in problems:
            pb = identity_problem(M, cube, K, terms)
            good = BR.generate(terms, K, 0, None, 3, BATCH - 1, 1234 + len(problems), P32)
            assert len(good) == BATCH - 1
            c = f32(rng.standard_normal((pb.n, K))).astype(np.float64)
            pb.A.set_c(c)
            problems[key] = (pb, good)
        pb, good = problems[key]
        A, N = pb.A, pb.A.level_size(0)[0]
        zero_s, zero_d = np.zeros(N, dtype=np.float32), np.zeros(N)
        R32 = BR.reference(terms, y[None, :], prec=P32)
        assert bool(R32.feasible[0]) == (not outside), what
        if not outside:
            assert np.all(np.abs(R32.phi[0]) > U32 * R32.bphi[0]), what
        for pos in (0, 29, BATCH - 1):
            Yb = np.insert(good, pos, y, axis=0)
            A.set_z(Yb.reshape(-1, order="F"))
            y32 = A.f0_f32(0, zero_s, 1.0)
            if outside:
                assert np.isposinf(y32), (what, pos, y32)
            else:
                assert np.isfinite(y32), (what, pos, y32)
            if double_finite:
                assert np.isfinite(A.f0(0, zero_d, 1.0)), (what, pos)
        A.set_z(np.vstack([good, good[:1]]).reshape(-1, order="F"))
        assert np.isfinite(A.f0_f32(0, zero_s, 1.0)), what                    # the good rows alone are inside
    print("\nclassification: %d rows x 3 node positions on %d term lists" % (len(rows), len(problems)))


# ---------------------------------------------------------------------------------------------------------- the handle
SOLVED = 1e-7      # size of the float32 s at a state solved to tol = sqrt(eps32): its rows are at relative distance 1e-5 from the cone


def _float_results(A, levels, t=37.0, seed=5, scale=2e-3):
    """Bytes of f0_f32, f1_f32 and f2_f32 at s = 0 and at a small float32 s, at the given levels in the given order."""
    out = []
    for l in levels:
        N = A.level_size(l)[0]
        for s in (np.zeros(N, dtype=np.float32), (scale * np.random.default_rng(seed + l).standard_normal(N)).astype(np.float32)):
            y = A.f0_f32(l, s, t)
            assert np.isfinite(y)
            out.append((l, np.float64(y).tobytes(), A.f1_f32(l, s, t).tobytes(), A.f2_f32(l, s, t).tobytes()))
    return out


def _double_results(A, levels, t=37.0, seed=5):
    out = []
    for l in levels:
        N = A.level_size(l)[0]
        s = 2e-3 * np.random.default_rng(seed + l).standard_normal(N)
        out.append((np.float64(A.f0(l, s, t)).tobytes(), A.f1(l, s, t).tobytes(), A.f2(l, s, t)[1].tobytes()))
    return out


def _menu_handle(M, L, c, z, pn=None, mask=None):
    gm = M.fem2d_mpi(L)
    A = M.AMG(gm, p=1.5, cones=[([1, 2, 3], 1.5), ("linear", [0], [1.0], -0.1)])
    A.set_c(c)
    A.set_z(z)
    if pn is not None:
        A.set_exponents(0, pn)
    if mask is not None:
        A.set_term_mask(mask)
    return A


def test_float_results_of_a_used_handle_equal_a_fresh_handle(M):
    """Bit for bit: before and after prepare() and a double solve(); after set_c, set_z, set_exponents and set_term_mask on a
    used handle; a coarse level called before and after the finest."""
    L = 3
    x = M.fem2d_mpi(L).x.to_numpy()
    cf, zg = O.map_rows(OBST_F, x), O.map_rows(OBST_G, x).reshape(-1, order="F")
    levels = list(range(L))
    fresh = _float_results(_menu_handle(M, L, cf, zg), levels)
    A = _menu_handle(M, L, cf, zg)
    assert _float_results(A, levels) == fresh
    A.prepare()
    assert _float_results(A, levels) == fresh, "after prepare()"
    A.solve(tol=TOL32)                                                     # a state the float path can stand at: t = 1e4
    z1 = A.get_z()
    assert not np.array_equal(z1, zg)
    after = _float_results(A, levels, scale=SOLVED)
    assert after == _float_results(_menu_handle(M, L, cf, z1), levels, scale=SOLVED), "after a double solve()"
    # new data on the used handle, one setter after the other
    c2 = cf * (1.0 + 0.25 * np.sin(3.0 * x[:, :1]))
    A.set_c(c2)
    assert _float_results(A, levels, scale=SOLVED) == _float_results(_menu_handle(M, L, c2, z1), levels, scale=SOLVED), "after set_c"
    A.set_z(zg)
    assert _float_results(A, levels) == _float_results(_menu_handle(M, L, c2, zg), levels), "after set_z"
    pn = np.array([1.6 + 0.5 * xi[0] for xi in x])
    A.set_exponents(0, pn)
    r_pn = _float_results(A, levels)
    assert r_pn == _float_results(_menu_handle(M, L, c2, zg, pn=pn), levels), "after set_exponents"
    mask = np.array([(True, xi[0] > 0.0) for xi in x], dtype=np.uint8)
    A.set_term_mask(mask)
    r_mask = _float_results(A, levels)
    assert r_mask == _float_results(_menu_handle(M, L, c2, zg, pn=pn, mask=mask), levels), "after set_term_mask"
    assert r_pn != r_mask and r_pn != after                                # the setters did change something
    # a coarse level before and after the finest
    B = _menu_handle(M, L, cf, zg)
    first = _float_results(B, [0])
    assert first == [r for r in fresh if r[0] == 0]
    assert _float_results(B, [L - 1]) == [r for r in fresh if r[0] == L - 1]
    assert _float_results(B, [0]) == first
    assert _float_results(_menu_handle(M, L, cf, zg), [L - 1, 0, 1]) == [r for l in (L - 1, 0, 1) for r in fresh if r[0] == l]


def test_float_calls_leave_the_double_state_alone(M):
    """A.f0, A.f1, A.f2 and a traced solve() are unchanged, bit for bit, by float calls made in between: the float path shares
    the reduction scratch and scalars with the double path, and its row buffers live beside the double ones."""
    L = 2
    gm = M.fem2d_mpi(L)
    x = gm.x.to_numpy()
    c, z0 = O.map_rows(lambda xi: O.DEFAULT_F[2](xi), x), O.map_rows(lambda xi: O.DEFAULT_G[2](xi), x).reshape(-1, order="F")
    levels = list(range(L))
    mode = M.AMG.TRACE_STEP.index("mode")
    keep = [i for i in range(len(M.AMG.TRACE_STEP)) if i != mode]

    def handle():
        A = M.AMG(gm, p=1.5)
        A.set_c(c)
        A.set_z(z0)
        return A

    def traced_solve(A, between):
        A.set_trace(4000, False)
        if between:
            _float_results(A, levels)
        A.solve(tol=TOL32)
        tr = A.trace()
        return tr["centerings"].tobytes(), tr["steps"][:, keep].tobytes(), A.get_z().tobytes()

    A = handle()
    d0 = _double_results(A, levels)
    _float_results(A, levels)
    assert _double_results(A, levels) == d0, "f0 / f1 / f2 after float calls"
    for l in levels:                                                           # interleaved call by call
        N = A.level_size(l)[0]
        s = np.zeros(N)
        y = A.f0(l, s, 2.0)
        A.f0_f32(l, s, 2.0)
        g = A.f1(l, s, 2.0)
        A.f1_f32(l, s, 2.0)
        v = A.f2(l, s, 2.0)[1]
        A.f2_f32(l, s, 2.0)
        assert A.f0(l, s, 2.0) == y and np.array_equal(A.f1(l, s, 2.0), g) and np.array_equal(A.f2(l, s, 2.0)[1], v), l
    plain = traced_solve(handle(), False)
    assert traced_solve(A, True) == plain, "a traced solve() after float calls on the handle"
    A.set_z(z0)
    _float_results(A, levels)
    assert traced_solve(A, True) == plain, "a second traced solve() with float calls before it"
    z_end = A.get_z()
    F = handle()
    F.set_z(z_end)
    assert _float_results(A, levels, scale=SOLVED) == _float_results(F, levels, scale=SOLVED)
