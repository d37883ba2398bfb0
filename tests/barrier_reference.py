"""Row reference of the barrier menu for the checks of the per-node barrier kernels (test_barrier_reference.py,
test_gpu_barrier_rows.py): plain numpy in long double on the CPU.  A helper module, not a test module.

Written from the formulas of csrc/kernels.hpp (ConeSpec) and oracle/mgb_oracle.py without calling either:

  power cone  (idx = (q_1..q_d, s), p [, is2])   F = -log(s^a - |q|^2) - mu log s,  a = fl(2.0 / p), s = y[is] (+ y[is2]),
                                                 mu = 0 (p = 2), 1 (p < 2), 2 (p > 2)
  half space  ("linear", idx, coef, off)         F = -log(sum_i coef_i y[idx_i] + off)

and F of a list of terms is the sum over the terms active at the row.  The inputs are exactly the doubles the kernels read:
the row of Dz, a (already rounded), mu, coef, off, optionally per-node a / mu and a term mask.  `reference()` gives F, the K
gradient entries and the K x K Hessian of every row in np.longdouble (64-bit mantissa), and beside every value a first-order
RUNNING ERROR BOUND in units of u = 2^-53 for an fp64 evaluation of the same formula:

  every rounded operation adds the magnitude of its own result; the bounds of the operands travel through it to first order
  (x y: e_x |y| + e_y |x|;  x / y: e_x / |y| + |x / y| e_y / |y|;  log x: e_x / |x|;  x^e: |x^e| (|e| e_x / |x| + |log x| e_e));
  multiplications by 2 and 4, negations, additions of zero and the subtractions a - 1, a - 2 where fp64 does them exactly add
  nothing (where fp64 rounds a - 1 or a - 2 the bound carries that rounding, which is known exactly).

With kappa = (s^a + |q|^2) / phi -- for a half space (sum |coef_i y_i| + |off|) / phi -- this gives a term with 1 / phi^m a
bound of about |term| (c + m kappa) and F a bound of about kappa + |log phi| + mu |log s| + |F|, c a small operation count.
Sums over terms add their bounds plus the magnitude of each partial sum.  `ratio(x, exact, bound)` = max |x - exact| /
(u bound): an fp64 code that evaluates these formulas with correctly rounded operations, in any association, has ratio <= 1 to first
order; a pow / log that is off by an ulp or two, or a fused multiply-add, moves it by a small constant.  A wrong slot, sign,
exponent or mu moves an entry by O(1) relative: a ratio of 1e13 and more where kappa is of order one, and still 1e13 / kappa
at the boundary.

Row generators (seeded) put rows strictly inside every term, the chosen term at relative distance phi / s^a (half space: phi /
(sum |coef_i y_i| + |off|)) near a target of 1e-4, 1e-8 or 1e-11, or of order one (the "1e0" regime draws it from [0.25, 1):
at exactly 1 the row has q = 0 and its gradient and mixed Hessian entries vanish), at scales s in 1e-3 .. 1e3 and, for the
single terms, 1e-30 .. 1e30; in an intersection every term in turn is the near-active one.  `level_reference()` carries rows, bounds and all to a level: f0, f1 = B' (w (F1 + t c)),
f2 = B' diag(w F2) B for the CSR B = D R (row q K + k) of the library's own host matrices; `diag_reference()` and
`hessian_apply_reference()` read diag(H) and H v off it, and `hessian_apply_matrix_free()` gives H v with the same bound without
forming H, for the levels of test_gpu_elop_kinds.py that are too large for a dense long-double matrix.

WORKING PRECISION.  reference(), level_reference(), ratio(), generate(), classes() and the row sets take `prec`: F64 (the default,
everything above) or F32, the float instantiation of the same kernel templates (csrc/kernels_f32.hip, test_gpu_barrier_rows_f32.py).
The bound model is the same first-order one with u = U32 = 2^-24, once the inputs are the floats those kernels read: rows, w, c,
B, coef and off rounded to float32, a = float32(fl(2.0 / p)) (the kernels cast T(P.cone[ci].a)), per-node a likewise; a_minus
carries float's rounding of a - 1 and a - 2 (a - 2 is not exact in float for every a < 1).  Rows are generated in double as
above, then rounded to float32 and filtered by the reference at the rounded rows.  Float has its own limits: every exact
intermediate, phi^2, s^2 and every entry of F1 and F2 stays inside RANGE32 = (2^-100, 2^100), the closest distance is MIN_DIST32 =
1e-5 (kappa 8 u32 < 1 on every kept row: the first-order bound means something) and the regimes are REGIMES32.  Overflow of
1 / phi^2 in float outside that range is a known limit of the float path and not part of this check.  rows_f32() is the float
baseline: the kernels' formulas in plain numpy float32, the counterpart of the fp64 oracle in rho_base."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "barrier_reference needs an extended-precision long double (x87); there is no fallback"

U = 2.0 ** -53
MARGIN = 16.0                # chol_reference.MARGIN: same arithmetic, other operation order / device pow and log / fma contraction
RANGE = (1e-280, 1e280)      # rows where an exact intermediate leaves this range are not generated
MIN_DIST = 1e-12             # generated rows keep every term at this relative distance or more
P_NEAR_ONE = 1.0 + 2.0 ** -20
U32 = 2.0 ** -24
RANGE32 = (2.0 ** -100, 2.0 ** 100)      # float: exact intermediates, phi^2, s^2 and the entries of F1 / F2 stay inside
MIN_DIST32 = 1e-5


class Precision:
    """A working precision of the kernels: the scalar type the inputs are rounded to, its unit roundoff (the unit of the bounds),
    the range outside of which rows are not generated, the closest relative distance and the regimes of the sweep."""

    def __init__(self, name, dtype, u, range_, min_dist):
        self.name, self.dtype, self.u, self.range, self.min_dist = name, dtype, u, range_, min_dist
        self.regimes = None                  # filled in below the case table

    def rnd(self, x):
        """x as the doubles that equal what a kernel of this precision reads."""
        x = np.asarray(x, dtype=np.float64)
        if self.dtype is np.float64:
            return x
        with np.errstate(all="ignore"):
            return x.astype(self.dtype).astype(np.float64)

    def __repr__(self):
        return self.name


F64 = Precision("fp64", np.float64, U, RANGE, MIN_DIST)
F32 = Precision("fp32", np.float32, U32, RANGE32, MIN_DIST32)


def mu_of(p):
    p = np.asarray(p, dtype=np.float64)
    return np.where(p == 2.0, 0.0, np.where(p < 2.0, 1.0, 2.0))


def a_of(p):
    """a = fl(2.0 / p), the double the kernels read (csrc/capi.cpp make_params_cones, csrc/amg.cpp set_exponents)."""
    return np.float64(2.0) / np.asarray(p, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------- values with bounds
class V:
    """Long-double values with their running error bound (units of u) for an fp64 evaluation."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape, dtype=LD) if e is None else np.asarray(e, dtype=LD)


def _both(x, y):
    return (x.v != 0) & (y.v != 0)


def add(x, y):
    v = x.v + y.v
    return V(v, x.e + y.e + np.where(_both(x, y), np.abs(v), 0))


def neg(x):
    return V(-x.v, x.e)


def sub(x, y):
    return add(x, neg(y))


def scale(x, c):
    """x times a power of two (or a small integer that fp64 multiplies exactly here: mu in {0, 1, 2})."""
    return V(x.v * c, x.e * np.abs(c))


def mul(x, y):
    v = x.v * y.v
    return V(v, x.e * np.abs(y.v) + y.e * np.abs(x.v) + np.abs(v))


def div(x, y):
    v = x.v / y.v
    return V(v, x.e / np.abs(y.v) + np.abs(v) * y.e / np.abs(y.v) + np.abs(v))


def log(x):
    v = np.log(x.v)
    return V(v, x.e / np.abs(x.v) + np.abs(v))


def power(x, e):
    v = np.power(x.v, e.v)
    return V(v, np.abs(v) * (np.abs(e.v) * x.e / np.abs(x.v) + np.abs(np.log(x.v)) * e.e + 1))


def const(c, n):
    return V(np.full(n, c, dtype=LD))


def a_minus(a64, k, prec=F64):
    """a - k as the working precision computes it from its a: the exact difference, and the rounding error of the working
    precision's difference as its bound (fp64 subtracts 1 and 2 exactly on the menu; float does not for every a < 1)."""
    exact = a64.astype(LD) - LD(k)
    if prec is F64:
        return V(exact, np.abs(exact - (a64 - np.float64(k)).astype(LD)) / LD(U))
    got = (a64.astype(prec.dtype) - prec.dtype(k)).astype(LD)
    return V(exact, np.abs(exact - got) / LD(prec.u))


# ---------------------------------------------------------------------------------------------------------- terms
def parse(term):
    """(kind, cols_q, is, is2, p, coef, off) of a term in the library's syntax."""
    if term[0] == "linear":
        _, idx, coef, off = term
        return dict(kind=1, q=list(idx), coef=[float(c) for c in coef], off=float(off), cols=list(idx))
    idx, p = term[0], term[1]
    is2 = int(term[2]) if len(term) > 2 else -1
    cols = list(idx) + ([is2] if is2 >= 0 else [])
    return dict(kind=0, q=list(idx[:-1]), s=int(idx[-1]), s2=is2, p=p, cols=cols)


def _power_cone(T, Y, a64, mu64, prec=F64):
    n = Y.shape[0]
    q = [V(Y[:, i]) for i in T["q"]]
    s = V(Y[:, T["s"]])
    if T["s2"] >= 0:
        s = add(s, V(Y[:, T["s2"]]))
    a, mu = V(a64), V(mu64)
    sa = power(s, a)
    qq = None
    for qi in q:
        qq = mul(qi, qi) if qq is None else add(qq, mul(qi, qi))
    phi = sub(sa, qq)
    ok = (s.v > 0) & (phi.v > 0)
    F = sub(neg(log(phi)), scale(log(s), mu.v))
    am1, am2 = a_minus(a64, 1, prec), a_minus(a64, 2, prec)
    ds = mul(a, power(s, am1))
    dds = mul(mul(a, am1), power(s, am2))
    ip = div(const(1, n), phi)
    ip2 = mul(ip, ip)
    gs = sub(neg(div(ds, phi)), div(mu, s))
    hss = add(add(neg(mul(dds, ip)), mul(mul(ds, ds), ip2)), div(mu, mul(s, s)))
    G, H = {}, {}
    scols = [T["s"]] + ([T["s2"]] if T["s2"] >= 0 else [])
    for i, ci in enumerate(T["q"]):
        G[ci] = div(scale(q[i], 2), phi)
        for j, cj in enumerate(T["q"]):
            h = mul(mul(scale(q[i], 4), q[j]), ip2)
            H[(ci, cj)] = add(h, scale(ip, 2)) if i == j else h
        hqs = scale(mul(mul(q[i], ds), ip2), -2)
        for cs in scols:
            H[(ci, cs)] = H[(cs, ci)] = hqs
    for cs in scols:
        G[cs] = gs
        for cs_ in scols:
            H[(cs, cs_)] = hss
    kappa = (sa.v + qq.v) / phi.v
    return dict(F=F, G=G, H=H, ok=ok, phi=phi.v, bphi=phi.e, dist=phi.v / sa.v, kappa=kappa,
                inter=[sa.v, qq.v, phi.v, phi.v * phi.v, s.v * s.v, ds.v])


def _half_space(T, Y, prec=F64):
    n = Y.shape[0]
    off, coef = float(prec.rnd(T["off"])), [float(c) for c in prec.rnd(T["coef"])]      # the kernels cast T(coef), T(off)
    T = dict(T, off=off, coef=coef)
    phi, mag = V(np.full(n, T["off"], dtype=LD)), np.full(n, abs(T["off"]), dtype=LD)
    for i, c in zip(T["q"], T["coef"]):
        t = mul(const(c, n), V(Y[:, i]))
        phi, mag = add(phi, t), mag + np.abs(t.v)
    ok = phi.v > 0
    F = neg(log(phi))
    ip2 = div(const(1, n), mul(phi, phi))
    G, H = {}, {}
    for i, ci in zip(T["q"], T["coef"]):
        G[i] = neg(div(const(ci, n), phi))
        for j, cj in zip(T["q"], T["coef"]):
            H[(i, j)] = mul(mul(const(ci, n), const(cj, n)), ip2)
    return dict(F=F, G=G, H=H, ok=ok, phi=phi.v, bphi=phi.e, dist=phi.v / mag, kappa=mag / phi.v, inter=[phi.v, phi.v * phi.v])


class Rows:
    """F (n), F1 (n, K), F2 (n, K, K) in long double, their bounds bF, bF1, bF2 (units of u), per term the cone distance
    `phi` with its bound `bphi`, the relative distance `dist`, the amplification `kappa` (n, nterms; +inf where the term is masked out), `feasible`
    (every active term strictly inside) and `in_range` (every exact intermediate inside RANGE)."""


def reference(terms, Y, a_node=None, mu_node=None, mask=None, prec=F64):
    """Rows of the barrier of `terms` at the rows of Y (n x K doubles).  a_node / mu_node: n x nterms doubles replacing the
    power cones' constants; mask: n x nterms, 0 = the term is inactive at that row.  prec: the working precision -- the rows,
    a, the per-node arrays, coef and off are rounded to it first (what its kernels read), the bounds are in its unit
    roundoff and in_range refers to its range."""
    Y = np.ascontiguousarray(prec.rnd(Y), dtype=np.float64)
    RANGE = prec.range
    n, K = Y.shape
    Yl = Y.astype(LD)
    nt = len(terms)
    R = Rows()
    F = V(np.zeros(n, dtype=LD))
    G = [V(np.zeros(n, dtype=LD)) for _ in range(K)]
    H = [[V(np.zeros(n, dtype=LD)) for _ in range(K)] for _ in range(K)]
    R.phi, R.dist, R.kappa = (np.full((n, nt), np.inf, dtype=LD) for _ in range(3))
    R.bphi = np.zeros((n, nt), dtype=LD)
    R.feasible, R.in_range = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for ti, term in enumerate(terms):
            T = parse(term)
            assert len(set(T["cols"])) == len(T["cols"]) and all(0 <= c < K for c in T["cols"]), term
            act = np.ones(n, dtype=bool) if mask is None else np.asarray(mask)[:, ti] != 0
            if T["kind"] == 0:
                a64 = prec.rnd(np.full(n, a_of(T["p"])) if a_node is None else np.asarray(a_node, dtype=np.float64)[:, ti])
                mu64 = prec.rnd(np.full(n, mu_of(T["p"])) if mu_node is None else np.asarray(mu_node, dtype=np.float64)[:, ti])
                t = _power_cone(T, Yl, a64, mu64, prec)
            else:
                t = _half_space(T, Yl, prec)
            z = lambda x: V(np.where(act, x.v, 0), np.where(act, x.e, 0))
            F = add(F, z(t["F"]))
            for c, g in t["G"].items():
                G[c] = add(G[c], z(g))
            for (ci, cj), h in t["H"].items():
                H[ci][cj] = add(H[ci][cj], z(h))
            R.phi[:, ti] = np.where(act, t["phi"], np.inf)
            R.bphi[:, ti] = np.where(act, t["bphi"], 0)
            R.dist[:, ti] = np.where(act, t["dist"], np.inf)
            R.kappa[:, ti] = np.where(act, t["kappa"], np.inf)
            R.feasible &= np.where(act, t["ok"], True)
            for x in t["inter"]:
                ax = np.abs(x)
                R.in_range &= ~act | (ax == 0) | ((ax >= RANGE[0]) & (ax <= RANGE[1]))
        R.F, R.bF = np.where(R.feasible, F.v, np.inf), F.e
        R.F1, R.bF1 = np.stack([g.v for g in G], axis=1), np.stack([g.e for g in G], axis=1)
        R.F2 = np.stack([np.stack([h.v for h in row], axis=1) for row in H], axis=1)
        R.bF2 = np.stack([np.stack([h.e for h in row], axis=1) for row in H], axis=1)
        for x in (R.F1, R.F2):
            ax = np.abs(x).reshape(n, -1)
            R.in_range &= np.all((ax == 0) | ((ax >= RANGE[0]) & (ax <= RANGE[1])), axis=1)
    return R


def ratio(x, exact, bound, rows=None, prec=F64):
    """max over entries of |x - exact| / (u bound), u the unit roundoff of prec; an entry whose bound is zero must be met
    exactly."""
    x, exact, bound = np.asarray(x, dtype=LD), np.asarray(exact, dtype=LD), np.asarray(bound, dtype=LD)
    if rows is not None:
        x, exact, bound = x[rows], exact[rows], bound[rows]
    if x.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(x - exact)
        r = np.where(err == 0, 0, np.where(bound > 0, err / (LD(prec.u) * bound), np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------- case table
CASES = [
    # name, K, terms
    ("cone nq1 K2 p1", 2, [([0, 1], 1.0)]),
    ("cone nq2 K4 p1.5", 4, [([1, 2, 3], 1.5)]),
    ("cone nq3 K5 p2", 5, [([1, 2, 3, 4], 2.0)]),
    ("cone nq3 K8 p3 idx 6,1,4|2", 8, [([6, 1, 4, 2], 3.0)]),
    ("cone nq2 K4 p8 idx 3,0|1", 4, [([3, 0, 1], 8.0)]),
    ("cone nq1 K4 p1+2^-20 idx 2|0", 4, [([2, 0], P_NEAR_ONE)]),
    ("cone nq2 K8 p1+2^-20", 8, [([5, 6, 7], P_NEAR_ONE)]),
    ("cone+is2 nq2 K5 p1.5", 5, [([1, 2, 3], 1.5, 4)]),
    ("cone+is2 nq1 K4 p1 idx 2|0+3", 4, [([2, 0], 1.0, 3)]),
    ("cone+is2 nq3 K8 p3 idx 7,5,0|3+1", 8, [([7, 5, 0, 3], 3.0, 1)]),
    ("cone+is2 nq2 K4 p2 idx 3,1|2+0", 4, [([3, 1, 2], 2.0, 0)]),
    ("half nq1 K2", 2, [("linear", [0], [1.0], -0.3)]),
    ("half nq2 K4 mixed signs idx 3,1", 4, [("linear", [3, 1], [2.0, -0.75], 0.5)]),
    ("half nq3 K5 mixed signs idx 4,0,2", 5, [("linear", [4, 0, 2], [-1.5, 0.25, 3.0], -2.0)]),
    ("half nq3 K8", 8, [("linear", [7, 2, 5], [1.0, 1.0, -1.0], 0.0)]),
    ("cone & half, shared columns K4", 4, [([1, 2, 3], 1.5), ("linear", [1, 3], [1.0, 0.5], 0.2)]),
    ("cone & half, disjoint K4", 4, [([1, 2, 3], 1.0), ("linear", [0], [1.0], 5.0)]),
    ("two cones disjoint K5 (parabolic)", 5, [([0, 3], 2.0), ([1, 2, 4], 1.5)]),
    ("two cones sharing a q column K4", 4, [([0, 2], 2.0), ([0, 1, 3], 1.5)]),
    ("cone & two halves K5", 5, [([1, 2, 4], 1.0), ("linear", [0], [1.0], -0.1), ("linear", [0, 3], [-1.0, 0.5], 2.0)]),
    ("two cones (one +is2) & half, shared K8", 8, [([0, 1, 2, 3], 2.0), ([4, 5], 8.0, 6),
                                                  ("linear", [7, 3, 4], [1.0, -1.0, 0.5], 1.0)]),
    ("three cones K8", 8, [([0, 1], 1.0), ([2, 3, 4], 3.0), ([5, 6, 7], P_NEAR_ONE)]),
    ("three halves sharing columns K2", 2, [("linear", [0], [1.0], 1.0), ("linear", [0], [-1.0], 1.0),
                                          ("linear", [1, 0], [1.0, -0.5], 0.25)]),
]
# regimes: (label, target relative distance of the near-active term (None: uniform in [0.25, 1)), decades of the scale)
REGIMES = [("1e0", None, 3), ("1e-4", 1e-4, 3), ("1e-8", 1e-8, 3), ("1e-11", 1e-11, 3), ("1e0 wide", None, 30),
           ("1e-8 wide", 1e-8, 30)]
REGIMES32 = [("1e0", None, 3), ("1e-2", 1e-2, 3), ("1e-4", 1e-4, 3), ("1e0 wide", None, 8), ("1e-3 wide", 1e-3, 8)]
F64.regimes, F32.regimes = REGIMES, REGIMES32


def _magnitudes(rng, n, decades):
    return np.power(LD(10), rng.uniform(-decades, decades, n).astype(LD))


def _fill_cone(T, Y, free, d, rng, decades):
    n = Y.shape[0]
    a = LD(a_of(T["p"]))
    qf = [c for c in T["q"] if free[c]]
    sf = [c for c in [T["s"]] + ([T["s2"]] if T["s2"] >= 0 else []) if free[c]]
    qfix = sum((Y[:, c] ** 2 for c in T["q"] if not free[c]), np.zeros(n, dtype=LD))
    direction = rng.standard_normal((n, max(len(qf), 1))).astype(LD)
    direction /= np.sqrt(np.sum(direction ** 2, axis=1))[:, None]
    if sf:
        if len(qf) == len(T["q"]):             # everything free: pick s, put q on the sphere of radius sqrt(s^a (1 - d))
            s = _magnitudes(rng, n, decades)
            r = np.sqrt(np.power(s, a) * (1 - d))
            for j, c in enumerate(qf):
                Y[:, c] = direction[:, j] * r
        else:                                  # some q are given: free q of their size, then s from |q|^2
            for j, c in enumerate(qf):
                Y[:, c] = direction[:, j] * np.sqrt(qfix)
            qq = sum((Y[:, c] ** 2 for c in T["q"]), np.zeros(n, dtype=LD))
            s = np.power(qq / (1 - d), 1 / a)
        other = sum((Y[:, c] for c in (T["s"], T["s2"]) if c >= 0 and not free[c]), np.zeros(n, dtype=LD))
        if len(sf) == 2:                       # split the slack over both columns, signs mixed
            Y[:, sf[0]] = s * rng.uniform(-1.0, 2.0, n).astype(LD)
            Y[:, sf[0]] = Y[:, sf[0]].astype(np.float64).astype(LD)
            Y[:, sf[1]] = s - Y[:, sf[0]]
        else:
            Y[:, sf[0]] = s - other
    elif qf:                                   # the slack is given: the free q take what is left of s^a (1 - d)
        s = sum((Y[:, c] for c in (T["s"], T["s2"]) if c >= 0), np.zeros(n, dtype=LD))
        with np.errstate(all="ignore"):
            left = np.power(s, a) * (1 - d) - qfix
            r = np.sqrt(np.where(left > 0, left, 0))
        for j, c in enumerate(qf):
            Y[:, c] = direction[:, j] * r
    for c in qf + sf:
        free[c] = False


def _fill_half(T, Y, free, d, rng, decades):
    n = Y.shape[0]
    fc = [(c, k) for c, k in zip(T["q"], T["coef"]) if free[c] and k != 0.0]
    for c, k in zip(T["q"], T["coef"]):
        if free[c] and (not fc or c != fc[-1][0]):
            Y[:, c] = _magnitudes(rng, n, decades) * rng.choice([-1.0, 1.0], n)
            free[c] = False
    if not fc:
        return
    cj, kj = fc[-1]
    rest, mag = np.full(n, T["off"], dtype=LD), np.full(n, abs(T["off"]), dtype=LD)
    for c, k in zip(T["q"], T["coef"]):
        if c != cj:
            rest, mag = rest + LD(k) * Y[:, c], mag + np.abs(LD(k) * Y[:, c])
    mag = np.where(mag > 0, mag, _magnitudes(rng, n, decades))
    Y[:, cj] = (d * (mag + np.abs(rest)) - rest) / LD(kj)
    free[cj] = False


def generate(terms, K, near, target, decades, n, seed, prec=F64):
    """n x K doubles strictly inside every term, term `near` at a relative distance close to `target` (None: order one), the
    others at order-one distances where their columns are still free; plus the reference at those rows.  Rows that miss (a
    term whose columns were all given is infeasible or closer than MIN_DIST, the near term off target by more than 8, an
    intermediate out of RANGE) are dropped, so fewer than n rows may come back.  For another working precision the rows are
    generated in double all the same, then rounded to it, and the reference AT THE ROUNDED ROWS decides what is kept (its
    range, its MIN_DIST)."""
    rng = np.random.default_rng(seed)
    m = 8 * n
    Y = np.zeros((m, K), dtype=LD)
    free = np.ones(K, dtype=bool)
    for ti in [near] + [i for i in range(len(terms)) if i != near]:
        T = parse(terms[ti])
        d = rng.uniform(0.25, 1.0, m).astype(LD) if (ti != near or target is None) else np.full(m, target, dtype=LD)
        (_fill_cone if T["kind"] == 0 else _fill_half)(T, Y, free, d, rng, decades)
    for c in range(K):
        if free[c]:
            Y[:, c] = _magnitudes(rng, m, decades) * rng.choice([-1.0, 1.0], m)
    with np.errstate(all="ignore"):
        Y64 = Y.astype(np.float64)
    if prec is not F64:
        Y64 = prec.rnd(Y64)
    Y64 = Y64[np.all(np.isfinite(Y64), axis=1)]
    R = reference(terms, Y64, prec=prec)
    with np.errstate(all="ignore"):
        keep = R.feasible & R.in_range & np.all(R.dist >= prec.min_dist, axis=1)
        if target is not None:
            keep &= (R.dist[:, near] <= 8 * target) & (R.dist[:, near] >= target / 8)
    rows = np.flatnonzero(keep)[:n]
    return Y64[rows]


def classes(rows_per_class=200, seed=20260101, prec=F64, only=None):
    """The sweep: for every case of the table (only: the cases with these indices, the same rows as in the whole sweep), every
    regime of the working precision and every term as the near-active one, a batch of rows.  Yields (label, K, terms, Y)."""
    for ci, (name, K, terms) in enumerate(CASES):
        if only is not None and ci not in only:
            continue
        for ri, (rl, target, decades) in enumerate(prec.regimes):
            if decades > 3 and len(terms) > 1:
                continue                       # the wide scales run on the single terms
            for near in range(len(terms)):
                Y = generate(terms, K, near, target, decades, rows_per_class, seed + 1000 * ci + 10 * ri + near, prec)
                label = "%s | %s" % (name, rl) + (" | near term %d" % near if len(terms) > 1 else "")
                yield label, K, terms, Y


def hand_made():
    """Rows with an exactly representable answer F = +inf: (K, terms, Y, what)."""
    nan = float("nan")
    return [
        (3, [([0, 1, 2], 1.0)], [[3.0, 4.0, 5.0]], "p = 1, (q, s) = (3, 4, 5): phi = 0 exactly"),
        (3, [([0, 1, 2], 2.0)], [[3.0, 4.0, 25.0]], "p = 2, (q, s) = (3, 4, 25): phi = 0 exactly"),
        (3, [([0, 1, 2], 1.5)], [[0.0, 0.0, 0.0]], "s = 0"),
        (3, [([0, 1, 2], 1.5)], [[0.0, 0.0, -1.0], [0.1, 0.1, -2.0]], "s < 0"),
        (3, [([0, 1, 2], 3.0)], [[2.0, 0.0, 1.0], [1.0, 1.0, 1.0]], "phi < 0"),
        (3, [([0, 1, 2], 1.0)], [[nan, 0.0, 1.0], [0.0, 0.0, nan]], "a NaN entry"),
        (4, [([0, 1, 2], 1.0, 3)], [[3.0, 4.0, 7.0, -2.0], [0.0, 0.0, 1.0, -1.0]], "is2: s + s2 on / outside the boundary"),
        (2, [("linear", [0, 1], [1.0, -1.0], 0.5)], [[1.0, 1.5]], "half space: affine form 0"),
        (2, [("linear", [0, 1], [1.0, -1.0], 0.5)], [[1.0, 2.0]], "half space: affine form < 0"),
        (4, [([1, 2, 3], 1.5), ("linear", [0], [1.0], -1.0)], [[0.5, 0.1, 0.1, 1.0], [2.0, 3.0, 0.0, 1.0]],
         "intersection: one term violated, the other satisfied"),
    ]


def float_representable(Y):
    """Per row of Y: every entry is a float32 (NaN counts as one)."""
    Y = np.asarray(Y, dtype=np.float64)
    with np.errstate(all="ignore"):
        back = Y.astype(np.float32).astype(np.float64)
    return np.all((back == Y) | np.isnan(Y), axis=1)


def rounding_rows():
    """Rows whose class is decided by the rounding to float: (K, terms, row, outside_in_float, what).  Every row is strictly
    feasible in double.  outside_in_float = True: the rounded row lies on or outside the boundary, F = +inf exactly in float
    while the double value stays finite; False: the rounded row is inside by more than the float bound of phi, F is finite."""
    e30, e18 = 2.0 ** -30, 2.0 ** -18
    half = [("linear", [0, 1], [1.0, -1.0], 0.5)]
    return [
        (3, [([0, 1, 2], 1.0)], [3.0, 4.0, 5.0 * (1 + e30)], True, "p = 1, s = 5 (1 + 2^-30) rounds to 5: phi = 0 in float"),
        (3, [([0, 1, 2], 2.0)], [3.0, 4.0, 25.0 * (1 + e30)], True, "p = 2, s = 25 (1 + 2^-30) rounds to 25: phi = 0 in float"),
        (3, [([0, 1, 2], 1.0)], [3.0 + 0.9 * 2.0 ** -22, 4.0, 5.0 + 0.28 * 2.0 ** -21], True,
         "p = 1, q_1 rounds up and s down: phi < 0 in float"),
        (4, [([0, 1, 2], 1.0, 3)], [3.0, 4.0, 7.0, -2.0 * (1 - e30)], True, "is2: s + s2 rounds to 5: phi = 0 in float"),
        (2, half, [1.0, 1.5 * (1 - e30)], True, "half space: y_2 rounds to 1.5, affine form 0 in float"),
        (2, half, [1.0 - 0.9 * 2.0 ** -24, 1.5 - 0.95 * 2.0 ** -24], True, "half space: y_1 rounds down to 1 - 2^-24, y_2 up to 1.5: form < 0"),
        (3, [([0, 1, 2], 1.0)], [3.0, 4.0, 5.0 * (1 + e18 + e30)], False, "p = 1, s rounds to 5 (1 + 2^-18): inside in float"),
        (3, [([0, 1, 2], 2.0)], [3.0, 4.0, 25.0 * (1 + e18 + e30)], False, "p = 2, s rounds to 25 (1 + 2^-18): inside in float"),
        (4, [([0, 1, 2], 1.0, 3)], [3.0, 4.0, 7.0, -2.0 * (1 - e18 - e30)], False, "is2: s + s2 rounds to 5 + 2^-17: inside in float"),
        (2, half, [1.0, 1.5 * (1 - e18 - e30)], False, "half space: the affine form rounds to 1.5 2^-18 in float"),
    ]


# ---------------------------------------------------------------------------------------------------------- levels
def _padded(Bk):
    Bk = sp.csr_matrix(Bk)
    n = Bk.shape[0]
    cnt = np.diff(Bk.indptr)
    m = max(int(cnt.max()) if n else 0, 1)
    cols, vals = np.zeros((n, m), dtype=np.int64), np.zeros((n, m), dtype=LD)
    rows = np.repeat(np.arange(n), cnt)
    pos = np.arange(Bk.nnz) - np.repeat(Bk.indptr[:-1], cnt)
    cols[rows, pos], vals[rows, pos] = Bk.indices, Bk.data
    return cols, vals


def _sum_by_key(keys, vals, size):
    """out[k] = sum of vals with key k, in long double (sort + reduceat: np.add.at is slow for long double)."""
    out = np.zeros(size, dtype=LD)
    nz = vals != 0
    keys, vals = keys[nz], vals[nz]
    if keys.size:
        order = np.argsort(keys, kind="stable")
        keys, vals = keys[order], vals[order]
        starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
        out[keys[starts]] = np.add.reduceat(vals, starts)
    return out


def spmv_reference(A, x):
    """(A x in long double, its any-order fp64 bound (m + 2) |A| |x| in units of u, m = longest row)."""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    y = _sum_by_key(rows, A.data.astype(LD) * np.asarray(x, dtype=LD)[A.indices], A.shape[0])
    m = int(np.diff(A.indptr).max()) if A.nnz else 0
    return y, (m + 2) * (abs(A) @ np.abs(np.asarray(x, dtype=np.float64)))


class Level:
    pass


def level_reference(B, K, w, c, t, Dz, terms, a_node=None, mu_node=None, mask=None, hessian=True, prec=F64):
    """Exact objective, gradient and Hessian of a level at the rows Dz (n x K doubles), with bounds (units of prec.u) that hold
    for any order of summation in the working precision; B, w, c, t and Dz are rounded to it first.  B: CSR, n K x N, row
    q K + k.

      f0F = sum_q w_q F_q               bound  sum_q w_q (bF_q + |F_q|) + (n - 1) sum_q |w_q F_q|
      f0C = sum_q w_q <c_q, Dz_q>       bound  sum_q w_q ((K + 1) sum_k |c_qk Dz_qk| + |<c_q, Dz_q>|) + (n - 1) sum_q |w_q <c_q, Dz_q>|
      g   = B' (w (F1 + t c))           bound  |B|' (w bF1 + 2 |t c| w) + (m + 2) |B|' |w (F1 + t c)|,      m = longest column of B
      H   = B' diag(w F2) B             bound  |B|' (w bF2) |B| + (m K + 2) |B|' |w F2| |B|
      H v                               bound  (bound of H) |v| + (r + 2) (|B|' |w F2| |B|) |v|,           r = longest row of H"""
    B = sp.csr_matrix(B)
    Dz = np.ascontiguousarray(Dz, dtype=np.float64)
    if prec is not F64:
        B = B.copy()                          # a matrix of its own: sorting one that shares index arrays would disturb the caller's
        B.data = prec.rnd(B.data)
        Dz, w, c, t = np.ascontiguousarray(prec.rnd(Dz)), prec.rnd(w), prec.rnd(c), float(prec.rnd(t))
    n, N = Dz.shape[0], B.shape[1]
    assert B.shape[0] == n * K and Dz.shape[1] == K
    R = reference(terms, Dz, a_node, mu_node, mask, prec=prec)
    Lv = Level()
    Lv.rows = R
    wl, cl, Dl = np.asarray(w, dtype=LD), np.asarray(c, dtype=LD), Dz.astype(LD)
    wF = wl * R.F
    Lv.f0F = wF.sum()
    Lv.b_f0F = float((wl * (R.bF + np.abs(R.F))).sum() + (n - 1) * np.abs(wF).sum())
    lin = (cl * Dl).sum(axis=1)
    Lv.f0C = (wl * lin).sum()
    Lv.b_f0C = float((wl * ((K + 1) * np.abs(cl * Dl).sum(axis=1) + np.abs(lin))).sum() + (n - 1) * np.abs(wl * lin).sum())
    Babs = abs(B)
    m = int(np.bincount(B.indices, minlength=N).max()) if B.nnz else 0
    v = wl[:, None] * (R.F1 + LD(t) * cl)
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    Lv.g = _sum_by_key(B.indices.astype(np.int64), B.data.astype(LD) * v.reshape(-1)[rows], N)
    bv = wl[:, None] * R.bF1 + 2 * np.abs(LD(t) * cl) * wl[:, None] + (m + 2) * np.abs(v)
    Lv.b_g = Babs.T @ bv.reshape(-1).astype(np.float64)
    if not hessian:
        return Lv
    wH = wl[:, None, None] * R.F2
    pads = [_padded(B[k::K]) for k in range(K)]
    keys, vals = [], []
    for k in range(K):
        for l in range(K):
            d = wH[:, k, l]
            if not np.any(d != 0):
                continue
            (ck, vk), (cl_, vl) = pads[k], pads[l]
            vals.append((vk[:, :, None] * d[:, None, None] * vl[:, None, :]).reshape(-1))
            keys.append((ck[:, :, None] * N + cl_[:, None, :]).reshape(-1))
    Lv.H = _sum_by_key(np.concatenate(keys), np.concatenate(vals), N * N).reshape(N, N)
    q = np.repeat(np.arange(n), K * K)
    kk = np.tile(np.repeat(np.arange(K), K), n)
    ll = np.tile(np.arange(K), n * K)
    blk = lambda X: sp.csr_matrix((np.asarray(X, dtype=np.float64).reshape(-1), (q * K + kk, q * K + ll)), shape=(n * K, n * K))
    Lv.H_abs = (Babs.T @ blk(np.abs(wH)) @ Babs).toarray()
    Lv.b_H = (Babs.T @ blk(wl[:, None, None] * R.bF2) @ Babs).toarray() + (m * K + 2) * Lv.H_abs
    Lv.H_rowlen = int((Lv.H_abs != 0).sum(axis=1).max())
    return Lv


def hessian_apply_reference(Lv, v):
    vl = np.asarray(v, dtype=LD)
    return Lv.H @ vl, Lv.b_H @ np.abs(v) + (Lv.H_rowlen + 2) * (Lv.H_abs @ np.abs(v))


def diag_reference(Lv):
    """(diag(H) in long double, its bound diag(b_H)): every diagonal entry is one of the sums that make up H."""
    return np.diagonal(Lv.H).copy(), np.diagonal(Lv.b_H).copy()


def hessian_apply_matrix_free(B, K, w, R, v, rows_per_el=None):
    """H v = B' ((w F2) (B v)) without forming H, for levels too large for a dense N x N long-double H: three keyed long-double
    sums (B v by row, (w F2) d by node and D-row, B' u by column) from the rows R = reference(terms, Dz).  The bound is
    hessian_apply_reference's, term by term, with every product by |H| or b_H replaced by three fp64 sparse products:

        |B|' (w bF2) (|B| |v|)  +  (m K + 2 + r + 2) |B|' (|w F2| (|B| |v|)),     m = longest column of B, r = longest row of H

    r comes from the sparsity pattern of |B|' |w F2| |B|, held as a sparse matrix; where that product is itself too large, give
    rows_per_el (the rows of B come in element blocks of that many): r is then the largest number of unknowns that share an
    element with one unknown, which is never smaller."""
    B = sp.csr_matrix(B)
    n, N = R.F2.shape[0], B.shape[1]
    assert B.shape[0] == n * K and R.F2.shape[1:] == (K, K)
    wl, vl = np.asarray(w, dtype=LD), np.asarray(v, dtype=LD)
    rows = np.repeat(np.arange(B.shape[0], dtype=np.int64), np.diff(B.indptr))
    cols = B.indices.astype(np.int64)
    Bl = B.data.astype(LD)
    d = _sum_by_key(rows, Bl * vl[cols], n * K).reshape(n, K)
    wH = wl[:, None, None] * R.F2
    nk = np.arange(n * K, dtype=np.int64).reshape(n, K)
    key = np.broadcast_to(nk[:, :, None], (n, K, K))
    u = _sum_by_key(key.reshape(-1), (wH * d[:, None, :]).reshape(-1), n * K)
    hv = _sum_by_key(cols, Bl * u[rows], N)
    # the bound, in fp64: node-block-diagonal matrices of |w F2| and w bF2 between |B|' and |B|
    q = np.repeat(np.arange(n), K * K)
    kk = np.tile(np.repeat(np.arange(K), K), n)
    ll = np.tile(np.arange(K), n * K)
    blk = lambda X: sp.csr_matrix((np.asarray(X, dtype=np.float64).reshape(-1), (q * K + kk, q * K + ll)), shape=(n * K, n * K))
    Babs = abs(B)
    Habs_blk, bH_blk = blk(np.abs(wH)), blk(wl[:, None, None] * R.bF2)
    m = int(np.bincount(B.indices, minlength=N).max()) if B.nnz else 0
    if rows_per_el is None:
        pat = sp.csr_matrix(Babs.T @ Habs_blk @ Babs)
        pat.eliminate_zeros()
    else:
        el = np.unique((rows // rows_per_el) * N + cols)
        E = sp.csr_matrix((np.ones(len(el)), (el // N, el % N)), shape=(B.shape[0] // rows_per_el, N))
        pat = sp.csr_matrix(E.T @ E)
    r = int(np.diff(pat.indptr).max()) if pat.nnz else 0
    bv = Babs @ np.abs(np.asarray(v, dtype=np.float64))
    bound = Babs.T @ (bH_blk @ bv) + (m * K + 2 + r + 2) * (Babs.T @ (Habs_blk @ bv))
    return hv, bound


def interleave(Dk):
    """B with row q K + k = row q of Dk[k] (K matrices of n rows each)."""
    K, n = len(Dk), Dk[0].shape[0]
    perm = (np.arange(n)[:, None] + n * np.arange(K)[None, :]).reshape(-1)
    return sp.csr_matrix(sp.vstack(Dk, format="csr")[perm])


# ---------------------------------------------------------------------------------------------------------- fp64 baseline
def oracle_set(terms, p_node=None, mask=None):
    """The oracle's convex set (oracle/mgb_oracle.py) for a term list: the independent fp64 code whose ratios are the
    yardstick (rho_base) the device is held to.  p_node: n x nterms per-node exponents; mask: n x nterms booleans."""
    import mgb_oracle as O
    sets = []
    for ti, term in enumerate(terms):
        T = parse(term)
        if T["kind"] == 1:
            sets.append(O.LinearBarrier(list(T["q"]), list(T["coef"]), T["off"]))
        else:
            Q = O.convex_Euclidian_power(T["q"] + [T["s"]], T["p"] if p_node is None else np.asarray(p_node)[:, ti])
            Q.idx_s2 = T["s2"]
            sets.append(Q)
    if mask is not None:
        return O.ConvexPiecewise(sets, np.asarray(mask, dtype=bool))
    return sets[0] if len(sets) == 1 else O.ConeIntersection(sets)


def rho_base(terms, Y, R, p_node=None, mask=None):
    """(ratio of F, of F1, of F2) of the oracle's fp64 rows against the reference R at the rows Y."""
    Q = oracle_set(terms, p_node, mask)
    with np.errstate(all="ignore"):
        return (ratio(Q.F(None, Y), R.F, R.bF), ratio(Q.F1(None, Y), R.F1, R.bF1), ratio(Q.F2(None, Y), R.F2, R.bF2))


# ---------------------------------------------------------------------------------------------------------- float baseline
def _pow_a32(s, a):
    return np.where(a == np.float32(2), s * s, np.where(a == np.float32(1), s, np.power(s, a)))


def rows_f32(terms, Y32, a_node=None, mu_node=None, mask=None, mutate=None):
    """F (n), F1 (n, K), F2 (n, K, K) of the rows Y32 in plain numpy float32: the float baseline, the counterpart of the fp64
    oracle in rho_base.  Written from the formulas of csrc/kernels_tpl.hpp (load_cone, pow_a, barrier_value and the f1 / f2
    kernels with unit weight) without calling the library or the oracle; every operation is a float32 numpy operation in the
    kernels' order.  F is +inf on an infeasible row; F1 and F2 are unspecified there.  `mutate` plants one error for the tests
    of the check itself: "slot" swaps the output slots of a term's first q column and its last column (the next column of the
    row if the term has only one), "mu" uses mu + 1, "a-1" uses the exponent a - 1 where a - 2 belongs."""
    f = np.float32
    assert mutate in (None, "slot", "mu", "a-1")
    Y = np.ascontiguousarray(Y32, dtype=f)
    n, K = Y.shape
    one, two, four = f(1), f(2), f(4)
    F, G, H = np.zeros(n, dtype=f), np.zeros((n, K), dtype=f), np.zeros((n, K, K), dtype=f)
    with np.errstate(all="ignore"):
        for ti, term in enumerate(terms):
            T = parse(term)
            act = np.ones(n, dtype=bool) if mask is None else np.asarray(mask)[:, ti] != 0
            g, h = np.zeros((n, K), dtype=f), np.zeros((n, K, K), dtype=f)
            if T["kind"] == 1:
                coef = [f(c) for c in T["coef"]]
                phi = np.full(n, f(T["off"]), dtype=f)
                for i, ci in zip(T["q"], coef):
                    phi = phi + ci * Y[:, i]
                ok = phi > 0
                Ft = -np.log(phi)
                ip2 = one / (phi * phi)
                for i, ci in zip(T["q"], coef):
                    g[:, i] = -(ci / phi)
                    for j, cj in zip(T["q"], coef):
                        h[:, i, j] = ci * cj * ip2
            else:
                a = np.full(n, f(a_of(T["p"])), dtype=f) if a_node is None else np.asarray(a_node)[:, ti].astype(f)
                mu = np.full(n, f(mu_of(T["p"])), dtype=f) if mu_node is None else np.asarray(mu_node)[:, ti].astype(f)
                q = [Y[:, i] for i in T["q"]]
                qq = np.zeros(n, dtype=f)
                for qi in q:
                    qq = qq + qi * qi
                s = Y[:, T["s"]] + Y[:, T["s2"]] if T["s2"] >= 0 else Y[:, T["s"]]
                ok = s > 0
                sa = np.where(ok, _pow_a32(s, a), f(-1))
                phi = sa - qq
                ok = ok & (phi > 0)
                if mutate == "mu":
                    mu = mu + one
                Ft = -np.log(phi) - mu * np.log(s)
                ds = a * _pow_a32(s, a - one)
                dds = np.where(a == one, f(0), a * (a - one) * _pow_a32(s, a - (one if mutate == "a-1" else two)))
                ip = one / phi
                ip2 = ip * ip
                gs = -ds / phi - mu / s
                hss = -dds * ip + ds * ds * ip2 + mu / (s * s)
                scols = [T["s"]] + ([T["s2"]] if T["s2"] >= 0 else [])
                for i, ci in enumerate(T["q"]):
                    g[:, ci] = two * q[i] / phi
                    for j, cj in enumerate(T["q"]):
                        h[:, ci, cj] = four * q[i] * q[j] * ip2 + (two * ip if i == j else f(0))
                    for cs in scols:
                        h[:, ci, cs] = h[:, cs, ci] = -two * q[i] * ds * ip2
                for cs in scols:
                    g[:, cs] = gs
                    for cs_ in scols:
                        h[:, cs, cs_] = hss
            if mutate == "slot":
                c0 = T["cols"][0]
                c1 = T["cols"][-1] if len(T["cols"]) > 1 else (c0 + 1) % K
                g[:, [c0, c1]] = g[:, [c1, c0]]
                h[:, [c0, c1], :] = h[:, [c1, c0], :]
                h[:, :, [c0, c1]] = h[:, :, [c1, c0]]
            F = F + np.where(act, np.where(ok, Ft, f(np.inf)), f(0))
            G = G + np.where(act[:, None], g, f(0))
            H = H + np.where(act[:, None, None], h, f(0))
    assert F.dtype == f and G.dtype == f and H.dtype == f
    return F, G, H


def rho_base32(terms, Y, R, a_node=None, mu_node=None, mask=None, mutate=None):
    """(ratio of F, of F1, of F2) of rows_f32 against the float reference R = reference(..., prec=F32) at the rows Y."""
    F, G, H = rows_f32(terms, Y, a_node, mu_node, mask, mutate)
    return (ratio(F, R.F, R.bF, prec=F32), ratio(G, R.F1, R.bF1, prec=F32), ratio(H, R.F2, R.bF2, prec=F32))


def level_f32(B, K, w, c, t, Dz, terms, a_node=None, mu_node=None, mask=None, hessian=True):
    """The level formulas in numpy float32 at the state Dz, the level baseline of the float kernels: (f0F, f0C, g, H) with the
    row values w F and w <c, Dz> formed in float and summed in double (as the kernels hand them to the double reduction),
    g = B' (w (F1 + t c)) and H = B' diag(w F2) B as float32 sparse products."""
    f = np.float32
    B32 = sp.csr_matrix(B).astype(f)          # a copy with index arrays of its own
    Y, w32, c32, t32 = np.asarray(Dz).astype(f), np.asarray(w).astype(f), np.asarray(c).astype(f), f(t)
    n = Y.shape[0]
    F, G, H = rows_f32(terms, Y, a_node, mu_node, mask)
    with np.errstate(all="ignore"):
        cd = np.zeros(n, dtype=f)
        for j in range(K):
            cd = cd + c32[:, j] * Y[:, j]
        f0F, f0C = float((w32 * F).astype(np.float64).sum()), float((w32 * cd).astype(np.float64).sum())
        g = B32.T @ (w32[:, None] * (G + t32 * c32)).reshape(-1)
        assert g.dtype == f
        if not hessian:
            return f0F, f0C, g, None
        q = np.repeat(np.arange(n), K * K)
        kk = np.tile(np.repeat(np.arange(K), K), n)
        ll = np.tile(np.arange(K), n * K)
        blk = sp.csr_matrix(((w32[:, None, None] * H).reshape(-1), (q * K + kk, q * K + ll)), shape=(n * K, n * K))
        Hd = (B32.T @ blk @ B32).toarray()
        assert Hd.dtype == f
    return f0F, f0C, g, Hd


def node_exponent_rows(rows_per_p=60, seed=7, prec=F64):
    """Rows for a power cone whose exponent varies from row to row and crosses p = 2 (mu takes all three values):
    (K, terms, Y, p_node); the term's own p is a placeholder, as in AMG(cones=[(idx, p(x))]).  The distances are those of the
    working precision's narrow regimes."""
    ps = [1.0, 1.1, 1.7, 2.0, 2.1, 2.6, 8.0]
    Ys, pn = [], []
    regimes = [(None, 3), (1e-4, 3), (1e-8, 3), (1e-11, 3)] if prec is F64 else [r[1:] for r in prec.regimes if r[2] <= 3]
    for i, p in enumerate(ps):
        for j, (target, decades) in enumerate(regimes):
            Y = generate([([1, 2, 3], p)], 4, 0, target, decades, rows_per_p // len(regimes), seed + 10 * i + j, prec)
            Ys.append(Y)
            pn.append(np.full(len(Y), p))
    return 4, [([1, 2, 3], 1.0)], np.vstack(Ys), np.concatenate(pn)[:, None]


def piecewise_rows(n=240, seed=11, prec=F64):
    """Rows for a piecewise set -- the cone everywhere, the half space on some rows only; where the half space is masked out
    half of the rows violate it (an inactive term constrains nothing): (K, terms, Y, mask).  The distances are those of the
    working precision's narrow regimes."""
    terms = [([1, 2, 3], 1.5), ("linear", [0], [1.0], -0.25)]
    rng = np.random.default_rng(seed)
    targets = (None, 1e-4, 1e-9) if prec is F64 else tuple(r[1] for r in prec.regimes if r[2] <= 3)
    Y = np.vstack([generate(terms, 4, near, target, 3, n // 6, seed + 10 * near + j, prec)
                   for near in (0, 1) for j, target in enumerate(targets)])
    mask = np.ones((len(Y), 2), dtype=bool)
    mask[:, 1] = rng.random(len(Y)) < 0.5
    out = ~mask[:, 1] & (rng.random(len(Y)) < 0.5)
    Y[out, 0] = -np.abs(Y[out, 0]) - 1.0
    return 4, terms, (Y if prec is F64 else prec.rnd(Y)), mask


# ---------------------------------------------------------------------------------------------------------- golden states
SMALL_GOLDENS = [("fem1d", 3, 1.0), ("fem1d", 4, 2.0), ("fem2d", 2, 1.5), ("fem2d", 3, 1.0), ("fem2d", 3, 2.0),
                 ("fem3d", 2, 1.0), ("fem3d", 2, 2.0)]      # CASES of test_gpu_parity.py


def golden_name(kind, L, p, large=False):
    return "%s%s_L%d_p%s.npz" % ("large_" if large else "", kind, L, str(p).replace(".", "_"))


def default_terms(dim, p):
    """The default barrier of AMG(geometry, p=p): one power cone on the last dim + 1 rows of the default D."""
    return [(list(range(1, dim + 2)), float(p))]


def level_matrices(geometry_operators, geometry_subspaces, state_variables, D, l, n):
    """(D as one CSR with row q K + k over the stacked state, B = D R_l likewise) from host matrices: operators[op] (n x n),
    subspaces[name][l] (n x N_name); a "fixed" state variable has no unknowns."""
    names = [sv[0] for sv in state_variables]
    Z = sp.csr_matrix((n, n))
    Dm = [sp.hstack([geometry_operators[op] if nm == var else Z for nm in names], format="csr") for var, op in D]
    R = sp.csr_matrix(sp.block_diag([sp.csr_matrix((n, 0)) if sv[1] == "fixed" else geometry_subspaces[sv[1]][l]
                                     for sv in state_variables], format="csr"))
    return interleave(Dm), interleave([sp.csr_matrix(Dk @ R) for Dk in Dm])


def oracle_level_baseline(Mo, l, z, c, t, terms, p_node=None, mask=None, hessian=True):
    """Level baseline: the oracle's fp64 f0 / f1 / f2 at the state z (n x S), s = 0, level l, against the exact values at the
    oracle's own fp64 Dz.  Returns (ratio f0, ratio f1, ratio f2, Level)."""
    import mgb_oracle as O
    K = len(Mo.D)
    zv = np.asarray(z, dtype=np.float64).reshape(-1, order="F")
    R = Mo.R[l]
    Bo = O.Barrier(oracle_set(terms, p_node, mask))
    Dz = Bo.apply_D(Mo.D, zv)
    B = interleave([sp.csr_matrix(Dk @ R) for Dk in Mo.D])
    an = None if p_node is None else a_of(p_node)
    mn = None if p_node is None else mu_of(p_node)
    Lv = level_reference(B, K, Mo.w, c, t, Dz, terms, a_node=an, mu_node=mn, mask=mask, hessian=hessian)
    s0 = np.zeros(R.shape[1])
    with np.errstate(all="ignore"):
        y = Bo.f0(s0, Mo.x, Mo.w, t * c, R, Mo.D, zv)
        g = Bo.f1(s0, Mo.x, Mo.w, t * c, R, Mo.D, zv)
        r0 = ratio(y, *f0_total(Lv, t))
        r1 = ratio(g, Lv.g, Lv.b_g)
        r2 = ratio(Bo.f2(s0, Mo.x, Mo.w, t * c, R, Mo.D, zv).toarray(), Lv.H, Lv.b_H) if hessian else 0.0
    return r0, r1, r2, Lv


def f0_total(Lv, t):
    """(f0 = f0F + t f0C, its bound: the parts' bounds plus the product and the sum)."""
    y = Lv.f0F + LD(t) * Lv.f0C
    return y, Lv.b_f0F + abs(t) * Lv.b_f0C + abs(float(LD(t) * Lv.f0C)) + abs(float(y))
