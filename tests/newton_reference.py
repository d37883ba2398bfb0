"""A numpy restatement of one Newton step and of the Newton loop's bookkeeping (csrc/amg.cpp: Amg::newton, amgb_step, solve;
oracle/mgb_oracle.py: newton, linesearch_backtracking, amgb_step, amgb_core), for the traces of AMG.set_trace.

Two kinds of statement, kept apart:

  decisions on computed sums  (replay_step)   The line search compares objective values -- sums over the nodes that fp64 forms
      in some order -- with one another and with the Armijo line, and every row's cone distance with a fraction of its value at
      the iterate.  The replay evaluates the objective and the distances at s_k - sigma nstep in long double from the traced
      s_k and the traced nstep (so the linear solver's error is not part of it), walks oracle.linesearch_backtracking statement
      by statement and calls a comparison AMBIGUOUS when its two sides differ by no more than the fp64 bound of the computed
      side(s): the depth-aware bound of the objective sums (linesearch_reference.f0_sums / f0_total, as test_gpu_linesearch.py
      holds the same sums to) plus the first-order effect of the SpMV bound of Dz = Dz0 + B x on them, times MARGIN.  It returns
      every step length reachable by deciding the ambiguous comparisons either way; a step without one is DECISIVE and has a
      single reachable length and a known number of objective evaluations.

  bookkeeping on recorded doubles  (replay_stop, replay_outer)   The running minima, the stagnation and decrement rules, the
      budget, the sequence of t, the history of kappa and the attempts of the first centre are functions of the traced doubles
      alone; the loop under test used these very doubles, so the restatement is exact and has no ambiguity.

reference_direction gives the exact gradient and Hessian at the iterate (barrier_reference.level_reference), n = H \\ g by the
refined solve of chol_reference.Reference and inc_ref = <g, n>; oracle_direction the fp64 yardstick: oracle f1, f2 and solve
(splu) on the same matrices at the same point."""
import math

import numpy as np
import scipy.sparse as sp

import barrier_reference as BR
import chol_reference as CR
import linesearch_reference as LR
import mgb_oracle as O

LD = BR.LD
U = BR.U
MARGIN = 4.0                      # test_gpu_linesearch.py MARGIN: what the objective sums are held to over their bound
ARMIJO, BETA, MIN_STEP, FRAC = O.ARMIJO, O.BETA, O.MIN_STEP, O.FRAC_TO_BOUNDARY
assert FRAC == LR.FRAC
KMAX = int(math.floor(-math.log2(MIN_STEP)))       # the smallest step length tried is 2^-KMAX
assert 2.0 ** -KMAX >= MIN_STEP > 2.0 ** -(KMAX + 1)

# trace columns (AMG.TRACE_CENTERING, AMG.TRACE_STEP)
C_LEVEL, C_T, C_FINEST, C_FINAL, C_BUDGET, C_K, C_CONVERGED, C_FIRST, C_STEPS = range(9)
S_CENT, S_Y, S_G, S_YMIN, S_GMIN, S_INC, S_STEP, S_YNEXT, S_GNEXT, S_PIVOT, S_MODE, S_CONSUMED, S_EVALS, S_REASON = range(14)
R_NONE, R_INC, R_DECREMENT, R_STAGNATION, R_BUDGET, R_PIVOT, R_NONFINITE = range(7)


class LevelData:
    """What the objective of a level is made of.  B: CSR (n K) x N, row q K + k; w (n); c (n, K), NOT scaled by t; terms in the
    library's syntax (power cones with a scalar exponent and half spaces); depth: the longest chain of additions of the
    objective's sums (linesearch_reference.depth_trial(n) for the device, n - 1 for any order)."""

    def __init__(self, B, K, w, c, terms, depth=None, mask=None):
        self.B = sp.csr_matrix(B)
        self.K, self.w, self.c, self.terms, self.mask = K, np.asarray(w, dtype=np.float64), np.asarray(c, dtype=np.float64), terms, mask
        self.n = len(self.w)
        self.N = self.B.shape[1]
        assert self.B.shape[0] == self.n * K and self.c.shape == (self.n, K)
        self.depth = self.n - 1 if depth is None else depth
        self.Bk = [sp.csr_matrix(self.B[k::K]) for k in range(K)]


class Point:
    pass


def _dphi(terms, dz, bdz):
    """first-order bound (units of u) of the change of every term's cone distance when dz moves by bdz u"""
    n = dz.shape[0]
    out = np.zeros((n, len(terms)))
    with np.errstate(all="ignore"):
        for ti, term in enumerate(terms):
            T = BR.parse(term)
            if T["kind"] == 1:
                for i, cf in zip(T["q"], T["coef"]):
                    out[:, ti] += abs(cf) * bdz[:, i]
                continue
            for i in T["q"]:
                out[:, ti] += 2.0 * np.abs(dz[:, i]) * bdz[:, i]
            s = dz[:, T["s"]] + (dz[:, T["s2"]] if T["s2"] >= 0 else 0.0)
            a = BR.a_of(T["p"])
            bs = bdz[:, T["s"]] + (bdz[:, T["s2"]] if T["s2"] >= 0 else 0.0)
            out[:, ti] += np.where(s > 0, a * np.abs(s) ** (a - 1.0), 0.0) * bs
    return out


def evaluate(lv, t, Dz0, x):
    """The objective and the cone distances at x (N long doubles or doubles) with their fp64 bounds, in units of u."""
    P = Point()
    xl = np.asarray(x, dtype=LD)
    bs, bb = BR.spmv_reference(lv.B, np.asarray(xl, dtype=np.float64))
    dzl = np.asarray(Dz0, dtype=np.float64).reshape(-1).astype(LD) + _spmv_ld(lv.B, xl)
    P.dz = np.asarray(dzl, dtype=np.float64).reshape(lv.n, lv.K)
    P.bdz = (bb + np.abs(P.dz).reshape(-1)).reshape(lv.n, lv.K) + 1.0       # SpMV, the addition of Dz0, the rounding of P.dz itself
    rows = BR.reference(lv.terms, P.dz, mask=lv.mask)
    P.rows = rows
    P.phi, P.bphi = rows.phi, np.asarray(rows.bphi, dtype=np.float64) + _dphi(lv.terms, P.dz, P.bdz)
    P.feasible = bool(rows.feasible.all())
    if not P.feasible:
        P.y, P.by = LD(np.inf), 0.0
        return P
    S = LR.f0_sums(rows, lv.w, lv.c, P.dz, lv.depth)
    P.y, by = LR.f0_total(S, t)
    grad = np.abs(np.asarray(rows.F1, dtype=np.float64) + t * lv.c)
    P.by = by + float((lv.w[:, None] * grad * P.bdz).sum())
    return P


def _spmv_ld(A, xl):
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return BR._sum_by_key(rows, A.data.astype(LD) * xl[A.indices], A.shape[0])


class StepReplay:
    """reachable: the step lengths the line search may return (0.0: rejected); decisive: no comparison on any path was
    ambiguous (then reachable has one element); sigma, evals: the length and the number of objective evaluations on the path
    that decides every comparison by the exact values; ambiguous: the comparisons found ambiguous, as text."""


def replay_step(lv, t, Dz0, s_k, nstep, y_k, inc, phi_ref=None, bphi_ref=None):
    """oracle.linesearch_backtracking from (s_k, y_k) along -nstep with the decrement inc, all as recorded.  phi_ref, bphi_ref:
    the cone distances of the iterate and their bound (default: evaluated at s_k)."""
    sk, nl = np.asarray(s_k, dtype=LD), np.asarray(nstep, dtype=LD)
    if phi_ref is None:
        P0 = evaluate(lv, t, Dz0, sk)
        phi_ref, bphi_ref = P0.phi, P0.bphi
    phi_ref64 = np.asarray(phi_ref, dtype=np.float64)
    cache, amb = {}, []
    y_k, inc = np.float64(y_k), np.float64(inc)

    def point(k):
        if k not in cache:
            sigma = np.float64(2.0 ** -k)
            P = evaluate(lv, t, Dz0, sk - LD(sigma) * nl)
            act = np.isfinite(np.asarray(phi_ref64))
            with np.errstate(all="ignore"):
                lhs, rhs = np.asarray(P.phi, dtype=LD), LD(FRAC) * np.asarray(phi_ref, dtype=LD)
                tol = MARGIN * U * (P.bphi + FRAC * np.asarray(bphi_ref, dtype=np.float64) + np.abs(np.asarray(rhs, dtype=np.float64)))
                gap = np.where(act, np.asarray(lhs - rhs, dtype=np.float64), np.inf)
                # inside the cone at all: phi > 0 with the same tolerance
                pos = np.where(act, np.asarray(P.phi, dtype=np.float64), np.inf)
            close = (np.abs(gap) <= tol) | (np.abs(pos) <= MARGIN * U * P.bphi)
            ok_exact = P.feasible and bool((gap >= 0).all())
            # the trial's value is finite: possible outcomes, with the close rows decided either way
            P.finite = set()
            if _could_pass(gap, pos, close):
                P.finite.add(True)
            if not ok_exact or close.any():
                P.finite.add(False)
            if len(P.finite) == 2:
                amb.append("sigma 2^-%d: a row's cone distance within its bound of the threshold" % k)
            P.finite_exact = ok_exact
            P.sigma = sigma
            cache[k] = P
        return cache[k]

    def armijo(k):
        """possible outcomes of `finite(yA) and yA <= y - ARMIJO sigma inc`, and the exact one"""
        P = point(k)
        line = y_k - ARMIJO * P.sigma * inc                      # fp64, the loop's own expression
        out = set()
        exact = False
        if True in P.finite:
            d = float(P.y - LD(line)) if P.feasible else np.inf
            tol = MARGIN * U * P.by
            if abs(d) <= tol:
                out |= {True, False}
                amb.append("sigma 2^-%d: Armijo within %.1f bounds" % (k, abs(d) / max(U * P.by, 1e-300)))
            else:
                out.add(d <= 0)
            exact = P.finite_exact and d <= 0
        if False in P.finite:
            out.add(False)
        return out, exact

    def improves(k):
        """possible outcomes of `finite(yB) and yB < yA` for B = k + 1, A = k, and the exact one"""
        A, Bp = point(k), point(k + 1)
        out = set()
        exact = False
        if True in Bp.finite:
            d = float(Bp.y - A.y) if Bp.feasible else np.inf
            tol = MARGIN * U * (A.by + Bp.by)
            if abs(d) <= tol:
                out |= {True, False}
                amb.append("sigma 2^-%d against 2^-%d: objectives within %.1f bounds" % (k + 1, k, abs(d) / max(U * (A.by + Bp.by), 1e-300)))
            else:
                out.add(d < 0)
            exact = Bp.finite_exact and d < 0
        if False in Bp.finite:
            out.add(False)
        return out, exact

    memo_r, memo_o = {}, {}

    def refine(k):
        if k not in memo_r:
            if k + 1 > KMAX:
                memo_r[k] = {2.0 ** -k}
            else:
                out, _ = improves(k)
                res = set()
                if False in out:
                    res.add(2.0 ** -k)
                if True in out:
                    res |= refine(k + 1)
                memo_r[k] = res
        return memo_r[k]

    def outer(k):
        if k not in memo_o:
            if k > KMAX:
                memo_o[k] = {0.0}
            else:
                out, _ = armijo(k)
                res = set()
                if True in out:
                    res |= refine(k)
                if False in out:
                    res |= outer(k + 1)
                memo_o[k] = res
        return memo_o[k]

    R = StepReplay()
    R.reachable = outer(0)
    R.ambiguous = list(amb)
    R.decisive = not amb
    # the path of the exact values, with its evaluations
    seen, k, sigma = set(), 0, 0.0
    while k <= KMAX:
        seen.add(k)
        if armijo(k)[1]:
            while k + 1 <= KMAX:
                seen.add(k + 1)
                if not improves(k)[1]:
                    break
                k += 1
            sigma = 2.0 ** -k
            break
        k += 1
    R.sigma, R.evals, R.visited = sigma, len(seen), sorted(seen)
    del amb[len(R.ambiguous):]
    R.point = cache.get(int(round(-math.log2(sigma)))) if sigma > 0 else None
    assert not R.decisive or R.reachable == {R.sigma}
    return R


def _could_pass(gap, pos, close):
    """with the close rows decided in favour of the point, does every row pass?"""
    return bool(((gap >= 0) | close).all() and ((pos > 0) | close).all())


# ------------------------------------------------------------------------------------------------------------ the direction
def _lower_csr(H):
    Lo = sp.csr_matrix(sp.tril(sp.csr_matrix(H)))
    Lo.sort_indices()
    return Lo.indptr, Lo.indices, Lo.data


def reference_direction(lv, t, Dz):
    """(g, n, inc_ref, floor): the exact gradient and Hessian at the rows Dz (n x K doubles: the iterate's) in long double,
    H n = g by the refined solve of chol_reference.Reference on H rounded to doubles, inc_ref = <g, n>, and `floor`, the
    relative change of inc_ref that the fp64 bounds of g and H account for."""
    Lv = BR.level_reference(lv.B, lv.K, lv.w, lv.c, t, Dz, lv.terms, mask=lv.mask, hessian=True)
    H64 = np.asarray(Lv.H, dtype=np.float64)
    rp, ci, lower = _lower_csr(sp.csr_matrix(H64))
    ref = CR.Reference(rp, ci, lower, lv.N)
    # the right-hand side keeps its long double digits: the residual is formed in long double
    g64 = np.asarray(Lv.g, dtype=np.float64)
    x = ref.solve(g64)["x_ref"]
    for _ in range(2):
        r = Lv.g - np.add.reduceat(ref._data * x[ref.H.indices], ref._starts)
        x = x + ref.lu.solve(np.asarray(r / ref.D.astype(LD), dtype=np.float64)).astype(LD) / ref.D.astype(LD)
    inc = (Lv.g * x).sum()
    # what the fp64 bounds of g and H alone do to inc = g' H^-1 g, to first order: 2 n' dg - n' dH n with |dg| <= b_g u,
    # |dH| <= b_H u.  No fp64 evaluation of the step can be asked for less; it is the floor under the oracle's own error.
    na = np.abs(np.asarray(x, dtype=np.float64))
    floor = U * (2.0 * float(Lv.b_g @ na) + float(na @ (Lv.b_H @ na))) / abs(float(inc))
    return Lv.g, x, inc, floor


def oracle_direction(lv, t, Dz):
    """inc of the fp64 oracle step: oracle Barrier.f1 and f2 (hessian_recipe) on the rows of B, oracle solve (splu)."""
    Q = BR.oracle_set(lv.terms, None, lv.mask)
    Bo = O.Barrier(Q)
    N = lv.N
    I = sp.identity(N, format="csr")
    pre = (np.asarray(Dz, dtype=np.float64), [sp.csr_matrix((lv.n, N))] * lv.K)
    s0 = np.zeros(N)
    with np.errstate(all="ignore"):
        g = Bo.f1(s0, None, lv.w, t * lv.c, I, lv.Bk, None, pre)
        H = Bo.f2(s0, None, lv.w, t * lv.c, I, lv.Bk, None, pre)
        n = O.solve(H, g)
    return float(np.dot(g, n))


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def replay_stop(cent, steps, w_min):
    """Amg::newton's bookkeeping on the recorded doubles of one centering.  cent: its trace row, steps: its step rows.  Returns
    (k, converged, reasons, ymin, gmin): what the loop must have reported, the reason of every step and the running minima
    BEFORE every step."""
    finest, final, budget = bool(cent[C_FINEST]), bool(cent[C_FINAL]), int(cent[C_BUDGET])
    theta = 0.1 if finest else 0.5
    dec_tol = O.DECREMENT_FRAC * w_min if finest else math.sqrt(w_min) / 2
    reasons, ymins, gmins = [], [], []
    converged, k = False, 0
    ymin = gmin = None
    for row in steps:
        assert not converged and k < budget, "the loop went on after it had ended"
        k += 1
        if ymin is None:
            ymin, gmin = row[S_Y], row[S_G]
        ymins.append(ymin)
        gmins.append(gmin)
        inc = row[S_INC]
        if row[S_PIVOT]:
            reasons.append(R_PIVOT)
            break
        if not math.isfinite(inc):
            reasons.append(R_NONFINITE)
            break
        if inc <= 0:
            converged = True
            reasons.append(R_INC)
            break
        ynext, gnext = row[S_YNEXT], row[S_GNEXT]
        exact = ynext >= ymin and gnext >= theta * gmin
        small = (not (finest and final)) and inc < dec_tol
        if small or exact:
            converged = True
        reasons.append(R_DECREMENT if small else R_STAGNATION if exact else R_BUDGET if k >= budget else R_NONE)
        ymin, gmin = min(ymin, ynext), min(gmin, gnext)
    return k, converged, reasons, ymins, gmins


def replay_outer(cents, L, tol=None, t0=0.1, kappa0=10.0, max_newton=48, schedule_all=False, maxit=10000):
    """Amg::solve / oracle.amgb_core (stop rule "fixed", centering "exact") on the recorded (level, k, converged) of the
    newton() calls: returns dict(t: the t every call must have run at, final: its `final`, level: its level, its (L x nt), ts,
    kappas: kappa after every continuation step).  Levels without unknowns run no newton() and are skipped here as there."""
    tol = math.sqrt(np.finfo(np.float64).eps) if tol is None else tol
    levels = list(range(L)) if schedule_all else [L - 1]
    present = sorted({int(c[C_LEVEL]) for c in cents})
    levels = [l for l in levels if l in present]
    pos = [0]
    want_t, want_final, want_level = [], [], []

    def amgb_step(t, final):
        its = np.zeros(L, dtype=np.int64)
        conv = True
        for J in levels:
            assert pos[0] < len(cents), "the trace ends before the solve does"
            c = cents[pos[0]]
            pos[0] += 1
            want_t.append(t)
            want_final.append(final)
            want_level.append(J)
            its[J] += int(c[C_K])
            if J == L - 1:
                conv = bool(c[C_CONVERGED])
        return its, conv

    t, kappa = t0, kappa0
    t_stop = t
    while t_stop <= 1 / tol:
        t_stop *= kappa0
    going = lambda tt: tt < t_stop
    its_cols, ts, kappas = [], [], []
    it0 = np.zeros(L, dtype=np.int64)
    ok = False
    for attempt in range(O.INITIAL_CENTERING_ATTEMPTS):
        it, ok = amgb_step(t, True)
        it0 += it
        if ok:
            break
    assert ok, "initial centering failed"
    its_cols.append(it0)
    ts.append(t)
    k = 1
    while going(t) and kappa > 1 and k < maxit:
        k += 1
        itk = np.zeros(L, dtype=np.int64)
        while kappa > 1:
            t1 = min(kappa * t, t_stop)
            it1, ok = amgb_step(t1, True)
            itk += it1
            if ok:
                if it1.max() <= max_newton * O.KAPPA_GROW_FRAC:
                    kappa = min(kappa0, kappa * kappa)
                t = t1
                break
            kappa = math.sqrt(kappa)
            if kappa < 1 + 1e-3:
                kappa = 1.0
        its_cols.append(itk)
        ts.append(t)
        kappas.append(kappa)
    assert pos[0] == len(cents), "the trace goes on after the solve has ended"
    return dict(t=np.array(want_t), final=np.array(want_final), level=np.array(want_level), its=np.array(its_cols).T,
                ts=np.array(ts), kappas=np.array(kappas), converged=not going(t))
