"""The yardstick of the time statistics (include/mgb_hip.h, mgb_geo_time_stats): the rule stated in exact rational arithmetic,
independent of the C++.  Every input double -- the values, the times, the levels, the weights and the steps h_m, which are
taken as the doubles ts[m+1] - ts[m] that the library is handed -- becomes a fractions.Fraction; every discrete decision
(above / not above, the first maximum, the first minimum) is the same comparison of the input doubles, so it is exact on both
sides.  Next to each value stands the sum of absolute terms that its bar needs.  Not a test."""
from fractions import Fraction as F

import numpy as np

EPS = 2.0 ** -52
NODE_NAMES = ("integral", "max", "tmax", "min", "tmin", "variation", "rate", "change")
LEVEL_NAMES = ("arrival", "left", "exposure", "excess", "entries")


def steps(ts):
    """h_m = ts[m+1] - ts[m] as the doubles both sides of the library are handed"""
    ts = np.asarray(ts, dtype=np.float64)
    return ts[1:] - ts[:-1]


class NodeRef:
    """The eight node columns of one node, exact, `abs_integral` = sum |0.5 h_m (v_m + v_{m+1})| and `abs_variation` (the
    variation itself).  `bad`: a non-finite value in the window -- every column is NaN then."""

    def __init__(self, v, ts, h):
        self.bad = not np.all(np.isfinite(v))
        if self.bad:
            return
        B = len(v)
        fv, ft, fh = [F(float(x)) for x in v], [F(float(x)) for x in ts], [F(float(x)) for x in h]
        terms = [F(1, 2) * fh[m] * (fv[m] + fv[m + 1]) for m in range(B - 1)]
        jumps = [abs(fv[m + 1] - fv[m]) for m in range(B - 1)]
        imax = imin = 0
        for m in range(1, B):
            if v[m] > v[imax]:
                imax = m
            if v[m] < v[imin]:
                imin = m
        self.integral, self.abs_integral = sum(terms, F(0)), sum((abs(t) for t in terms), F(0))
        self.max, self.tmax, self.min, self.tmin = fv[imax], ft[imax], fv[imin], ft[imin]
        self.variation = self.abs_variation = sum(jumps, F(0))
        self.rate = max(j / hm for j, hm in zip(jumps, fh))
        self.change = fv[-1] - fv[0]

    def columns(self):
        return [getattr(self, k) for k in NODE_NAMES]


class LevelRef:
    """The five level columns of one node and one level, exact; arrival / left are None where there is no event.
    `arrival_scale` = |ts[m]| + h_m of the arrival's interval (0 where the arrival is ts[0] itself), `left_scale` =
    |ts[m+1]| + h_m, `abs_excess` = sum h_m (|v_m| + |v_{m+1}| + |c|) over the intervals that contribute; `t_range` is True
    while every crossing parameter lies in [0, 1]."""

    def __init__(self, v, ts, h, c):
        self.bad = not np.all(np.isfinite(v))
        if self.bad:
            return
        B = len(v)
        fv, ft, fh, fc = [F(float(x)) for x in v], [F(float(x)) for x in ts], [F(float(x)) for x in h], F(float(c))
        self.arrival = self.left = None
        self.arrival_scale = self.left_scale = F(0)
        self.exposure = self.excess = self.abs_excess = F(0)
        self.entries, self.t_range = 0, True
        if v[0] > c:
            self.entries, self.arrival = 1, ft[0]
        for m in range(B - 1):
            ua, ub = bool(v[m] > c), bool(v[m + 1] > c)
            if not ua and not ub:
                continue
            self.abs_excess += fh[m] * (abs(fv[m]) + abs(fv[m + 1]) + abs(fc))
            if ua and ub:
                self.exposure += fh[m]
                self.excess += fh[m] * ((fv[m] + fv[m + 1]) / 2 - fc)
                continue
            lo, hi = (fv[m + 1], fv[m]) if ua else (fv[m], fv[m + 1])
            t = (fc - lo) / (hi - lo)
            self.t_range = self.t_range and 0 <= t <= 1
            e = (1 - t) * fh[m]
            self.exposure += e
            self.excess += e * ((hi - fc) / 2)
            if ub:
                self.entries += 1
                if self.arrival is None:
                    self.arrival, self.arrival_scale = ft[m] + t * fh[m], abs(ft[m]) + fh[m]
            else:
                self.left, self.left_scale = ft[m + 1] - t * fh[m], abs(ft[m + 1]) + fh[m]


class Reference:
    """The whole call: `node[i]` a NodeRef, `level[l][i]` a LevelRef, `rows[r]` the exact totals (None where a term is NaN: the
    sums and maxima of that row are NaN then) and `abs_rows[r]` the sums of |w term| of the three sums.  Z: (B, n) values of
    the column, ts: (B,), levels: (nl,), w: (n,)."""

    def __init__(self, Z, ts, levels, w):
        Z, ts, w = np.asarray(Z, dtype=np.float64), np.asarray(ts, dtype=np.float64), np.asarray(w, dtype=np.float64)
        levels = np.zeros(0) if levels is None else np.atleast_1d(np.asarray(levels, dtype=np.float64))
        self.B, self.n, self.nl = Z.shape[0], Z.shape[1], len(levels)
        self.ts, self.h, self.levels, self.w = ts, steps(ts), levels, w
        self.span = F(float(ts[-1])) - F(float(ts[0]))
        self.node = [NodeRef(Z[:, i], ts, self.h) for i in range(self.n)]
        self.level = [[LevelRef(Z[:, i], ts, self.h, c) for i in range(self.n)] for c in levels]
        fw = [F(float(x)) for x in w]
        self.bad = any(nd.bad for nd in self.node)
        self.rows, self.abs_rows = [], []
        if self.bad:
            self.rows, self.abs_rows = [None] * (1 + self.nl), [None] * (1 + self.nl)
            return
        nd = self.node
        sums = [[fw[i] * x for i, x in enumerate(col)] for col in ([q.integral for q in nd], [q.variation for q in nd], [q.change for q in nd])]
        self.rows.append([sum(s, F(0)) for s in sums] + [max(q.max for q in nd), max(-q.min for q in nd)])
        self.abs_rows.append([sum((abs(x) for x in s), F(0)) for s in sums])
        for lv in self.level:
            sums = [[fw[i] * x for i, x in enumerate(col)] for col in ([F(int(q.entries > 0)) for q in lv], [q.exposure for q in lv], [q.excess for q in lv])]
            reached = [q.arrival for q in lv if q.entries > 0]
            self.rows.append([sum(s, F(0)) for s in sums] + [max(reached) if reached else None, max(q.exposure for q in lv)])
            self.abs_rows.append([sum((abs(x) for x in s), F(0)) for s in sums])
