"""What test_timestat_host.py and test_gpu_time_stats.py share: host geometries, the call of mgb_geo_time_stats_host and the
comparison of a library result with the exact yardstick tests/timestat_reference.py under the bars below.  Not a test.

Bars, eps = 2^-52, each from counting the roundings of the rule (B snapshots):
  max, min, tmax, tmin, entries, reached   equal
  change      eps |value|                            one subtraction
  integral    (B + 2) eps sum |terms|                 three roundings per term, B - 2 additions
  variation   (B + 1) eps sum |terms|
  rate        4 eps |value|
  arrival     8 eps (|ts[m]| + h_m) of its interval   (equal where the arrival is ts[0] itself)
  left        8 eps (|ts[m+1]| + h_m)
  exposure    (B + 6) eps (ts[B-1] - ts[0])
  excess      (B + 8) eps sum_m h_m (|v_m| + |v_{m+1}| + |c|) over the intervals that contribute
  totals      the bars of their terms weighted by w, plus 8 eps sum |terms|
  maxima of the totals: [3], [4] of row 0 equal; of row 1 + l the largest arrival bar among the reached nodes and the exposure
  bar -- the maximum of values that lie within their bars lies within the largest of them."""
import ctypes as C
from fractions import Fraction as F

import numpy as np

import levelset_util as LU
import timestat_reference as TR

MGB_E_ARG = -1
FEPS = F(TR.EPS)
QUANTITIES = ("change", "integral", "variation", "rate", "arrival", "left", "exposure", "excess", "totals")


def host_mesh(kind, L):
    """fem1d / fem2d level L, or fem3d level L of degree 1: handle, n, x, w"""
    if kind == "fem3d":
        import isosurface_util as IU
        return IU.host_mesh(L, 1)
    return LU.host_mesh(kind, L)


class Result:
    """node (n, 8), level (nl, n, 5), rows (1 + nl, 5) of a library call"""

    def __init__(self, node, level, rows):
        self.node, self.level, self.rows = node, level, rows


def host_time_stats(lib, g, fields, ts, levels=None, never=float("nan"), u=0, rc_only=False, **over):
    """mgb_geo_time_stats_host on a host mesh: `fields` a list of (n,) or (n, S) arrays.  Outputs are prefilled so that an
    unwritten word shows.  `over` replaces arguments of the C call by name (geo, B, table, times, S, u, nl, levels, never, node, level, out)."""
    from mgb_amd import _lib
    fields = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    S, B = fields[0].shape[1], len(fields)
    lv = None if levels is None else _lib.f64(np.atleast_1d(levels))
    nl = 0 if lv is None else lv.size
    tsa = _lib.f64(np.asarray(ts, dtype=np.float64))
    table = (_lib.c_dbl_p * max(B, 1))(*[_lib.dptr(z) for z in fields])
    node, level, rows = np.full((g.n, 8), 7.0), np.full((max(nl, 1), g.n, 5), 7.0), np.full((1 + max(over.get("nl", nl), 0), 5), 7.0)
    a = dict(geo=g.handle, B=B, table=table, times=_lib.dptr(tsa), S=S, u=u, nl=nl, levels=None if lv is None else _lib.dptr(lv),
             never=never, node=_lib.dptr(node), level=_lib.dptr(level) if nl else None, out=_lib.dptr(rows))
    a.update(over)
    rc = lib.mgb_geo_time_stats_host(a["geo"], a["B"], a["table"], a["times"], a["S"], a["u"], a["nl"], a["levels"], a["never"], a["node"],
                                     a["level"], a["out"])
    if rc_only:
        if rc != 0:      # MGB_E_ARG comes before anything is written
            assert (node == 7.0).all() and (level == 7.0).all() and (rows == 7.0).all()
        return rc
    assert rc == 0, lib.mgb_last_error()
    return Result(node, level[:nl], rows)


def _same_never(got, never):
    return np.isnan(got) if np.isnan(never) else got == never


def _ratio(worst, key, got, ref, bar, who):
    """|got - ref| against the bar, exactly; a zero bar asks for equality"""
    assert np.isfinite(got), (who, key, got)
    gap = abs(F(float(got)) - ref)
    if bar == 0:
        assert gap == 0, (who, key, got, float(ref))
        return
    r = float(gap / bar)
    worst[key] = max(worst[key], r)
    assert r <= 1.0, (who, key, got, float(ref), r)


def against_reference(name, got, R, never, worst=None):
    """A library Result against the yardstick R (timestat_reference.Reference) under the bars of this module's docstring.
    Prints the largest ratio to each bar, then returns them; every comparison is asserted on the way."""
    worst = {k: 0.0 for k in QUANTITIES} if worst is None else worst
    B, n, nl = R.B, R.n, R.nl
    assert got.node.shape == (n, 8) and got.level.shape == (nl, n, 5) and got.rows.shape == (1 + nl, 5)
    fw = [F(float(x)) for x in R.w]
    bars0 = [F(0)] * 3
    for i, q in enumerate(R.node):
        row, who = got.node[i], "%s node %d" % (name, i)
        if q.bad:
            assert np.isnan(row).all(), who
            continue
        assert F(float(row[1])) == q.max and F(float(row[2])) == q.tmax and F(float(row[3])) == q.min and F(float(row[4])) == q.tmin, who
        bars = ((B + 2) * FEPS * q.abs_integral, (B + 1) * FEPS * q.abs_variation, FEPS * abs(q.change))
        _ratio(worst, "integral", row[0], q.integral, bars[0], who)
        _ratio(worst, "variation", row[5], q.variation, bars[1], who)
        _ratio(worst, "rate", row[6], q.rate, 4 * FEPS * abs(q.rate), who)
        _ratio(worst, "change", row[7], q.change, bars[2], who)
        bars0 = [b + fw[i] * x for b, x in zip(bars0, bars)]
    ebar = (B + 6) * FEPS * R.span
    lbars, abars = [], []
    for l in range(nl):
        bl, amax = [F(0)] * 3, F(0)
        for i, q in enumerate(R.level[l]):
            row, who = got.level[l, i], "%s level %d node %d" % (name, l, i)
            if q.bad:
                assert np.isnan(row).all(), who
                continue
            assert q.t_range, who
            assert row[4] == q.entries, (who, row[4], q.entries)
            for k, key, ref, scale in ((0, "arrival", q.arrival, q.arrival_scale), (1, "left", q.left, q.left_scale)):
                if ref is None:
                    assert _same_never(row[k], never), (who, key, row[k])
                else:
                    _ratio(worst, key, row[k], ref, 8 * FEPS * scale, who)
            if q.entries > 0:
                amax = max(amax, 8 * FEPS * q.arrival_scale)
            xbar = (B + 8) * FEPS * q.abs_excess
            _ratio(worst, "exposure", row[2], q.exposure, ebar if q.exposure != 0 else F(0), who)
            _ratio(worst, "excess", row[3], q.excess, xbar, who)
            bl = [bl[0], bl[1] + fw[i] * (ebar if q.exposure != 0 else 0), bl[2] + fw[i] * xbar]
        lbars.append(bl)
        abars.append(amax)
    for r in range(1 + nl):
        row, who = got.rows[r], "%s row %d" % (name, r)
        if R.rows[r] is None:
            assert np.isnan(row).all(), who
            continue
        for k in range(3):
            bar = (bars0 if r == 0 else lbars[r - 1])[k] + 8 * FEPS * R.abs_rows[r][k]
            _ratio(worst, "totals", row[k], R.rows[r][k], bar, who)
        if r == 0:
            assert F(float(row[3])) == R.rows[0][3] and F(float(row[4])) == R.rows[0][4], who
        else:
            if R.rows[r][3] is None:
                assert row[3] == -np.inf, (who, row[3])
            else:
                _ratio(worst, "arrival", row[3], R.rows[r][3], abars[r - 1], who)
            _ratio(worst, "exposure", row[4], R.rows[r][4], ebar if R.rows[r][4] != 0 else F(0), who)
    print("%s: largest ratio to the bar: %s" % (name, ", ".join("%s %.3f" % (k, worst[k]) for k in QUANTITIES)))
    return worst


def front(x, ts, width=0.2):
    """the moving front tanh((t - |x|) / width) at the nodes x for the times ts: (B, n)"""
    r = np.sqrt((np.asarray(x).reshape(len(x), -1) ** 2).sum(axis=1))
    return np.tanh((np.asarray(ts)[:, None] - r[None, :]) / width)
