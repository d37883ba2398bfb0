"""The yardstick tests/timestat_reference.py against closed forms, with values that are exact in binary so that the rational
arithmetic must hit the closed form exactly: a straight line v(t) = a + b t on a uniform grid, and a hat up and down."""
from fractions import Fraction as F

import numpy as np

import timestat_reference as TR


def test_a_straight_line_on_a_uniform_grid():
    a, b, c = F(-1, 2), F(1, 4), F(3, 16)               # v = -1/2 + t/4 crosses c = 3/16 at t = 11/4, between snapshots
    ts = np.arange(0.0, 4.5, 0.5)
    v = np.array([float(a + b * F(float(t))) for t in ts])
    T = F(float(ts[-1]))
    q = TR.NodeRef(v, ts, TR.steps(ts))
    assert not q.bad
    assert q.integral == a * T + b * T * T / 2          # the trapezoid rule is exact on a line
    assert (q.max, q.tmax, q.min, q.tmin) == (a + b * T, T, a, 0)
    assert q.variation == b * T and q.rate == b and q.change == b * T
    assert q.abs_integral >= abs(q.integral) and q.abs_variation == q.variation
    lv = TR.LevelRef(v, ts, TR.steps(ts), float(c))
    t_c = (c - a) / b
    assert lv.arrival == t_c == F(11, 4) and lv.left is None and lv.entries == 1 and lv.t_range
    assert lv.exposure == T - t_c
    assert lv.excess == b * (T - t_c) ** 2 / 2          # the triangle under the line above c
    assert lv.arrival_scale == F(5, 2) + F(1, 2)        # |ts[m]| + h_m of the interval [5/2, 3]
    falling = TR.LevelRef(v[::-1].copy(), ts, TR.steps(ts), float(c))
    assert falling.arrival == 0 and falling.entries == 1 and falling.left == T - t_c and falling.exposure == T - t_c
    assert falling.excess == lv.excess and falling.left_scale == F(3, 2) + F(1, 2)      # |ts[m+1]| + h_m of [1, 3/2]


def test_a_hat_up_and_down():
    ts = np.array([-1.0, 0.0, 0.5, 2.5])                 # non-uniform, one negative
    v = np.array([0.0, 0.0, 1.0, 0.0])
    q = TR.NodeRef(v, ts, TR.steps(ts))
    assert q.integral == F(1, 4) + 1 and (q.max, q.tmax, q.min, q.tmin) == (1, F(1, 2), 0, -1)
    assert q.variation == 2 and q.rate == 2 and q.change == 0
    lv = TR.LevelRef(v, ts, TR.steps(ts), 0.25)
    assert lv.entries == 1 and lv.arrival == F(1, 8) and lv.left == F(2) and lv.exposure == F(2) - F(1, 8)
    assert lv.excess == F(3, 4) * lv.exposure / 2
    on = TR.LevelRef(v, ts, TR.steps(ts), 0.0)           # the plateau on the level is not above
    assert on.entries == 1 and on.arrival == 0 and on.left == F(5, 2) and on.exposure == F(5, 2)
    top = TR.LevelRef(v, ts, TR.steps(ts), 1.0)          # the peak on the level is not above
    assert top.entries == 0 and top.arrival is None and top.left is None and top.exposure == 0 and top.excess == 0
    twice = TR.LevelRef(np.array([0.0, 1.0, 0.0, 1.0, 0.0]), np.arange(5.0), np.ones(4), 0.5)
    assert twice.entries == 2 and twice.arrival == F(1, 2) and twice.left == F(7, 2) and twice.exposure == 2


def test_totals_and_non_finite_values():
    ts = np.array([0.0, 1.0, 2.0])
    Z = np.array([[0.0, 1.0, 2.0], [1.0, 1.0, 0.0], [2.0, 1.0, 4.0]])
    w = np.array([0.5, 0.25, 0.25])
    R = TR.Reference(Z, ts, [0.5, 9.0], w)
    assert R.rows[0][:3] == [F(1, 2) * 2 + F(1, 4) * 2 + F(1, 4) * 3, F(1, 2) * 2 + 0 + F(1, 4) * 6, F(1, 2) * 2 + 0 + F(1, 4) * 2]
    assert R.rows[0][3:] == [4, 0]
    assert R.rows[1][0] == 1 and R.rows[1][3] == F(1, 2) and R.rows[1][4] == 2      # every node reached; node 0 arrives last
    assert R.rows[2] == [0, 0, 0, None, 0]
    Z[1, 2] = np.nan
    bad = TR.Reference(Z, ts, [0.5], w)
    assert bad.node[2].bad and not bad.node[0].bad and bad.level[0][2].bad and bad.rows == [None, None]
