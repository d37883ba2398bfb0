"""The yardstick tests/pathline_reference.py against closed forms, and the second order of the midpoint rule in dt.  No library
call: the meshes are those of test_flowline_reference.py (the square [-1, 1]^2 in P2 + bubble triangles, the cube as one tensor
element).

Tolerances.  A path that the rule integrates exactly (a velocity linear in t) is held to 1e-13: the nodal values are doubles,
so every snapshot's gradient is off by at most sum_j |grad N_j| eps / 2 max|z| <= 15 eps max|z| / h (the P2 + bubble basis
gradients sum to less than 30 / h), here h = 1/2, max|z| <= 4, T = 1: 120 eps = 2.7e-14; the longdouble sums add nothing
visible.  An exit time: span 2^-40 for the bisection plus the containment tolerance tau h / |w| <= 2e-12 / |w|.

Measured (substeps 2, 4, 8; ratios of consecutive errors): u = c(t) |x|^2 / 2, p = 2: 4.37 and 4.17; p = 1.5 on u = x_0^2 / 2:
4.22 and 4.11 (the triangles and the tensor element alike)."""
import numpy as np
import pytest

import flowline_reference as FR
import pathline_reference as PR
from test_flowline_reference import cube, mesh2

LD = FR.LD
TS = np.array([0.0, 0.25, 0.5, 1.0])
C = np.array([1.0, 0.5, -0.75, 0.25])      # c(t_j), d(t_j): dyadic, piecewise linear in between
D = np.array([-0.5, 0.25, 0.5, 1.0])
SEEDS = np.stack([-0.33 + 0.0917 * np.arange(6), 0.21 - 0.0531 * np.arange(6)], axis=1)


def integral(v, a, b):
    """int_{TS[a]}^{TS[b]} of the piecewise-linear function with values v at TS"""
    return sum((LD(v[j]) + LD(v[j + 1])) / 2 * (LD(TS[j + 1]) - LD(TS[j])) for j in range(a, b))


def linear_fields(M):
    x = M.X.reshape(-1, 2).astype(np.float64)
    return [FR.Field(M, C[j] * x[:, 0] + D[j] * x[:, 1]) for j in range(len(TS))]


@pytest.mark.parametrize("substeps", [1, 3])
def test_velocity_linear_in_time_is_integrated_exactly(substeps):
    M = mesh2(3)
    F = linear_fields(M)
    for rel, stop in ((0, 3), (1, 2), (2, 3)):
        for s in SEEDS:
            R = PR.trace(M, F, TS, s, rel, stop, substeps, p=2.0, direction=-1)
            assert R.status == PR.DONE and R.count == (stop - rel) * substeps + 1 and R.rested == 0
            want = np.array([LD(s[0]) - integral(C, rel, stop), LD(s[1]) - integral(D, rel, stop)])
            assert np.abs(R.end - want).max() <= 1e-13, (rel, stop, s)
            assert R.time == LD(TS[stop])
            assert abs(R.u_start - (C[rel] * LD(s[0]) + D[rel] * LD(s[1]))) <= 1e-13
            assert abs(R.u_end - (C[stop] * want[0] + D[stop] * want[1])) <= 1e-13


def test_unit_speed_for_p_1():
    M = mesh2(3)
    F = linear_fields(M)
    for speed in (1.0, 0.5):
        for s in SEEDS:
            R = PR.trace(M, F, TS, s, 0, 3, 4, p=1.0, direction=-1, speed=speed)
            assert R.status == PR.DONE
            assert abs(R.length - speed * (LD(TS[3]) - LD(TS[0]))) <= 1e-13
            assert abs(R.max_step - speed * LD(0.125)) <= 1e-13      # the longest step: the last slab, (1 - 0.5) / 4


def ratios(errs):
    errs = [float(e) for e in errs]
    r = [errs[k] / errs[k + 1] for k in range(len(errs) - 1)]
    print("errors", errs, "ratios", r)
    return r


def test_second_order_contraction():
    """u = c(t) |x|^2 / 2, exactly a P2 field at every node time, p = 2, down the gradient: x(t) = x_0 exp(-int c)"""
    M = mesh2(3)
    x = M.X.reshape(-1, 2).astype(np.float64)
    c = np.array([0.5, 0.75, 0.25, 0.625])      # c dt <= 0.1 from substeps = 2 on: the next order moves a ratio by about c dt
    F = [FR.Field(M, c[j] * (x ** 2).sum(axis=1) / 2) for j in range(4)]
    s = np.array([0.83, -0.61])
    want = s.astype(LD) * np.exp(-integral(c, 0, 3))
    errs = []
    for n in (2, 4, 8):
        R = PR.trace(M, F, TS, s, 0, 3, n, p=2.0, direction=-1)
        assert R.status == PR.DONE
        errs.append(np.abs(R.end - want).max())
    assert all(3.0 <= r <= 5.0 for r in ratios(errs))


def test_second_order_p_1_5():
    """u = x_0^2 / 2, the same in every snapshot, p = 1.5: dx_0/dt = -sqrt(x_0), sqrt(x_0) falls linearly; on one tensor element
    of degree 2 as well"""
    x = cube(2)
    cases = [(mesh2(3), mesh2(3).X.reshape(-1, 2).astype(np.float64), np.array([0.83, -0.61])),
             (FR.Mesh(x, 27), x, np.array([0.83, -0.61, 0.27]))]
    for M, xx, s in cases:
        F = [FR.Field(M, xx[:, 0] ** 2 / 2)] * 4
        want = (np.sqrt(LD(s[0])) - (LD(TS[3]) - LD(TS[0])) / 2) ** 2
        errs = []
        for n in (2, 4, 8):
            R = PR.trace(M, F, TS, s, 0, 3, n, p=1.5, direction=-1)
            assert R.status == PR.DONE and np.abs(R.end[1:] - s[1:].astype(LD)).max() <= 1e-13
            errs.append(abs(R.end[0] - want))
        assert all(3.0 <= r <= 5.0 for r in ratios(errs))


def test_rest_and_resume():
    """no gradient in the first slab, u = x_0 growing in the second: the particle rests n steps, is recorded all the same, and
    goes on; the first step of the second slab has w(g) = 0 at its start and moves by its midpoint velocity"""
    M = mesh2(2)
    x = M.X.reshape(-1, 2).astype(np.float64)
    F = [FR.Field(M, np.zeros(len(x))), FR.Field(M, np.zeros(len(x))), FR.Field(M, x[:, 0])]
    ts, n, s = np.array([0.0, 0.5, 1.0]), 4, np.array([0.31, 0.17])
    R = PR.trace(M, F, ts, s, 0, 2, n, p=2.0, direction=-1)
    assert R.status == PR.DONE and R.rested == n and R.count == 2 * n + 1
    assert (R.pts[: n + 1] == s.astype(LD)).all()      # resting: x + dt 0 and (np.diff(R.pts[n:, 0].astype(np.float64)) < 0).all()
    # velocity -th in the second slab, th = (t - 1/2) / (1/2): x_0 falls by int_0^1 th dth / 2 = 1/4, exactly (linear in t)
    assert abs(R.end[0] - (LD(s[0]) - LD(0.25))) <= 1e-13 and abs(R.end[1] - LD(s[1])) <= 1e-13
    assert abs(R.length - LD(0.25)) <= 1e-13


def test_exit_time():
    """u = c x_0, p = 2, down the gradient: the particle leaves through x_0 = -1 at t = (1 + s_0) / c"""
    M = mesh2(3)
    x = M.X.reshape(-1, 2).astype(np.float64)
    c = 2.5
    F = [FR.Field(M, c * x[:, 0])] * 4
    for n in (1, 4):
        for s in SEEDS:
            R = PR.trace(M, F, TS, s, 0, 3, n, p=2.0, direction=-1)
            want = (1 + LD(s[0])) / c
            j = int(np.searchsorted(TS, float(want))) - 1      # the slab of the exit
            span = (TS[j + 1] - TS[j]) / n
            assert R.status == PR.EXIT and R.undecided == 0
            assert abs(R.time - want) <= span * 2.0 ** -40 + 2e-12 / c, (n, s)
            assert abs(R.end[0] + 1) <= span * c * 2.0 ** -40 + 2e-12 and abs(R.end[1] - LD(s[1])) <= 1e-13
            assert abs(R.length - (1 + LD(s[0]))) <= span * c * 2.0 ** -40 + 2e-12
            assert abs(R.u_end + c) <= 1e-11


def test_streakline_through_the_python_result():
    """Seeds released one snapshot after another from one point in the linear field: PathLines.positions(stop) is the streakline
    x - int_{t_rel}^{t_stop} (c, d), positions(j) is NaN for the particles not yet released, and times() are the step times.  The
    PathLines object is filled from the yardstick's trajectories: no library call."""
    import mgb_amd as MG
    M = mesh2(3)
    F = linear_fields(M)
    s, stop, n = np.array([-0.21, 0.33]), 3, 2
    R = [PR.trace(M, F, TS, s, rel, stop, n, p=2.0, direction=-1) for rel in range(stop)]
    rows = np.array([[r.length, r.time, r.u_start, r.u_end, r.max_step] for r in R], dtype=np.float64)
    i32 = lambda v: np.array(v, dtype=np.int32)
    count = i32([r.count for r in R])
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    pl = MG.PathLines(rows, np.array([r.end for r in R], dtype=np.float64), i32([r.status for r in R]), count,
                      i32([r.end_element for r in R]), i32([r.rested for r in R]), TS.copy(), i32(range(stop)), stop, n, offsets,
                      np.concatenate([r.pts for r in R]).astype(np.float64), np.concatenate([r.elems for r in R]).astype(np.int32))
    assert (pl.status == pl.DONE).all()
    streak = pl.positions(stop)
    for rel in range(stop):
        want = np.array([LD(s[0]) - integral(C, rel, stop), LD(s[1]) - integral(D, rel, stop)])
        assert np.abs(streak[rel] - want.astype(np.float64)).max() <= 1e-13
        assert pl.times(rel)[0] == TS[rel] and pl.times(rel)[-1] == TS[stop] and len(pl.times(rel)) == count[rel]
        assert pl.times(rel)[1] == TS[rel] + (TS[rel + 1] - TS[rel]) / n
    at1 = pl.positions(1)
    assert np.array_equal(at1[0], pl.path(0)[n]) and np.array_equal(at1[1], s) and np.isnan(at1[2]).all()
    assert np.array_equal(pl.positions(0)[0], s) and np.isnan(pl.positions(0)[1:]).all()
    with pytest.raises(IndexError):
        pl.positions(4)
    bare = MG.PathLines(rows, pl.end, pl.status, count, pl.end_element, pl.rested, TS.copy(), pl.release, stop, n)
    for call in (lambda: bare.path(0), lambda: bare.elements(0), lambda: bare.times(0), lambda: bare.positions(1)):
        with pytest.raises(ValueError, match="paths=False"):
            call()
