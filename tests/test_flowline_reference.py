"""The yardstick tests/flowline_reference.py against closed forms on exactly represented fields, and the second order of the
midpoint rule in ds.  No library call: the meshes are built here (the square [-1, 1]^2 cut into 2 4^(L-1) triangles with the
P2 + bubble block, the cube [-1, 1]^3 as one tensor element of degree k).

Tolerance of an exit point, a length or a time that the rule reproduces exactly: ds 2^-40 + 2e-12 -- the bisection, plus the
containment tolerance tau = 1e-12 times the element size (the mesh ends tau outside its last element) and the rounding of at
most max_steps additions of ds (256 2^-53 2 < 1e-13).

Measured (ds = 0.125, 0.0625, 0.03125 on L = 3, arc length 0.5): drift of x^2 - y^2 along u = x y, ratios 4.34 and 4.16; p = 2
time on the rays of u = x^2 + y^2, ratios 3.94 and 3.98."""
import numpy as np
import pytest

import flowline_reference as FR

LD = FR.LD


def square(L):
    """(n, 2) nodes of the square [-1, 1]^2: 2 4^(L-1) triangles, rows v1 v2 v3 m12 m23 m31 centroid"""
    T = [np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0]]), np.array([[-1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])]
    for _ in range(L - 1):
        nxt = []
        for t in T:
            m = [(t[0] + t[1]) / 2, (t[1] + t[2]) / 2, (t[2] + t[0]) / 2]
            nxt += [np.array([t[0], m[0], m[2]]), np.array([m[0], t[1], m[1]]), np.array([m[2], m[1], t[2]]), np.array([m[0], m[1], m[2]])]
        T = nxt
    rows = []
    for t in T:
        rows += [t[0], t[1], t[2], (t[0] + t[1]) / 2, (t[1] + t[2]) / 2, (t[2] + t[0]) / 2, (t[0] + t[1] + t[2]) / 3]
    return np.array(rows)


def cube(k):
    """((k+1)^3, 3) nodes of [-1, 1]^3 as one tensor element, x fastest"""
    t = -1.0 + 2.0 * np.arange(k + 1) / k
    return np.array([[t[i], t[j], t[m]] for m in range(k + 1) for j in range(k + 1) for i in range(k + 1)])


SEEDS = np.stack([-0.83 + 0.0917 * np.arange(8), 0.41 - 0.0531 * np.arange(8)], axis=1)
MESH = {}


def mesh2(L):
    if L not in MESH:
        MESH[L] = FR.Mesh(square(L), 7)
    return MESH[L]


def tol(ds, end=None):
    """ds 2^-40 + 2e-12; for a line that meets the boundary at an angle (the rays to `end`) the tau h <= 2e-12 by which the mesh
    overhangs is measured along the line: times |end|_2 / |end|_inf, the secant of that angle"""
    sec = 1.0 if end is None else float(np.sqrt((end ** 2).sum()) / np.abs(end).max())
    return ds * 2.0 ** -40 + 2e-12 * sec


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("p", [1.0, 1.5, 2.0, 3.0])
def test_u_equals_x(L, p):
    M = mesh2(L)
    x = M.X.reshape(-1, 2).astype(np.float64)
    F = FR.Field(M, x[:, 0])
    assert M.default_ds == 2.0 ** -L      # a quarter of the short side 2^(2-L)
    for s in SEEDS:
        R = FR.trace(M, F, s, p=p, direction=1, max_steps=256)
        t = tol(M.default_ds)
        assert R.status == FR.EXIT and R.undecided == 0
        assert abs(R.end[0] - 1) <= t and abs(R.end[1] - LD(s[1])) <= t
        assert abs(R.length - (1 - LD(s[0]))) <= t and abs(R.time - (1 - LD(s[0]))) <= t
        assert R.u_start == LD(s[0]) or abs(R.u_start - LD(s[0])) <= 1e-15
        assert abs(R.u_end - 1) <= t
        back = FR.trace(M, F, s, p=p, direction=-1, max_steps=256)
        assert back.status == FR.EXIT and abs(back.end[0] + 1) <= t and abs(back.length - (1 + LD(s[0]))) <= t


def ray_exit(s):
    """where the ray from the origin through s leaves [-1, 1]^d"""
    s = np.asarray(s, dtype=LD)
    return s / np.abs(s).max()


@pytest.mark.parametrize("L", [2, 3])
def test_paraboloid_rays(L):
    M = mesh2(L)
    x = M.X.reshape(-1, 2).astype(np.float64)
    F = FR.Field(M, (x * x).sum(axis=1))
    ds = M.default_ds
    for s in SEEDS:
        r0 = np.sqrt((s.astype(LD) ** 2).sum())
        end = ray_exit(s)
        for p in (1.0, 2.0):
            R = FR.trace(M, F, s, p=p, direction=1, max_steps=256)
            assert R.status == FR.EXIT
            assert np.abs(R.end - end).max() <= tol(ds, end)
            assert abs(R.length - (np.sqrt((end ** 2).sum()) - r0)) <= tol(ds, end)
            if p == 1.0:
                assert abs(R.time - R.length) <= tol(ds, end)
            else:      # the midpoint rule of int dr / (2 r): second order, checked below; here only that it is close
                assert abs(R.time - np.log(np.sqrt((end ** 2).sum()) / r0) / 2) <= ds * ds / r0 ** 2
        R = FR.trace(M, F, s, p=2.0, direction=-1, max_steps=256, gmin=2 * ds)
        # |grad u| = 2 r <= gmin = 2 ds holds where the stall is SEEN: at x_k, or by step 5 of the rule at the midpoint ds / 2
        # ahead of it, in which case the line ends at x_k: the end point is within ds + ds / 2 of the origin
        assert R.status == FR.STALLED and np.sqrt((R.end ** 2).sum()) <= 1.5 * ds + 1e-15
        assert np.abs(R.end * r0 - s.astype(LD) * np.sqrt((R.end ** 2).sum())).max() <= 1e-15      # still on the ray


@pytest.mark.parametrize("k", [1, 2, 3])
def test_cube(k):
    M = FR.Mesh(cube(k), (k + 1) ** 3)
    x = cube(k)
    seeds = np.stack([-0.83 + 0.1917 * np.arange(5), 0.41 - 0.1531 * np.arange(5), 0.29 - 0.2713 * np.arange(5)], axis=1)
    assert M.default_ds == 0.5
    F = FR.Field(M, x[:, 0])
    for s in seeds:
        R = FR.trace(M, F, s, p=1.5)
        assert R.status == FR.EXIT and abs(R.end[0] - 1) <= tol(0.5) and np.abs(R.end[1:] - s[1:].astype(LD)).max() <= tol(0.5)
        assert abs(R.length - (1 - LD(s[0]))) <= tol(0.5) and abs(R.time - R.length) <= tol(0.5)
    F = FR.Field(M, (x * x).sum(axis=1))
    for s in seeds:
        R = FR.trace(M, F, s, p=1.0, ds=0.125)
        if k == 1:      # the trilinear interpolant of |x|^2 is the constant 3
            assert R.status == FR.STALLED and R.count == 1 and R.length == 0 and abs(R.u_start - 3) <= 1e-15
            continue
        end = ray_exit(s)
        r0 = np.sqrt((s.astype(LD) ** 2).sum())
        assert R.status == FR.EXIT and np.abs(R.end - end).max() <= tol(0.125, end)
        assert abs(R.length - (np.sqrt((end ** 2).sum()) - r0)) <= tol(0.125, end) and abs(R.time - R.length) <= tol(0.125, end)


def test_second_order_in_ds():
    """At a fixed arc length 0.5 (4, 8, 16 steps of ds, ds / 2, ds / 4; MAXSTEPS, no exit) on L = 3: the drift of x^2 - y^2
    along the hyperbolas of u = x y, and the error of the p = 2 time on the rays of u = x^2 + y^2.  The midpoint rule predicts
    ratios of 4; both quantities, both halvings: inside [3, 5]."""
    M = mesh2(3)
    x = M.X.reshape(-1, 2).astype(np.float64)
    seeds = np.array([[0.31 + 0.0417 * i, 0.23 - 0.0331 * i] for i in range(4)])      # away from the origin, 0.5 from the boundary
    Fxy, Fr = FR.Field(M, x[:, 0] * x[:, 1]), FR.Field(M, (x * x).sum(axis=1))
    drift, terr = [], []
    for j in range(3):
        ds, n = 0.125 / 2 ** j, 4 * 2 ** j
        d = t = LD(0)
        for s in seeds:
            R = FR.trace(M, Fxy, s, p=2.0, ds=ds, max_steps=n)
            assert R.status == FR.MAXSTEPS and R.count == n + 1 and abs(R.length - 0.5) <= 1e-15
            c = LD(s[0]) ** 2 - LD(s[1]) ** 2
            d = max(d, abs(R.end[0] ** 2 - R.end[1] ** 2 - c))
            R = FR.trace(M, Fr, s, p=2.0, ds=ds, max_steps=n)
            r0 = np.sqrt((s.astype(LD) ** 2).sum())
            assert R.status == FR.MAXSTEPS
            t = max(t, abs(R.time - np.log((r0 + LD(0.5)) / r0) / 2))
        drift.append(d), terr.append(t)
    ratios = [float(drift[0] / drift[1]), float(drift[1] / drift[2]), float(terr[0] / terr[1]), float(terr[1] / terr[2])]
    print("drift of x^2 - y^2: %.3e %.3e %.3e; time error: %.3e %.3e %.3e; ratios %s"
          % (*map(float, drift), *map(float, terr), ["%.3f" % r for r in ratios]))
    assert all(3.0 <= r <= 5.0 for r in ratios), ratios
