"""CPU tests of the yardstick tests/ray_reference.py itself (the np.longdouble brute force over all elements that the host
restatement and the gfx950 kernels are held to) against closed forms on [-1, 1]^dim and on the L shape.  Every comparison is
within the yardstick's own sum bar plus overlap x max|integrand|: the documented tau / |beta| overlap of neighbouring pieces
is part of the rule, not an error of the yardstick.

Measured: no ray of any case here is undecided (0 of 72 on each mesh, the 12 named degenerate rays included).  The excess of a
computed length over the exact chord is systematic -- every interior piece end really reaches tau / |beta| into its neighbour --
so the largest ratio of a gap to bar + overlap x max|integrand| is close to 1 by nature: 0.999 (length), 0.963 (paraboloid),
0.975 (oblique chords), 0.373 (gates).  The bound is met with nothing to spare and nothing added.  Because the excess has a
known sign and size, the length is also held to the sharper statement excess = overlap within the ROUNDING bar alone, at the
usual 0.5: measured ratio 0.001 on both meshes (a factor 2 in `overlap` would give ratios of about 100)."""
import numpy as np
import pytest

import mesh_cases as MC      # noqa: F401  (the L shape comes through ray_util)
import ray_reference as RR
import ray_util as RU

LD = RR.LD


def chord(a, b):
    """(t_in, t_out) of the segment in the closed box [-1, 1]^dim, longdouble; t_in > t_out: no chord."""
    a, d = a.astype(LD), b.astype(LD) - a.astype(LD)
    t0, t1 = LD(0), LD(1)
    for k in range(len(a)):
        if d[k] == 0:
            if abs(a[k]) > 1:
                return LD(1), LD(0)
            continue
        q0, q1 = sorted(((-1 - a[k]) / d[k], (1 - a[k]) / d[k]))
        t0, t1 = max(t0, q0), min(t1, q1)
    return t0, t1


def check(name, gaps):
    worst = max(gaps) if gaps else 0.0
    print("%s: largest ratio to bar + overlap x max|integrand|: %.3f" % (name, worst))
    assert worst <= 1.0, (name, worst)


CASES = [("fem2d", 4, 0), ("fem3d", 3, 2)]


@pytest.mark.parametrize("kind,L,k", CASES)
def test_length_is_the_clipped_chord(lib, kind, L, k):
    g = RU.host_mesh(kind, L, k)
    a, b = RU.rays(g.dim, 72)
    ref = RU.reference(g, np.zeros(g.n), a, b)
    assert not any(R.undecided for R in ref)
    gaps, sharp = [], []
    for i, R in enumerate(ref):
        t0, t1 = chord(a[i], b[i])
        ell = np.sqrt(((b[i].astype(LD) - a[i].astype(LD)) ** 2).sum())
        exact = max(t1 - t0, LD(0)) * ell
        if exact == 0:
            assert R.count == 0 or R.rows[0] <= R.bars[0] + R.overlap, (i, R.rows[0])
            continue
        assert R.count > 0, i
        gaps.append(float(abs(R.rows[0] - exact) / (R.bars[0] + R.overlap)))
        # the sharper statement: the excess has a known sign and size, the whole of `overlap`, up to the rounding bar alone.
        # Not for the two rays 1e-13 beside a face: there the lowest element on either side owns the piece, and where the two
        # sides are not mirror images the union of the owned intervals misses or doubles the chord by that distance times
        # the difference of the cotangents of the two edges that meet the face there: at most 2 x 1e-13 on these meshes,
        # whose edges are axis-parallel or at 45 degrees.
        if i not in (4, 5):
            sharp.append(float(abs((R.rows[0] - exact) - R.overlap) / R.bars[0]))
        else:
            assert abs((R.rows[0] - exact) - R.overlap) <= R.bars[0] + LD(2e-13), i
        assert abs(R.rows[6] - t0) <= R.bars[6] + R.overlap / ell and abs(R.rows[7] - t1) <= R.bars[7] + R.overlap / ell, i
    check("length %s" % g.name, gaps)
    print("length %s: largest ratio of |excess - overlap| to the rounding bar: %.3f" % (g.name, max(sharp)))
    assert max(sharp) <= 0.5, max(sharp)
    # the diagonal that runs along element edges (2-D) or through cell corners (3-D): one piece per cell, in the lowest element
    assert ref[8 if g.dim == 2 else 7].count == 2 ** (L - 1)


@pytest.mark.parametrize("kind,L,k", CASES)
def test_integral_of_the_paraboloid(lib, kind, L, k):
    """u = |x|^2 lies in both element spaces: int u ds = l [|a|^2 t + (a . d) t^2 + |d|^2 t^3 / 3] over the chord."""
    g = RU.host_mesh(kind, L, k)
    a, b = RU.rays(g.dim, 72)
    ref = RU.reference(g, (g.x * g.x).sum(axis=1), a, b)
    gaps = []
    for i, R in enumerate(ref):
        t0, t1 = chord(a[i], b[i])
        if not t1 > t0:
            continue
        al, d = a[i].astype(LD), b[i].astype(LD) - a[i].astype(LD)
        ell = np.sqrt((d * d).sum())
        F = lambda t: ell * ((al * al).sum() * t + (al * d).sum() * t * t + (d * d).sum() * t ** 3 / 3)
        gaps.append(float(abs(R.rows[1] - (F(t1) - F(t0))) / (R.bars[1] + R.overlap * g.dim)))
        # p = 2: along = u(leave) - u(enter) for a continuous field; |grad u| <= 2 sqrt(dim)
        u = lambda t: ((al + t * d) ** 2).sum()
        gap = abs(R.rows[2] - (u(t1) - u(t0)))
        gaps.append(float(gap / (R.bars[2] + R.overlap * 2 * np.sqrt(LD(g.dim)))))
        assert R.rows[5] >= -R.bars[5] and R.rows[4] <= g.dim + R.bars[4]
    check("paraboloid %s" % g.name, gaps)


@pytest.mark.parametrize("kind,L,k", [("fem3d", 1, 1), ("fem3d", 2, 3), ("fem3d", 3, 2), ("fem2d", 4, 0)])
def test_oblique_chords_against_a_12_point_rule(lib, kind, L, k):
    """u = x^k y^k z^k + x (2-D: x y + x) is a member of the element space; along a line its degree is at most 9, which a
    12-point Gauss rule on the WHOLE chord integrates exactly."""
    g = RU.host_mesh(kind, L, k)
    a, b = RU.rays(g.dim, 72)
    f = (lambda X: np.prod(X ** k, axis=-1) + X[..., 0]) if g.dim == 3 else (lambda X: X[..., 0] * X[..., 1] + X[..., 0])
    ref = RU.reference(g, f(g.x), a, b)
    gx, gw = RR.SR.gauss01(12)
    gaps = []
    for i, R in enumerate(ref):
        t0, t1 = chord(a[i], b[i])
        if not t1 > t0:
            continue
        al, d = a[i].astype(LD), b[i].astype(LD) - a[i].astype(LD)
        ell = np.sqrt((d * d).sum())
        tq = t0 + gx * (t1 - t0)
        exact = (gw * f(al[None, :] + tq[:, None] * d[None, :])).sum() * (t1 - t0) * ell
        gaps.append(float(abs(R.rows[1] - exact) / (R.bars[1] + R.overlap * 2)))      # |u| <= 2 on the box
    check("oblique chords %s" % g.name, gaps)


def test_gates_of_a_harmonic_field(lib):
    """2-D, p = 2, u = x^2 - y^2, grad u = (2 x, -2 y): through the chord x = x_0, |y| <= 1, upwards, across = -4 x_0 (the left
    normal is -e_x), downwards +4 x_0; the four gates of a closed quadrilateral sum to - int laplace u = 0."""
    g = RU.host_mesh("fem2d", 4)
    z = g.x[:, 0] ** 2 - g.x[:, 1] ** 2
    xs = [-0.75, -0.3, 0.0, 0.1, 0.625]
    a = np.array([[x0, -1.0] for x0 in xs] + [[x0, 1.0] for x0 in xs])
    b = np.array([[x0, 1.0] for x0 in xs] + [[x0, -1.0] for x0 in xs])
    ref = RU.reference(g, z, a, b)
    gaps = []
    for i, R in enumerate(ref):
        assert not R.undecided
        want = LD(-4 if i < 5 else 4) * LD(xs[i % 5])
        gaps.append(float(abs(R.rows[3] - want) / (R.bars[3] + R.overlap * 2 * np.sqrt(LD(2)))))
        assert abs(R.rows[0] - 2) <= R.bars[0] + R.overlap
    Q = np.array([[-0.6, -0.5], [0.7, -0.35], [0.55, 0.8], [-0.45, 0.6]])
    ref = RU.reference(g, z, Q, np.roll(Q, -1, axis=0))
    total = sum(R.rows[3] for R in ref)
    bar = sum(R.bars[3] + R.overlap * 2 * np.sqrt(LD(2)) for R in ref)
    gaps.append(float(abs(total) / bar))
    check("gates", gaps)


@pytest.mark.parametrize("L,count", [(1, 2), (2, 6)])
def test_chord_through_the_notch_of_the_l_shape(lib, L, count):
    """The line x + y = 0.3 from (-1.2, 1.5) to (1.5, -1.2) meets the L shape [-1, 1]^2 without (0, 1]^2 in two stretches, x
    in [-0.7, 0] and x in [0.3, 1]: at L = 1 one triangle each, at L = 2 three each (corner, centre, corner child)."""
    g = RU.host_mesh("lshape", L)
    a, b = np.array([[-1.2, 1.5]]), np.array([[1.5, -1.2]])
    R = RU.reference(g, g.x[:, 0].copy(), a, b)[0]
    assert not R.undecided and R.count == count
    ell = np.sqrt(LD(2)) * LD(27) / 10
    assert abs(R.rows[0] - np.sqrt(LD(2)) * LD(14) / 10) <= R.bars[0] + R.overlap
    assert abs(R.rows[6] - LD(5) / 27) <= R.bars[6] + R.overlap / ell and abs(R.rows[7] - LD(22) / 27) <= R.bars[7] + R.overlap / ell
    # int x ds over both stretches: sqrt(2) (0 - 0.49) / 2 + sqrt(2) (1 - 0.09) / 2
    assert abs(R.rows[1] - np.sqrt(LD(2)) * LD(21) / 100) <= R.bars[1] + R.overlap
    gap = np.sort(R.t0)[count // 2] - np.sort(R.t1)[count // 2 - 1]
    assert abs(gap - LD(3) / 27) <= 1e-10      # the notch
