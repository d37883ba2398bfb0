"""The numpy yardstick tests/levelset_reference.py against known answers, on the library's fem2d meshes (the mesh alone comes
from the library; no level-set code of it runs here).

Field and level: the nodal interpolant of u = x^2 + y^2 reproduces u, and c = 0.37 = 37/100 is no lattice value (those are
rationals with denominators 9 4^m).  The contour is the circle of radius sqrt(c): length 2 pi sqrt(c), area of {u > c} on the
square [-1, 1]^2 is 4 - pi c.  The rule is second order in the item size, so each refine step should divide the error by
about 4; the bar is a factor >= 2.5 at L = 4 (a prototype on the diagonally split square measured 3.9 .. 4.1 and nothing below
3.0 from L = 2 up).  Measured here, fem2d L = 4, r = 0 -> 1 -> 2: length 4.13 and 3.90, area 3.97 and 3.95."""
import math

import numpy as np
import pytest

import levelset_reference as LR
import levelset_util as LU

C0 = 0.37


@pytest.fixture(scope="module")
def mesh4(lib):
    return LU.host_mesh("fem2d", 4)


def test_small_triangles_tile_the_macro_triangle():
    """N^2 small triangles of area 1 / (2 N^2) in lattice units, every lattice point inside, orientation kept."""
    for r in range(4):
        N = 2 ** r
        T = LR.small_triangles(r)
        assert T.shape == (N * N, 3, 2) and (T >= 0).all() and (T.sum(axis=2) <= N).all()
        a, b, c = T[:, 0], T[:, 1], T[:, 2]
        twice = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
        assert (twice == 1).all()
        assert len({tuple(sorted(map(tuple, t))) for t in T}) == N * N


def test_basis_is_nodal_and_reproduces_quadratics():
    Nb = LR.basis(LR.REF[:, 0], LR.REF[:, 1])
    assert np.abs(Nb - np.eye(7)).max() < 1e-18
    rng = np.random.default_rng(0)
    p = rng.random((20, 2)).astype(LR.LD) / 2
    q = lambda x, y: 0.3 + x - 2 * y + 0.7 * x * x - x * y + 1.3 * y * y
    got = LR.basis(p[:, 0], p[:, 1]) @ q(LR.REF[:, 0], LR.REF[:, 1])
    assert np.abs(got - q(p[:, 0], p[:, 1])).max() < 1e-17


def test_circle_length_and_area_converge_at_second_order(mesh4):
    z = LU.paraboloid(mesh4.x)
    want_len, want_area = 2 * math.pi * math.sqrt(C0), 4 - math.pi * C0
    errs = []
    for r in range(3):
        R = LR.level_sets(mesh4.x, z, [C0], r)[0]
        errs.append((abs(float(R.rows[1]) - want_len), abs(float(R.rows[0]) - want_area)))
        print("fem2d L=4 r=%d: length %.12f (error %.3e), area %.12f (error %.3e), %d segments"
              % (r, R.rows[1], errs[-1][0], R.rows[0], errs[-1][1], R.count))
    for r in range(2):
        fl, fa = errs[r][0] / errs[r + 1][0], errs[r][1] / errs[r + 1][1]
        print("r = %d -> %d: the length error falls by %.2f, the area error by %.2f" % (r, r + 1, fl, fa))
        assert fl >= 2.5 and fa >= 2.5


@pytest.mark.parametrize("refine", [0, 1])
def test_orientation_by_green(lib, refine):
    """The above side lies to the left: around a disk that is above the loop runs counter-clockwise and encloses column [0];
    around a disk that is below it runs clockwise, and the sum is column [0] minus the area 4 of the square.  Also on the mesh
    whose second half has elements of negative determinant."""
    for mixed in (False, True):
        g = LU.host_mesh("fem2d", 3, mixed)
        z = LU.paraboloid(g.x)
        R = LR.level_sets(g.x, -z, [-C0], refine)[0]
        s = LU.green(R.seg)
        print("mixed=%s r=%d: disk above, Green sum %.15f, column [0] %.15f" % (mixed, refine, s, R.rows[0]))
        assert s > 0 and abs(s - float(R.rows[0])) <= 1e-12 * float(R.rows[0])
        R = LR.level_sets(g.x, z, [C0], refine)[0]
        s = LU.green(R.seg)
        print("mixed=%s r=%d: disk below, Green sum %.15f, column [0] - 4 %.15f" % (mixed, refine, s, R.rows[0] - 4))
        assert s < 0 and abs(s - (float(R.rows[0]) - 4.0)) <= 1e-12 * 4.0


def test_excess_is_the_integral_of_the_linear_pieces(mesh4):
    """int_{u > c} (u - c) of u = x^2 + y^2 on the square: 8/3 - 4 c + pi c^2 / 2; the piecewise linear rule converges to it."""
    z = LU.paraboloid(mesh4.x)
    want = 8.0 / 3.0 - 4 * C0 + math.pi * C0 * C0 / 2
    errs = [abs(float(LR.level_sets(mesh4.x, z, [C0], r)[0].rows[2]) - want) for r in range(3)]
    print("excess errors r = 0, 1, 2: %.3e %.3e %.3e" % tuple(errs))
    assert errs[0] / errs[1] >= 2.5 and errs[1] / errs[2] >= 2.5
