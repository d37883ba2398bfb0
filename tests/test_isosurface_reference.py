"""The numpy yardstick tests/isosurface_reference.py against known answers, on the library's fem3d meshes (the mesh alone comes
from the library; no isosurface code of it runs here).

Field and level: the nodal interpolant of degree 2 of u = x^2 + y^2 + z^2 reproduces u, and c = 0.37 = 37/100 is no lattice
value (the lattice coordinates have denominators 2^a 3^b only).  The level is the sphere of radius r = sqrt(c) inside the cube
[-1, 1]^3: area 4 pi r^2, volume of {u > c} = 8 - 4/3 pi r^3.  The rule is second order in the item size, so each refine step
should divide the error by about 4; the bar is the factor >= 2.5 of test_levelset_reference.py.  Measured here, fem3d L = 3,
k = 2, r = 0 -> 1 -> 2: volume 1.134e-1, 3.026e-2, 7.521e-3 (3.75 and 4.02), area 3.098e-1, 8.454e-2, 2.081e-2 (3.66 and 4.06)."""
import math

import numpy as np
import pytest

import isosurface_reference as IR
import isosurface_util as IU

C0 = 0.37


@pytest.fixture(scope="module")
def mesh(lib):
    return IU.host_mesh(3, 2)


def sphere(mesh, refine, sign=1.0):
    """The yardstick of +-(x^2 + y^2 + z^2) at +-c, once per refine."""
    z = IU.paraboloid(mesh.x)
    return IU.reference("sphere%+d" % sign, mesh.x, sign * z, mesh.k, [sign * C0], refine)[0]


def test_kuhn_tetrahedra_tile_the_cell():
    """Six tetrahedra of volume 1/6 in lattice units, alternating orientation, all holding the diagonal; every face diagonal
    of the cell that is used runs from the lower to the upper corner, so neighbouring cells agree."""
    K = IR.kuhn()
    assert K.shape == (6, 4, 3) and (K[:, 0] == 0).all() and (K[:, 3] == 1).all()
    d = [int(round(np.linalg.det((K[t, 1:] - K[t, 0]).astype(float)))) for t in range(6)]
    assert sorted(d) == [-1, -1, -1, 1, 1, 1]
    assert len({tuple(map(tuple, K[t])) for t in range(6)}) == 6
    assert (np.diff(K.sum(axis=2), axis=1) == 1).all()      # each corner one axis step beyond the one before


def test_lagrange_is_nodal_and_reproduces_polynomials():
    for k in (1, 2, 3):
        nodes = np.arange(k + 1).astype(IR.LD) / k
        assert np.abs(IR.lagrange(k, nodes) - np.eye(k + 1)).max() < 1e-18
        f = np.linspace(0, 1, 9).astype(IR.LD)
        for deg in range(k + 1):
            assert np.abs(IR.lagrange(k, f) @ nodes ** deg - f ** deg).max() < 1e-17


def test_sphere_volume_and_area_converge_at_second_order(mesh):
    r = math.sqrt(C0)
    want_vol, want_area = 4.0 / 3.0 * math.pi * r ** 3, 4 * math.pi * r * r
    errs = []
    for refine in range(3):
        R = sphere(mesh, refine)
        errs.append((abs(8.0 - float(R.rows[0]) - want_vol), abs(float(R.rows[1]) - want_area)))
        print("fem3d L=3 k=2 r=%d: volume of the ball %.12f (error %.3e), area %.12f (error %.3e), %d triangles"
              % (refine, 8.0 - R.rows[0], errs[-1][0], R.rows[1], errs[-1][1], R.count))
    for refine in range(2):
        fv, fa = errs[refine][0] / errs[refine + 1][0], errs[refine][1] / errs[refine + 1][1]
        print("r = %d -> %d: the volume error falls by %.2f, the area error by %.2f" % (refine, refine + 1, fv, fa))
        assert fv >= 2.5 and fa >= 2.5


@pytest.mark.parametrize("refine", [0, 1])
def test_orientation_by_gauss(mesh, refine):
    """The normals point to the below side: around a ball that is above they point outwards and Gauss's sum
    1/6 sum det [P0, P1, P2] is column [0]; around a ball that is below it is column [0] minus the volume 8 of the cube."""
    R = sphere(mesh, refine, -1.0)
    s = IU.gauss(R.tri)
    print("r=%d: ball above, Gauss sum %.15f, column [0] %.15f" % (refine, s, R.rows[0]))
    assert s > 0 and abs(s - float(R.rows[0])) <= 1e-12 * float(R.rows[0])
    R = sphere(mesh, refine)
    s = IU.gauss(R.tri)
    print("r=%d: ball below, Gauss sum %.15f, column [0] - 8 %.15f" % (refine, s, R.rows[0] - 8))
    assert s < 0 and abs(s - (float(R.rows[0]) - 8.0)) <= 1e-12 * 8.0


def test_closed_surface_at_refine_0(mesh):
    """Every directed edge of the emitted triangles occurs exactly once and its reverse exactly once, bit for bit: every edge
    lies in two triangles, which run through it in opposite directions."""
    for sign in (1.0, -1.0):
        R = sphere(mesh, 0, sign)
        fwd, rev = IU.edge_pairs(R.tri.astype(np.float64))
        assert len(fwd) == 3 * R.count > 0 and set(fwd.values()) == {1}
        assert all(rev.get(e, 0) == 1 for e in fwd)


def test_excess_converges(mesh):
    """int_{u > c} (u - c) over the cube: 8 - 8 c + int_ball (c - r^2) = 8 - 8 c + 8/15 pi c^(5/2)."""
    want = 8.0 - 8.0 * C0 + 8.0 / 15.0 * math.pi * C0 ** 2.5
    errs = [abs(float(sphere(mesh, refine).rows[2]) - want) for refine in range(3)]
    print("excess errors r = 0, 1, 2: %.3e %.3e %.3e" % tuple(errs))
    assert errs[0] / errs[1] >= 2.5 and errs[1] / errs[2] >= 2.5


def test_lattice_planes_on_the_level(lib):
    """u = x, c = 0 (k = 2: dyadic coordinates): a whole lattice plane lies on the level.  A face on the level is emitted by the
    tetrahedron whose fourth corner is above and by no other: area exactly 4 (every triangle area is dyadic), volume 4 and
    excess 2 to the rounding of the sixths in np.longdouble, every vertex on x = 0, every normal along -x."""
    g = IU.host_mesh(2, 2)
    R = IR.isosurfaces(g.x, g.x[:, 0].copy(), 2, [0.0], 0)[0]
    assert R.rows[1] == 4 and abs(R.rows[0] - 4) <= 1e-17 and abs(R.rows[2] - 2) <= 1e-17 and R.count > 0
    t = R.tri.reshape(-1, 3, 3)
    assert (t[:, :, 0] == 0).all()
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert (n[:, 0] < 0).all() and (n[:, 1:] == 0).all() and abs(float(-n[:, 0].sum() / 2) - 4.0) == 0


def test_constant_field_and_levels_outside(lib):
    g = IU.host_mesh(2, 2)
    R = IR.isosurfaces(g.x, np.full(g.n, 0.3), 2, [0.3], 0)[0]
    assert R.count == 0 and (R.rows == 0).all()
    lo, hi = IR.isosurfaces(g.x, IU.paraboloid(g.x), 2, [-0.5, 3.5], 0)
    assert lo.count == hi.count == 0
    assert abs(lo.rows[0] - 8) <= 1e-17 * 8 * 64 and lo.rows[3] > 0 > lo.rows[4]          # below the minimum: everything above, not reached
    assert hi.rows[0] == 0 and hi.rows[3] < 0 < hi.rows[4]          # above the maximum 3
