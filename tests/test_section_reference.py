"""The yardstick tests/section_reference.py against closed forms (CPU, numpy only; the meshes come from the library's host
geometry).  On [-1, 1]^dim a plane that separates the domain has a known measure, and the integral of a field that lies in the
element space and its flow rate at p = 2 are polynomial integrals: every sum must come out within 1e-12 of the sum of its
absolute terms -- the exactness claim of the quadrature rules rests on this -- and the degenerate placements (planes on
element faces, on the boundary, on the faces of the Kuhn tetrahedra, outside) must cut every piece exactly once."""
import numpy as np
import pytest

import section_reference as SR
import section_util as SU

LD = SR.LD
TILT3 = [1.0, 0.5, 0.25, 0.05]
TILT2 = [1.0, 0.5, 0.05]


def gauss_yz(f, n=12):
    """int over [-1, 1]^2 of f(y, z), with the sum of the absolute terms, by an n x n Gauss rule in longdouble."""
    g, w = SR.gauss01(n)
    y, z = np.meshgrid(2 * g - 1, 2 * g - 1, indexing="ij")
    terms = f(y, z) * (2 * w)[:, None] * (2 * w)[None, :]
    return terms.sum(), np.abs(terms).sum()


def close(got, want, scale, who):
    print("%s: got %.18Lg, want %.18Lg, gap / bar %.3e" % (who, got, want, abs(got - want) / (SU.KTOL * scale)))
    assert abs(got - want) <= SU.KTOL * scale, who


@pytest.mark.parametrize("k", [1, 2, 3])
def test_axis_plane_3d(k):
    g = SU.host_mesh(3, 3, k)
    z = (g.x * g.x).sum(axis=1)
    R = SR.sections(g.x, z, 3, k, [[0.0, 0.0, 1.0, 0.3]])[0]
    close(R.rows[0], LD(4), R.abs_terms[0], "k=%d z = 0.3 area" % k)
    if k >= 2:
        close(R.rows[1], 4 * (LD(2) / 3 + LD(0.3) ** 2), R.abs_terms[1], "k=%d z = 0.3 int x^2 + y^2 + z^2" % k)
        close(R.rows[2], 4 * 2 * LD(0.3), R.abs_terms[2], "k=%d z = 0.3 flow rate" % k)
    assert R.count > 0 and (R.piece[:, [2, 5, 8]] == LD(0.3)).all()
    n = np.cross(R.piece[:, 3:6] - R.piece[:, 0:3], R.piece[:, 6:9] - R.piece[:, 0:3])
    assert (n[:, 2] < 0).all()      # towards the below side


@pytest.mark.parametrize("k", [1, 2, 3])
def test_tilted_plane_3d(k):
    g = SU.host_mesh(3, 3, k)
    X, Y, Z = g.x.T
    z = X ** k * Y ** k * Z ** k + X
    R = SR.sections(g.x, z, 3, k, [TILT3])[0]
    n0, n1, n2, c = (LD(v) for v in TILT3)
    nn = np.sqrt(n0 * n0 + n1 * n1 + n2 * n2)
    close(R.rows[0], 4 * np.sqrt(LD(1.3125)), R.abs_terms[0], "k=%d tilted area" % k)
    xs = lambda y, zz: (c - n1 * y - n2 * zz) / n0
    want, scale = gauss_yz(lambda y, zz: (xs(y, zz) ** k * y ** k * zz ** k + xs(y, zz)) * nn / n0)
    close(R.rows[1], want, max(scale, R.abs_terms[1]), "k=%d tilted int u" % k)
    assert R.count > R.ncut > 0      # wedges: two triangles of one item
    if k >= 2:
        h = X * X - Y * Y
        Rh = SR.sections(g.x, h, 3, k, [[1.0, 0.0, 0.0, 0.3], [1.0, 0.0, 0.0, -0.45], TILT3])
        close(Rh[0].rows[2], 2 * LD(0.3) * 4, Rh[0].abs_terms[2], "k=%d harmonic, x = 0.3" % k)
        close(Rh[1].rows[2], 2 * LD(-0.45) * 4, Rh[1].abs_terms[2], "k=%d harmonic, x = -0.45" % k)
        want, scale = gauss_yz(lambda y, zz: (2 * xs(y, zz) * n0 - 2 * y * n1) / n0)
        close(Rh[2].rows[2], want, max(scale, Rh[2].abs_terms[2]), "k=%d harmonic, tilted" % k)


def test_line_2d():
    g = SU.host_mesh(2, 3)
    X, Y = g.x.T
    z = X * X + X * Y
    R = SR.sections(g.x, z, 2, 0, [TILT2])[0]
    close(R.rows[0], 2 * np.sqrt(LD(1.25)), R.abs_terms[0], "2-D length")
    gq, w = SR.gauss01(8)
    y = 2 * gq - 1
    xs = LD(0.05) - LD(0.5) * y
    terms = (xs * xs + xs * y) * np.sqrt(LD(1.25)) * 2 * w
    close(R.rows[1], terms.sum(), max(np.abs(terms).sum(), R.abs_terms[1]), "2-D int x^2 + x y")
    # the flow rate of the same field at p = 2: grad u . nu = ((2 x + y) + 0.5 x) / sqrt(1.25)
    terms = (2 * xs + y + LD(0.5) * xs) * 2 * w
    close(R.rows[2], terms.sum(), max(np.abs(terms).sum(), R.abs_terms[2]), "2-D flow rate")
    # the above side on the left of every segment
    e = R.piece[:, 2:4] - R.piece[:, 0:2]
    assert (e[:, 0] * LD(0.5) - e[:, 1] * LD(1.0) > 0).all()      # cross(e, n) < 0 <=> n on the left


def unique_pieces(R, dim):
    V = np.asarray(R.piece[:, :dim * dim], dtype=np.float64).reshape(-1, dim, dim) + 0.0
    keys = {tuple(sorted(map(tuple, v))) for v in V}
    return len(keys) == len(V)


@pytest.mark.parametrize("k", [1, 2])
def test_degenerate_placements(k):
    g = SU.host_mesh(3, 3, k)
    z = g.x[:, 0] + 2.0
    block = (k + 1) ** 3
    centre = g.x.reshape(-1, block, 3).mean(axis=1)
    faces, left, right, kuhn, outside = SR.sections(g.x, z, 3, k, [[1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, -1.0], [1.0, 0.0, 0.0, 1.0],
                                                                    [1.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 2.0]])
    # 16 element faces, two triangles each, whose areas are dyadic: their sum is exactly 4; the quadrature weights round
    assert SU.piece_measure(faces.piece, 3).sum() == 4 and faces.count == 2 * 16 and unique_pieces(faces, 3)
    assert (centre[faces.items // 6, 0] > 0).all() and (faces.piece[:, [0, 3, 6]] == 0).all()
    for j, want in enumerate((4, 8, 4)):      # area, int (x + 2), flow rate of grad = e_x
        close(faces.rows[j], LD(want), faces.abs_terms[j], "k=%d x = 0 column %d" % (k, j))
    assert abs(faces.rows[3] - 2) <= faces.mbar and abs(faces.rows[4] + 2) <= faces.mbar
    assert SU.piece_measure(left.piece, 3).sum() == 4 and left.count == 32 and unique_pieces(left, 3)
    close(left.rows[0], LD(4), left.abs_terms[0], "k=%d x = -1 area" % k)
    close(left.rows[1], LD(4), left.abs_terms[1], "k=%d x = -1 int (x + 2)" % k)
    for R in (right, outside):
        assert R.count == 0 and len(R.items) == 0 and np.array_equal(R.rows, [0, 0, 0, -np.inf, -np.inf])
    close(kuhn.rows[0], 4 * np.sqrt(LD(2)), kuhn.abs_terms[0], "k=%d Kuhn plane area" % k)
    assert unique_pieces(kuhn, 3) and kuhn.count > 0
    assert abs(SU.piece_measure(kuhn.piece, 3).sum() - kuhn.rows[0]) <= SU.KTOL * kuhn.abs_terms[0]


def test_degenerate_placements_2d():
    g = SU.host_mesh(2, 3)
    z = g.x[:, 0] + 2.0
    edges, left, right, diag, outside = SR.sections(g.x, z, 2, 0, [[1.0, 0.0, 0.0], [1.0, 0.0, -1.0], [1.0, 0.0, 1.0], [1.0, -1.0, 0.0],
                                                                    [0.0, 1.0, 3.0]])
    centre = g.x.reshape(-1, 7, 2)[:, 6]
    assert SU.piece_measure(edges.piece, 2).sum() == 2 and unique_pieces(edges, 2) and (centre[edges.items, 0] > 0).all()
    close(edges.rows[0], LD(2), edges.abs_terms[0], "2-D x = 0 length")
    assert SU.piece_measure(left.piece, 2).sum() == 2 and unique_pieces(left, 2)
    close(left.rows[0], LD(2), left.abs_terms[0], "2-D x = -1 length")
    for R in (right, outside):
        assert R.count == 0 and np.array_equal(R.rows, [0, 0, 0, -np.inf, -np.inf])
    close(diag.rows[0], 2 * np.sqrt(LD(2)), diag.abs_terms[0], "2-D diagonal length")
    assert unique_pieces(diag, 2)


def test_gauss_rules():
    for n in (3, 4, 6, 12):
        x, w = SR.gauss01(n)
        for d in range(2 * n):
            assert abs((w * x ** d).sum() - LD(1) / (d + 1)) <= 4 * np.finfo(LD).eps
