"""CPU tests of the host restatement mgb_geo_isosurfaces_host (csrc/isosurface.hpp: the per-item routine the gfx950 kernels
also run) against the numpy yardstick tests/isosurface_reference.py, plus the exact degenerate cases, the closed surface and
the argument errors.

Bars (tests/isosurface_reference.py, tests/isosurface_util.py): counts, items and row offsets equal; every vertex within
8 eps (|P_hi - P_lo|_inf + max|x|), for r > 0 plus 32 eps (S / |v_hi - v_lo|) |P_hi - P_lo|_inf; the three sums within 1e-12 of
the sum of their absolute terms; the maxima within 8 eps (max|v| + |c|).  Largest ratios measured: vertices 0.063 at r = 0 and
0.024 at r > 0, sums 3.0e-4, maxima 0.050."""
import numpy as np
import pytest

import isosurface_util as IU

LEVELS = [0.37, 0.91, 1.37]      # n/100: never a lattice value of x^2 + y^2 + z^2 (denominators 2^a 3^b)


def tilted(x):
    """A field without symmetry that every degree reproduces."""
    return x[:, 0] + 0.5 * x[:, 1] + 0.25 * x[:, 2] + 0.05


def smooth(x):
    """A field without symmetry, continuous across the elements."""
    return np.sin(3.0 * x[:, 0] + 0.5) * np.cos(2.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 2] + 0.2 * x[:, 2]


@pytest.mark.parametrize("L,k,refine", [(1, 1, 0), (2, 3, 0), (3, 2, 0), (3, 2, 1), (1, 1, 2), (2, 3, 1)])
def test_host_against_numpy(lib, L, k, refine):
    g = IU.host_mesh(L, k)
    z = np.stack([np.zeros(g.n), IU.paraboloid(g.x) if k > 1 else tilted(g.x)], axis=1)      # column 1 of 2: a wrong stride shows
    levels = LEVELS if k > 1 else [-0.31, 0.23, 0.97]
    got = IU.host_isosurfaces(lib, g, [z], levels, refine, u=1)
    IU.against_reference("fem3d L=%d k=%d r=%d" % (L, k, refine), got, g, [z], levels, refine, u=1)
    assert (got.counts > 0).all()
    assert got.rows.shape == (1, 3, 5) and len(got.tri) == got.offsets[-1]


def test_six_items(lib):
    """L = 1, k = 1: one element, one cell, six items; the plane x + y/2 + z/4 = -0.05 cuts every one of them."""
    g = IU.host_mesh(1, 1)
    assert g.items() == 6
    got = IU.host_isosurfaces(lib, g, [tilted(g.x)], [0.0])
    tri, item = got.row(0, 0)
    assert set(item.tolist()) == set(range(6)) and len(item) > 6      # some items are wedges: two triangles each
    n = np.cross(tri[:, 3:6] - tri[:, 0:3], tri[:, 6:9] - tri[:, 0:3])
    assert (n @ np.array([1.0, 0.5, 0.25]) < 0).all()                  # every normal points down the gradient


@pytest.mark.parametrize("L,k", [(2, 1), (2, 3)])
def test_host_against_numpy_on_broken_and_smooth_fields(lib, L, k):
    """r = 0 (values are loaded: classification is exact): a random field, broken across the elements, and a smooth one, three
    fields and four levels in one call, one level above every value."""
    g = IU.host_mesh(L, k)
    rng = np.random.default_rng(40 + k)
    fields = [rng.standard_normal(g.n), smooth(g.x), rng.standard_normal(g.n)]
    levels = [-0.4, 0.0, 0.55, 9.0]
    got = IU.host_isosurfaces(lib, g, fields, levels)
    IU.against_reference("fem3d L=%d k=%d r=0 three fields" % (L, k), got, g, fields, levels, 0)
    assert (got.counts[:, 3] == 0).all() and (got.rows[:, 3, 3] < 0).all() and (got.rows[:, 3, 0] == 0).all()
    # wedges: more triangles than emitting items
    tri, item = got.row(1, 1)
    assert len(item) > len(np.unique(item)) > 0
    twice = item[1:] == item[:-1]
    assert twice.any() and (np.diff(item) >= 0).all()


def test_lattice_planes_on_the_level(lib):
    """u = x with c = 0 on dyadic coordinates: the area is exactly 4 (the faces on the level are emitted once), volume 4, excess 2."""
    g = IU.host_mesh(2, 2)
    z = g.x[:, 0].copy()
    got = IU.host_isosurfaces(lib, g, [z], [0.0])
    IU.against_reference("u = x, c = 0", got, g, [z], [0.0], 0)
    print("u = x, c = 0: rows %s, %d triangles" % (got.rows[0, 0], got.counts[0, 0]))
    assert got.rows[0, 0, 1] == 4.0 and np.abs(got.rows[0, 0, [0, 2]] - [4.0, 2.0]).max() <= 1e-12 and got.counts[0, 0] > 0
    assert (got.tri[:, [0, 3, 6]] == 0).all()


def test_a_corner_on_the_level_with_three_above_gives_no_triangle(lib):
    """One element: node 0 is corner 0 of all six tetrahedra; it lies on the level and every other node above."""
    g = IU.host_mesh(1, 1)
    z = np.ones(8)
    z[0] = 0.25
    got = IU.host_isosurfaces(lib, g, [z], [0.25, 0.5])
    IU.against_reference("corner on the level", got, g, [z], [0.25, 0.5], 0)
    assert got.counts[0, 0] == 0 and got.rows[0, 0, 1] == 0.0 and got.rows[0, 0, 0] == 8.0 and got.rows[0, 0, 4] == 0.0
    assert got.counts[0, 1] == 6 and got.rows[0, 1, 1] > 0.0      # the level above it cuts the corner off in every item


def test_constant_field_on_the_level(lib):
    g = IU.host_mesh(2, 2)
    got = IU.host_isosurfaces(lib, g, [np.full(g.n, 0.3)], [0.3])
    assert got.counts[0, 0] == 0 and np.array_equal(got.rows[0, 0], np.zeros(5))


def test_level_outside_the_range(lib):
    g = IU.host_mesh(2, 2)
    z = IU.paraboloid(g.x)
    got = IU.host_isosurfaces(lib, g, [z], [3.5, -0.5])
    IU.against_reference("levels outside", got, g, [z], [3.5, -0.5], 0)
    assert np.array_equal(got.counts, [[0, 0]])
    assert got.rows[0, 0, 0] == 0.0 and got.rows[0, 0, 3] < 0 < got.rows[0, 0, 4]            # above the maximum: not reached
    assert abs(got.rows[0, 1, 0] - 8.0) <= 1e-12 and got.rows[0, 1, 4] < 0 < got.rows[0, 1, 3]


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_node_is_never_dropped(lib, bad):
    g = IU.host_mesh(2, 3)
    z = IU.paraboloid(g.x)
    clean = IU.host_isosurfaces(lib, g, [z, z + 0.1], LEVELS)
    zb = z.copy()
    node = 64 * 5 + 21      # local node (1, 1, 1) of element 5: the eight cells around it hold it
    zb[node] = bad
    got = IU.host_isosurfaces(lib, g, [zb, z + 0.1], LEVELS)
    IU.against_reference("non-finite node", got, g, [zb, z + 0.1], LEVELS, 0)
    assert np.isnan(got.rows[0]).all()
    assert got.rows[1].tobytes() == clean.rows[1].tobytes() and np.array_equal(got.counts[1], clean.counts[1])
    missing = 0
    for l in range(len(LEVELS)):
        tri, item = got.row(0, l)
        ctri, citem = clean.row(0, l)
        keep = np.isin(citem, item)
        assert np.array_equal(item, citem[keep]) and tri.tobytes() == ctri[keep].tobytes()
        assert got.row(1, l)[0].tobytes() == clean.row(1, l)[0].tobytes()
        assert (citem[~keep] // 162 == 5).all()      # only items of element 5 (162 items each) are missing
        missing += int((~keep).sum())
    assert missing > 0


@pytest.mark.parametrize("L,k", [(2, 3), (3, 2)])
def test_closed_surface_at_refine_0(lib, L, k):
    """Every directed edge whose endpoints are not both on the boundary of the cube occurs once, and its reverse once."""
    g = IU.host_mesh(L, k)
    for z, levels in ((IU.paraboloid(g.x), LEVELS), (smooth(g.x), [-0.4, 0.1, 0.55])):
        got = IU.host_isosurfaces(lib, g, [z], levels)
        for l in range(len(levels)):
            tri, _ = got.row(0, l)
            fwd, rev = IU.edge_pairs(tri)
            inner = [e for e in fwd if not (np.abs(np.frombuffer(e, dtype=np.float64).reshape(2, 3)) == 1.0).any(axis=1).all()]
            assert len(inner) > 0 and all(fwd[e] == 1 and rev.get(e, 0) == 1 for e in inner), (L, k, levels[l])


def test_orientation_by_gauss(lib):
    g = IU.host_mesh(3, 2)
    z = IU.paraboloid(g.x)
    for refine in (0, 1):
        got = IU.host_isosurfaces(lib, g, [-z, z], [-0.37, 0.37], refine)
        ball, hole = IU.gauss(got.row(0, 0)[0]), IU.gauss(got.row(1, 1)[0])
        print("r=%d: Gauss sums %.15f %.15f, columns [0] %.15f %.15f" % (refine, ball, hole, got.rows[0, 0, 0], got.rows[1, 1, 0]))
        assert ball > 0 and abs(ball - got.rows[0, 0, 0]) <= 1e-12 * got.rows[0, 0, 0]
        assert hole < 0 and abs(hole - (got.rows[1, 1, 0] - 8.0)) <= 1e-12 * 8.0


def test_argument_errors(lib):
    from mgb_amd import _lib
    import levelset_util as LU
    g3, g2 = IU.host_mesh(2, 1), LU.host_mesh("fem2d", 2)
    z3 = np.zeros((g3.n, 2))
    ok = dict(levels=[0.1], refine=0, rc_only=True)
    assert IU.host_isosurfaces(lib, g3, [z3], **ok) == 0
    for kw, msg in ((dict(B=0), b"B must be >= 1"), (dict(nl=0), b"nl must be >= 1"), (dict(S=0), b"S must be >= 1"),
                    (dict(u=2), b"column u outside"), (dict(u=-1), b"column u outside"), (dict(refine=3), b"refine must be 0, 1 or 2"),
                    (dict(refine=-1), b"refine must be 0, 1 or 2"), (dict(levels=[np.nan]), b"every level must be finite"),
                    (dict(levels=[0.1, np.inf]), b"every level must be finite")):
        assert IU.host_isosurfaces(lib, g3, [z3], **{**ok, **kw}) == IU.MGB_E_ARG, kw
        err = lib.mgb_last_error()
        assert b"geo_isosurfaces_host" in err and msg in err, (kw, err)
    rows, counts = np.empty(5), np.empty(1, dtype=np.int64)
    cp = counts.ctypes.data_as(_lib.c_ll_p)
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z3))
    lv = np.array([0.1])
    call = lambda h, t, l, r, c: lib.mgb_geo_isosurfaces_host(h, 1, t, 2, 0, 1, l, 0, r, c, None, None, None, 0)
    assert call(g3.handle, table, _lib.dptr(lv), _lib.dptr(rows), cp) == 0
    for args in ((None, table, _lib.dptr(lv), _lib.dptr(rows), cp), (g3.handle, None, _lib.dptr(lv), _lib.dptr(rows), cp),
                 (g3.handle, table, None, _lib.dptr(rows), cp), (g3.handle, table, _lib.dptr(lv), None, cp),
                 (g3.handle, table, _lib.dptr(lv), _lib.dptr(rows), None)):
        assert call(*args) == IU.MGB_E_ARG and b"null argument" in lib.mgb_last_error()
    assert call(g3.handle, (_lib.c_dbl_p * 1)(None), _lib.dptr(lv), _lib.dptr(rows), cp) == IU.MGB_E_ARG
    assert b"null field" in lib.mgb_last_error()
    # triangles without items, and arrays that are too small
    tri, item = np.empty((1, 9)), np.empty(1, dtype=np.int32)
    z = tilted(g3.x)
    t1 = (_lib.c_dbl_p * 1)(_lib.dptr(z))
    lv = np.array([0.0])
    host = lambda tp, ip, cap: lib.mgb_geo_isosurfaces_host(g3.handle, 1, t1, 1, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows), cp, None, tp, ip, cap)
    assert host(_lib.dptr(tri), None, 1) == IU.MGB_E_ARG and b"come together" in lib.mgb_last_error()
    assert host(_lib.dptr(tri), _lib.iptr(item), -1) == IU.MGB_E_ARG and b"negative capacity" in lib.mgb_last_error()
    assert host(_lib.dptr(tri), _lib.iptr(item), 1) == IU.MGB_E_ARG and b"more triangles than the arrays hold" in lib.mgb_last_error()
    # 1-D and 2-D geometries belong to level_sets
    z2 = np.zeros(g2.n)
    assert lib.mgb_geo_isosurfaces_host(g2.handle, 1, (_lib.c_dbl_p * 1)(_lib.dptr(z2)), 1, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows), cp,
                                        None, None, None, 0) == IU.MGB_E_ARG
    assert b"level_sets" in lib.mgb_last_error()


def test_python_names():
    import mgb_amd as M
    assert {"isosurfaces", "Isosurfaces"} <= set(M.__all__)
