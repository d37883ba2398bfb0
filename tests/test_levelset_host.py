"""CPU tests of the host restatement mgb_geo_level_sets_host (csrc/levelset.hpp: the per-item routine the gfx950 kernels also
run) against the numpy yardstick tests/levelset_reference.py, plus the exact degenerate cases, watertightness, 1-D and the
argument errors.

Bars (tests/levelset_reference.py, tests/levelset_util.py): counts, items and row offsets equal; every endpoint within
8 eps (|P_hi - P_lo|_inf + max|x|), for r > 0 plus 32 eps (S / |v_hi - v_lo|) |P_hi - P_lo|_inf; the three sums within 1e-12 of
the sum of their absolute terms; the maxima within 8 eps (max|v| + |c|).  Largest ratios measured: endpoints 0.083 at r = 0 and
0.059 at r > 0, sums 7e-4, maxima 0.048."""
import numpy as np
import pytest

import levelset_reference as LR
import levelset_util as LU

LEVELS = [0.37, 0.91, 1.37]      # n/100: never a lattice value of x^2 + y^2 (denominators 9 4^m)


def smooth(x):
    """A field without symmetry, continuous across the elements."""
    return np.sin(3.0 * x[:, 0] + 0.5) * np.cos(2.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 1]


@pytest.mark.parametrize("L,refine", [(2, 0), (3, 0), (4, 0), (2, 1), (3, 2), (2, 3)])
def test_host_against_numpy(lib, L, refine):
    g = LU.host_mesh("fem2d", L)
    z = np.stack([np.zeros(g.n), LU.paraboloid(g.x)], axis=1)      # column 1 of 2: a wrong stride or column shows
    got = LU.host_level_sets(lib, g, [z], LEVELS, refine, u=1)
    LU.against_reference("fem2d L=%d r=%d paraboloid" % (L, refine), got, g.x, [z], LEVELS, refine, u=1)
    assert (got.counts > 0).all()


@pytest.mark.parametrize("L", [2, 4])
def test_host_against_numpy_on_broken_and_smooth_fields(lib, L):
    """r = 0 (values are loaded: classification is exact): a random field, broken across the elements, and a smooth one, three
    fields and four levels in one call, one level above every value."""
    g = LU.host_mesh("fem2d", L)
    rng = np.random.default_rng(40 + L)
    fields = [rng.standard_normal(g.n), smooth(g.x), rng.standard_normal(g.n)]
    levels = [-0.4, 0.0, 0.55, 9.0]
    got = LU.host_level_sets(lib, g, fields, levels)
    LU.against_reference("fem2d L=%d r=0 three fields" % L, got, g.x, fields, levels, 0)
    assert (got.counts[:, 3] == 0).all() and (got.rows[:, 3, 3] < 0).all() and (got.rows[:, 3, 0] == 0).all()


@pytest.mark.parametrize("L", [2, 3])
def test_nodes_on_the_level(lib, L):
    """u = x with c = 0: nodes and whole edges lie on the level.  Above is exactly half the square, the contour is the line
    x = 0 of length 2 -- an edge on the level is emitted only by the triangle whose third corner is above, a corner on the level
    with both others above emits nothing -- and every segment runs downwards (above, x > 0, on its left)."""
    g = LU.host_mesh("fem2d", L)
    z = g.x[:, 0].copy()
    got = LU.host_level_sets(lib, g, [z], [0.0])
    LU.against_reference("fem2d L=%d u = x, c = 0" % L, got, g.x, [z], [0.0], 0)
    seg, _ = got.row(0, 0)
    print("u = x, c = 0, L=%d: above %.17g, length %.17g, %d segments" % (L, got.rows[0, 0, 0], got.rows[0, 0, 1], len(seg)))
    assert abs(got.rows[0, 0, 0] - 2.0) <= 1e-12 and abs(got.rows[0, 0, 1] - 2.0) <= 1e-12
    assert abs(got.rows[0, 0, 2] - 1.0) <= 1e-12      # int_{x > 0} x over the square
    assert np.array_equal(seg[:, [0, 2]], np.zeros((len(seg), 2))) and (seg[:, 3] < seg[:, 1]).all()
    assert abs(np.sum(seg[:, 1] - seg[:, 3]) - 2.0) <= 1e-12 and got.counts[0, 0] == len(seg) > 0


def test_constant_field_on_the_level(lib):
    g = LU.host_mesh("fem2d", 2)
    got = LU.host_level_sets(lib, g, [np.full(g.n, 0.3)], [0.3])
    assert got.counts[0, 0] == 0 and np.array_equal(got.rows[0, 0], np.zeros(5))


def test_level_outside_the_range(lib):
    g = LU.host_mesh("fem2d", 2)
    z = LU.paraboloid(g.x)
    got = LU.host_level_sets(lib, g, [z], [2.5, -0.5])
    LU.against_reference("levels outside", got, g.x, [z], [2.5, -0.5], 0)
    assert np.array_equal(got.counts, [[0, 0]])
    assert got.rows[0, 0, 0] == 0.0 and got.rows[0, 0, 3] < 0 < got.rows[0, 0, 4]            # above the maximum: not reached
    assert abs(got.rows[0, 1, 0] - 4.0) <= 1e-12 and got.rows[0, 1, 4] < 0 < got.rows[0, 1, 3]


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_node_is_never_dropped(lib, bad):
    g = LU.host_mesh("fem2d", 3)
    z = LU.paraboloid(g.x)
    clean = LU.host_level_sets(lib, g, [z, z + 0.1], LEVELS)
    zb = z.copy()
    node = 7 * 5 + 1      # v2 of element 5: four items hold it
    zb[node] = bad
    got = LU.host_level_sets(lib, g, [zb, z + 0.1], LEVELS)
    LU.against_reference("non-finite node", got, g.x, [zb, z + 0.1], LEVELS, 0)
    assert np.isnan(got.rows[0]).all()
    assert got.rows[1].tobytes() == clean.rows[1].tobytes() and np.array_equal(got.counts[1], clean.counts[1])
    holds = {(5 * 6 + k) for k in (1, 2)}      # ring position 2: the macro triangles (m12, v2, C) and (v2, m23, C)
    for l in range(len(LEVELS)):
        seg, item = got.row(0, l)
        cseg, citem = clean.row(0, l)
        assert not (set(item.tolist()) & holds)
        keep = ~np.isin(citem, list(holds))
        assert np.array_equal(item, citem[keep]) and seg.tobytes() == cseg[keep].tobytes()
        assert got.row(1, l)[0].tobytes() == clean.row(1, l)[0].tobytes()


def test_orientation_on_elements_of_negative_determinant(lib):
    g = LU.host_mesh("fem2d", 3, mixed=True)
    xe = g.x.reshape(-1, 7, 2)
    det = (xe[:, 1, 0] - xe[:, 0, 0]) * (xe[:, 2, 1] - xe[:, 0, 1]) - (xe[:, 1, 1] - xe[:, 0, 1]) * (xe[:, 2, 0] - xe[:, 0, 0])
    assert (det < 0).any() and (det > 0).any()
    z = LU.paraboloid(g.x)
    for refine in (0, 1):
        got = LU.host_level_sets(lib, g, [-z, z], [-0.37, 0.37], refine)
        disk, _ = got.row(0, 0)
        hole, _ = got.row(1, 1)
        print("r=%d: Green sums %.15f %.15f, columns [0] %.15f %.15f"
              % (refine, LU.green(disk), LU.green(hole), got.rows[0, 0, 0], got.rows[1, 1, 0]))
        assert LU.green(disk) > 0 and abs(LU.green(disk) - got.rows[0, 0, 0]) <= 1e-12 * got.rows[0, 0, 0]
        assert LU.green(hole) < 0 and abs(LU.green(hole) - (got.rows[1, 1, 0] - 4.0)) <= 1e-12 * 4.0
        used = np.unique(got.row(0, 0)[1] // (6 * 4 ** refine))
        assert (det[used] < 0).any() and (det[used] > 0).any()


@pytest.mark.parametrize("L", [2, 4])
def test_watertight_at_refine_0(lib, L):
    """Every endpoint that is not on the boundary of the square occurs an even number of times, bit for bit."""
    g = LU.host_mesh("fem2d", L)
    for z, levels in ((LU.paraboloid(g.x), LEVELS), (smooth(g.x), [-0.4, 0.1, 0.55])):
        got = LU.host_level_sets(lib, g, [z], levels)
        for l in range(len(levels)):
            seg, _ = got.row(0, l)
            pts = seg.reshape(-1, 2)
            inner = pts[(np.abs(pts) != 1.0).all(axis=1)]
            _, times = np.unique(inner.view([("x", "f8"), ("y", "f8")]), return_counts=True)
            assert len(inner) > 0 and (times % 2 == 0).all(), (L, levels[l], times)


def test_fem1d(lib):
    g = LU.host_mesh("fem1d", 3)
    z = np.stack([g.x[:, 0] ** 2 - 0.3, np.ones(g.n)], axis=1)
    levels = [-0.2, 0.0, 0.25, 0.7, 1.0]
    got = LU.host_level_sets(lib, g, [z, -z], levels)
    LU.against_reference("fem1d L=3", got, g.x, [z, -z], levels, 0)
    pts, item = got.row(0, 1)
    assert np.array_equal(got.counts[0], [2, 2, 2, 0, 0]) and got.seg.shape[1] == 2
    assert np.abs(np.abs(pts[:, 0]) - np.sqrt(0.3)).max() < 0.02 and np.array_equal(pts[:, 1], [-1.0, 1.0])
    assert np.array_equal(got.row(1, 1)[0][:, 1], [1.0, -1.0])
    assert got.rows[0, 1, 1] == 2.0 and abs(got.rows[0, 1, 0] - (2 - 2 * np.sqrt(0.3))) < 0.02


def test_argument_errors(lib):
    g2, g1 = LU.host_mesh("fem2d", 2), LU.host_mesh("fem1d", 3)
    z2, z1 = np.zeros((g2.n, 2)), np.zeros(g1.n)
    ok = dict(levels=[0.1], refine=0, rc_only=True)
    assert LU.host_level_sets(lib, g2, [z2], **ok) == 0
    for kw in (dict(B=0), dict(nl=0), dict(S=0), dict(u=2), dict(u=-1), dict(refine=4), dict(refine=-1), dict(levels=[np.nan]),
               dict(levels=[0.1, np.inf])):
        assert LU.host_level_sets(lib, g2, [z2], **{**ok, **kw}) == LU.MGB_E_ARG, kw
        assert b"geo_level_sets_host" in lib.mgb_last_error()
    assert LU.host_level_sets(lib, g1, [z1], **{**ok, "refine": 1}) == LU.MGB_E_ARG
    from mgb_amd import _lib
    import ctypes as C
    rows, counts = np.empty(5), np.empty(1, dtype=np.int64)
    cp = counts.ctypes.data_as(_lib.c_ll_p)
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z2))
    lv = np.array([0.1])
    call = lambda h, t, l, r, c: lib.mgb_geo_level_sets_host(h, 1, t, 2, 0, 1, l, 0, r, c, None, None, None, 0)
    assert call(g2.handle, table, _lib.dptr(lv), _lib.dptr(rows), cp) == 0
    for args in ((None, table, _lib.dptr(lv), _lib.dptr(rows), cp), (g2.handle, None, _lib.dptr(lv), _lib.dptr(rows), cp),
                 (g2.handle, table, None, _lib.dptr(rows), cp), (g2.handle, table, _lib.dptr(lv), None, cp),
                 (g2.handle, table, _lib.dptr(lv), _lib.dptr(rows), None),
                 (g2.handle, (_lib.c_dbl_p * 1)(None), _lib.dptr(lv), _lib.dptr(rows), cp)):
        assert call(*args) == LU.MGB_E_ARG
    # segments without items, and arrays that are too small
    seg = np.empty((1, 4))
    z = LU.paraboloid(g2.x)
    t1 = (_lib.c_dbl_p * 1)(_lib.dptr(z))
    lv = np.array([0.37])
    assert lib.mgb_geo_level_sets_host(g2.handle, 1, t1, 1, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows), cp, None, _lib.dptr(seg), None, 1) == LU.MGB_E_ARG
    item = np.empty(1, dtype=np.int32)
    assert lib.mgb_geo_level_sets_host(g2.handle, 1, t1, 1, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows), cp, None, _lib.dptr(seg), _lib.iptr(item), 1) == LU.MGB_E_ARG
    h3 = C.c_void_p()
    _lib.call("mgb_fem3d_native", 1, 1, C.byref(h3))
    z3 = np.zeros(8)
    assert lib.mgb_geo_level_sets_host(h3, 1, (_lib.c_dbl_p * 1)(_lib.dptr(z3)), 1, 0, 1, _lib.dptr(lv), 0, _lib.dptr(rows), cp, None, None, None, 0) == LU.MGB_E_ARG
    assert b"3-D" in lib.mgb_last_error()
    _lib.call("mgb_geo_destroy", h3)


def test_python_names():
    import mgb_amd as M
    assert {"level_sets", "LevelSets"} <= set(M.__all__)
