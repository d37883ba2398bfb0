"""CPU tests of the host restatement mgb_geo_sections_host (csrc/section.hpp: the per-item routine the gfx950 kernels also
run) against the numpy yardstick tests/section_reference.py, plus non-finite nodes, the exponents and the argument errors.

Bars (tests/section_reference.py, tests/section_util.py): counts, items and row offsets equal; every vertex within
8 eps (|P_hi - P_lo|_inf + max|x|); every vertex value and both maxima within the value bar
32 eps S + 8 eps (max|x| / h + 1) G + 2 |grad u|_1 dy; the three sums within 1e-12 of the sum of their absolute terms.
Largest ratios measured: vertices 0.033, vertex values 0.006, sums 6.7e-4, maxima 0.004."""
import ctypes as C

import numpy as np
import pytest

import section_util as SU

PLANES2, PLANES3, smooth = SU.PLANES2, SU.PLANES3, SU.smooth


@pytest.mark.parametrize("dim,L,k", [(2, 1, 0), (2, 4, 0), (3, 1, 1), (3, 2, 3), (3, 3, 2)])
def test_host_against_numpy(lib, dim, L, k):
    g = SU.host_mesh(dim, L, k)
    z = np.stack([np.zeros(g.n), smooth(g.x)], axis=1)      # column 1 of 2: a wrong stride shows
    planes = PLANES2 if dim == 2 else PLANES3
    name = "fem%dd L=%d k=%d" % (dim, L, k)
    got = SU.host_sections(lib, g, [z], planes, u=1)
    SU.against_reference(name, got, g, [z], planes, u=1, keys=["host " + name])
    assert got.rows.shape == (1, 7, 5) and len(got.piece) == got.offsets[-1]
    assert (got.counts[0, :4] > 0).all() and (got.counts[0, 5:] == 0).all()
    # x = -1 with n pointing outwards: every corner is below or on the plane, nothing is above it
    assert got.counts[0, 4] == 0
    # the faces in a plane: exact measure from the pieces, each piece once
    piece, item = got.row(0, 2)
    per = 6 if dim == 3 else 1
    block = g.block
    centre = g.x.reshape(-1, block, dim).mean(axis=1)
    if L > 1:      # at L = 1 the plane x = 0 passes through the inside of the elements
        assert SU.piece_measure(piece, dim).sum() == (4 if dim == 3 else 2) and (centre[item // per, 0] > 0).all()


@pytest.mark.parametrize("dim,L,k", [(2, 3, 0), (3, 2, 2)])
def test_boundary_face_from_inside(lib, dim, L, k):
    """x = -1 with n = e_x: the boundary face is cut by the elements inside; x = 1: nothing is above."""
    g = SU.host_mesh(dim, L, k)
    z = g.x[:, 0] + 2.0
    planes = [[1.0] + [0.0] * (dim - 1) + [-1.0], [1.0] + [0.0] * (dim - 1) + [1.0]]
    got = SU.host_sections(lib, g, [z], planes)
    SU.against_reference("boundary faces %d-D" % dim, got, g, [z], planes)
    full = 4.0 if dim == 3 else 2.0
    assert SU.piece_measure(got.row(0, 0)[0], dim).sum() == full and abs(got.rows[0, 0, 0] - full) <= 1e-12 * full
    assert abs(got.rows[0, 0, 1] - full) <= 1e-12 * full and abs(got.rows[0, 0, 2] - full) <= 1e-12 * full      # u = 1, grad = e_x
    assert got.counts[0, 1] == 0 and np.array_equal(got.rows[0, 1], [0.0, 0.0, 0.0, -np.inf, -np.inf])


@pytest.mark.parametrize("dim,L,k", [(2, 3, 0), (3, 2, 3), (3, 2, 1)])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_nodes(lib, dim, L, k, bad):
    g = SU.host_mesh(dim, L, k)
    planes = [[1.0, 0.0, 0.3], [0.0, 1.0, -0.4]] if dim == 2 else [[0.0, 0.0, 1.0, 0.3], [1.0, 0.0, 0.0, -0.4]]
    per = 6 if dim == 3 else 1
    z = smooth(g.x)
    clean = SU.host_sections(lib, g, [z, z + 0.1], planes)
    cut = np.unique(clean.row(0, 0)[1] // per)
    both = np.union1d(cut, np.unique(clean.row(0, 1)[1] // per))
    uncut = np.setdiff1d(np.arange(g.nel), both)
    assert len(cut) and len(uncut)
    # in an uncut element: not seen
    zu = z.copy()
    zu[uncut[0] * g.block + 1] = bad
    got = SU.host_sections(lib, g, [zu, z + 0.1], planes)
    assert got.rows.tobytes() == clean.rows.tobytes() and got.piece.tobytes() == clean.piece.tobytes()
    # in an element that plane 0 cuts and plane 1 does not: row (0, 0) is NaN and loses that element's pieces, nothing else moves
    only0 = np.setdiff1d(cut, np.unique(clean.row(0, 1)[1] // per))
    assert len(only0)
    e = int(only0[0])
    zb = z.copy()
    zb[e * g.block + g.block - 1] = bad
    got = SU.host_sections(lib, g, [zb, z + 0.1], planes)
    SU.against_reference("non-finite node %d-D k=%d" % (dim, k), got, g, [zb, z + 0.1], planes)
    assert np.isnan(got.rows[0, 0]).all() and got.rows[0, 1].tobytes() == clean.rows[0, 1].tobytes()
    assert got.rows[1].tobytes() == clean.rows[1].tobytes() and np.array_equal(got.counts[1], clean.counts[1])
    piece, item = got.row(0, 0)
    cpiece, citem = clean.row(0, 0)
    keep = citem // per != e
    assert (~keep).any() and np.array_equal(item, citem[keep]) and piece.tobytes() == cpiece[keep].tobytes()
    for b, l in ((0, 1), (1, 0), (1, 1)):
        assert got.row(b, l)[0].tobytes() == clean.row(b, l)[0].tobytes()


@pytest.mark.parametrize("dim,L,k", [(2, 3, 0), (3, 2, 2)])
@pytest.mark.parametrize("p", [1.0, 1.5, 2.0])
def test_exponents(lib, dim, L, k, p):
    g = SU.host_mesh(dim, L, k)
    z = smooth(g.x)
    planes = (PLANES2 if dim == 2 else PLANES3)[:3]
    got = SU.host_sections(lib, g, [z], planes, p=p)
    SU.against_reference("p=%g %d-D" % (p, dim), got, g, [z], planes, p=p)
    two = SU.host_sections(lib, g, [z], planes, p=2.0)
    cols = [0, 1, 3, 4]
    assert got.rows[:, :, cols].tobytes() == two.rows[:, :, cols].tobytes() and got.piece.tobytes() == two.piece.tobytes()
    if p == 1.0:      # |sigma| = 1: the flow rate is at most the measure
        assert (np.abs(got.rows[0, :, 2]) <= got.rows[0, :, 0]).all()
    # the zero field has no flux at any p, also where |g|^(p-2) is singular: sigma is exactly 0 where g = 0
    flat = SU.host_sections(lib, g, [np.zeros(g.n)], planes, p=p)
    assert (flat.rows[0, :, 1:] == 0.0).all() and flat.rows[0, :, 0].tobytes() == two.rows[0, :, 0].tobytes()


def test_rows_do_not_depend_on_the_batch(lib):
    g = SU.host_mesh(3, 2, 3)
    rng = np.random.default_rng(3)
    fields = [smooth(g.x), rng.standard_normal(g.n)]      # the second one broken across the elements
    got = SU.host_sections(lib, g, fields, PLANES3)
    SU.against_reference("two fields", got, g, fields, PLANES3)
    for b in range(2):
        for l in (0, 1, 3, 6):
            one = SU.host_sections(lib, g, [fields[b]], [PLANES3[l]])
            assert one.rows[0, 0].tobytes() == got.rows[b, l].tobytes() and one.piece.tobytes() == got.row(b, l)[0].tobytes()
    # wedges: items with two triangles, adjacent and in ascending item order
    item = got.row(0, 1)[1]
    assert (item[1:] == item[:-1]).any() and (np.diff(item) >= 0).all()


def test_argument_errors(lib):
    from mgb_amd import _lib
    import levelset_util as LU
    g3, g2, g1 = SU.host_mesh(3, 2, 1), SU.host_mesh(2, 2), LU.host_mesh("fem1d", 3)
    z3 = np.zeros((g3.n, 2))
    ok = dict(planes=[PLANES3[1]], rc_only=True)
    assert SU.host_sections(lib, g3, [z3], **ok) == 0
    assert SU.host_sections(lib, g2, [np.zeros(g2.n)], planes=[PLANES2[1]], rc_only=True) == 0
    for kw, msg in ((dict(B=0), b"B must be >= 1"), (dict(nc=0), b"nc must be >= 1"), (dict(S=0), b"S must be >= 1"),
                    (dict(u=2), b"column u outside"), (dict(u=-1), b"column u outside"),
                    (dict(p=0.5), b"p must be one finite real >= 1"), (dict(p=np.nan), b"p must be one finite real >= 1"),
                    (dict(p=np.inf), b"p must be one finite real >= 1"),
                    (dict(planes=[[0.0, 0.0, 0.0, 0.1]]), b"normal of every plane must be finite and not zero"),
                    (dict(planes=[PLANES3[0], [np.nan, 0.0, 1.0, 0.1]]), b"normal of every plane must be finite and not zero"),
                    (dict(planes=[[np.inf, 0.0, 1.0, 0.1]]), b"normal of every plane must be finite and not zero"),
                    (dict(planes=[[1e200, 1e200, 0.0, 0.1]]), b"finite, positive length"),
                    (dict(planes=[[0.0, 0.0, 1.0, np.inf]]), b"offset c of every plane must be finite"),
                    (dict(planes=[[0.0, 0.0, 1.0, np.nan]]), b"offset c of every plane must be finite"),
                    (dict(B=65536, nc=32768), b"more than INT_MAX rows")):
        assert SU.host_sections(lib, g3, [z3], **{**ok, **kw}) == SU.MGB_E_ARG, kw
        err = lib.mgb_last_error()
        assert b"geo_sections_host" in err and msg in err, (kw, err)
    rows, counts = np.empty(5), np.empty(1, dtype=np.int64)
    cp = counts.ctypes.data_as(_lib.c_ll_p)
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z3))
    pl = np.array(PLANES3[1])
    call = lambda h, t, l, r, c: lib.mgb_geo_sections_host(h, 1, t, 2, 0, 1, l, 2.0, r, c, None, None, None, 0)
    assert call(g3.handle, table, _lib.dptr(pl), _lib.dptr(rows), cp) == 0
    for args in ((None, table, _lib.dptr(pl), _lib.dptr(rows), cp), (g3.handle, None, _lib.dptr(pl), _lib.dptr(rows), cp),
                 (g3.handle, table, None, _lib.dptr(rows), cp), (g3.handle, table, _lib.dptr(pl), None, cp),
                 (g3.handle, table, _lib.dptr(pl), _lib.dptr(rows), None)):
        assert call(*args) == SU.MGB_E_ARG and b"null argument" in lib.mgb_last_error()
    assert call(g3.handle, (_lib.c_dbl_p * 1)(None), _lib.dptr(pl), _lib.dptr(rows), cp) == SU.MGB_E_ARG
    assert b"null field" in lib.mgb_last_error()
    # pieces without items, and arrays that are too small
    piece, item = np.empty((1, 12)), np.empty(1, dtype=np.int32)
    z = smooth(g3.x)
    t1 = (_lib.c_dbl_p * 1)(_lib.dptr(z))
    host = lambda pp, ip, cap: lib.mgb_geo_sections_host(g3.handle, 1, t1, 1, 0, 1, _lib.dptr(pl), 2.0, _lib.dptr(rows), cp, None, pp, ip, cap)
    assert host(_lib.dptr(piece), None, 1) == SU.MGB_E_ARG and b"come together" in lib.mgb_last_error()
    assert host(_lib.dptr(piece), _lib.iptr(item), -1) == SU.MGB_E_ARG and b"negative capacity" in lib.mgb_last_error()
    assert host(_lib.dptr(piece), _lib.iptr(item), 1) == SU.MGB_E_ARG and b"more pieces than the arrays hold" in lib.mgb_last_error()
    # a 1-D geometry: the value at a point is interpolate's
    z1 = np.zeros(g1.n)
    p1 = np.array([1.0, 0.1])
    assert lib.mgb_geo_sections_host(g1.handle, 1, (_lib.c_dbl_p * 1)(_lib.dptr(z1)), 1, 0, 1, _lib.dptr(p1), 2.0, _lib.dptr(rows), cp,
                                     None, None, None, 0) == SU.MGB_E_ARG
    assert b"interpolate" in lib.mgb_last_error()


def custom_geo(lib, x, block):
    from mgb_amd import _lib
    x = _lib.f64(x)
    w = np.ones(x.shape[0])
    h = C.c_void_p()
    assert lib.mgb_geo_create(x.shape[0], x.shape[1], 1, block, _lib.dptr(x), _lib.dptr(w), C.byref(h)) == 0
    return h


@pytest.mark.parametrize("m1", [5, 1])
def test_elements_outside_k_1_to_3_are_refused(lib, m1):
    """One axis-aligned box with m1^3 equispaced tensor nodes: degree 4 (block 125) and degree 0 (block 1).  Only
    (k+1)^3, k = 1..3, exists; the locator names the rule when it refuses the block, before anything is cut."""
    from mgb_amd import _lib
    t = np.linspace(-1.0, 1.0, m1) if m1 > 1 else np.zeros(1)
    zc, yc, xc = np.meshgrid(t, t, t, indexing="ij")
    x = np.stack([xc.ravel(), yc.ravel(), zc.ravel()], axis=1)      # x fastest
    h = custom_geo(lib, x, m1 ** 3)
    z = np.zeros(len(x))
    rows, counts, pl = np.full(5, 7.0), np.full(1, -7, dtype=np.int64), np.array(PLANES3[1])
    rc = lib.mgb_geo_sections_host(h, 1, (_lib.c_dbl_p * 1)(_lib.dptr(z)), 1, 0, 1, _lib.dptr(pl), 2.0, _lib.dptr(rows),
                                   counts.ctypes.data_as(_lib.c_ll_p), None, None, None, 0)
    err = lib.mgb_last_error()
    assert lib.mgb_geo_destroy(h) == 0
    assert rc == SU.MGB_E_ARG and b"k = 1..3" in err, (rc, err)
    assert (rows == 7.0).all() and counts[0] == -7      # nothing was written


def test_a_box_of_degree_2_made_by_hand_is_cut(lib):
    """The same construction with 27 nodes is accepted: the refusal above is about the block, not about mgb_geo_create."""
    from mgb_amd import _lib
    t = np.linspace(-1.0, 1.0, 3)
    zc, yc, xc = np.meshgrid(t, t, t, indexing="ij")
    x = np.stack([xc.ravel(), yc.ravel(), zc.ravel()], axis=1)
    h = custom_geo(lib, x, 27)
    z = np.ones(27)
    rows, counts, pl = np.full(5, 7.0), np.full(1, -7, dtype=np.int64), np.array(PLANES3[0])
    rc = lib.mgb_geo_sections_host(h, 1, (_lib.c_dbl_p * 1)(_lib.dptr(z)), 1, 0, 1, _lib.dptr(pl), 2.0, _lib.dptr(rows),
                                   counts.ctypes.data_as(_lib.c_ll_p), None, None, None, 0)
    assert lib.mgb_geo_destroy(h) == 0
    assert rc == 0 and abs(rows[0] - 4.0) <= 1e-12 * 4.0 and abs(rows[1] - 4.0) <= 1e-12 * 4.0 and counts[0] > 0


def test_python_names():
    import mgb_amd as M
    assert {"sections", "Sections"} <= set(M.__all__)
