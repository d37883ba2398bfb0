"""CPU tests of the boundary facets (csrc/boundary.hpp: build_facets, through M.boundary and mgb_geo_boundary_get) and of the
host restatement mgb_geo_boundary_flux_host (the per-node routine the gfx950 kernels also run) against the numpy yardstick
tests/boundary_reference.py and against known answers: counts, measures and the divergence theorem on fields the elements hold
exactly.  Shapes: those of test_gpu_boundary.py.

Bars (tests/boundary_reference.py): a sum within KTOL = 1e-12 times its absolute sum, a maximum within KTOL relative; facet
tables within KTOL relative to the size of the domain (indices exactly)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import boundary_reference as BR
import energy_reference as ER

MGB_E_ARG = -1
KTOL = BR.KTOL


@pytest.fixture(scope="module", params=list(BR.SHAPES))
def geo(request, lib):
    g = BR.HostMesh(request.param)
    yield g
    g.close()


def _fields(g, B, seed):
    """B distinct random (n, 3) fields, broken across elements: a wrong element, row, stride or column shows."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((g.n, 3)) for _ in range(B)]


def _exact(lib, g, u, p=2.0, mask=None):
    """Host results and the yardstick's absolute sums for the single column u."""
    out, fac = BR.host_boundary_flux(lib, g, [u.reshape(-1, 1)], p, mask=mask)
    _, sums, _, _ = BR.boundary_flux(g.ops, g.F, u, p, mask)
    return out[0], sums, fac[0]


def test_facets_against_numpy(lib, geo):
    import mgb_amd as M
    b = M.boundary(geo.py)
    assert M.boundary(geo.py) is b and len(b) == geo.nf                   # kept on the geometry
    assert b.nodes.shape == (geo.nf, geo.q) and b.nodes.size == BR.SHAPES[geo.name][4]
    assert np.array_equal(b.element, geo.F["element"]) and np.array_equal(b.nodes, geo.F["nodes"])
    assert (np.diff(b.element) >= 0).all()
    for key in ("weights", "normal", "measure", "centre"):
        gap = np.abs(getattr(b, key) - geo.F[key]).max()
        print("%s: %s off the yardstick by %.3e" % (geo.name, key, gap))
        assert getattr(b, key).shape == geo.F[key].shape and gap <= KTOL
    want = {1: 2.0, 2: 8.0, 3: 24.0}[geo.dim]                             # |boundary| of [-1, 1]^dim and of the L shape
    assert abs(b.measure.sum() - want) <= KTOL * want and abs(b.weights.sum() - want) <= KTOL * want
    assert np.abs(np.sqrt((b.normal ** 2).sum(axis=1)) - 1.0).max() <= KTOL
    assert (b.element == b.nodes[:, 0] // geo.block).all() and (b.element == b.nodes[:, -1] // geo.block).all()
    centre_e = np.array([geo.x[e * geo.block:(e + 1) * geo.block].mean(axis=0) for e in b.element])
    assert (((b.centre - centre_e) * b.normal).sum(axis=1) > 0).all()     # outward
    # the C entry point on the library's own geometry gives the same tables
    nf, q, dim = C.c_int(), C.c_int(), C.c_int()
    assert lib.mgb_geo_boundary_dims(geo.handle, C.byref(nf), C.byref(q), C.byref(dim)) == 0
    assert (nf.value, q.value, dim.value) == (geo.nf, geo.q, geo.dim)
    from mgb_amd import _lib
    el, nodes, w = np.empty(geo.nf, dtype=np.int32), np.empty((geo.nf, geo.q), dtype=np.int32), np.empty((geo.nf, geo.q))
    assert lib.mgb_geo_boundary_get(geo.handle, _lib.iptr(el), _lib.iptr(nodes), _lib.dptr(w), None, None, None) == 0
    assert np.array_equal(el, b.element) and np.array_equal(nodes, b.nodes) and np.array_equal(w, b.weights)


@pytest.mark.parametrize("L,count", [(1, 12), (2, 24), (3, 48)])
def test_counts_of_the_square(L, count):
    import mgb_amd as M
    b = M.boundary(M.fem2d(L))
    assert b.nodes.size == count == 3 * 2 ** (L + 1) and abs(b.measure.sum() - 8.0) <= 8.0 * KTOL


@pytest.mark.parametrize("p", ER.P_VALUES)
def test_host_against_numpy(lib, geo, p):
    pv = ER.exponent(p, geo.x)
    zs = _fields(geo, 3, 400)
    rng = np.random.default_rng(401)
    half = rng.random(geo.nf) < 0.5
    half[0] = True
    for u, mask in ((0, None), (2, half)):
        out, fac = BR.host_boundary_flux(lib, geo, zs, pv, u=u, mask=mask)
        for b in range(3):
            want, sums, pf, pfa = BR.boundary_flux(geo.ops, geo.F, zs[b][:, u], pv, mask)
            name = "%s p=%s u=%d field %d%s" % (geo.name, p, u, b, "" if mask is None else " masked")
            BR.check(name, out[b], want, sums)
            BR.check_facets(name, fac[b], pf, pfa)
            if mask is not None:
                assert np.array_equal(fac[b][~mask], np.zeros((~mask).sum()))
            gap = abs(fac[b].sum() - out[b, 0])
            print("%s: per-facet values sum to the flux within %.3e (bar %.3e)" % (name, gap, KTOL * sums[0]))
            assert gap <= KTOL * sums[0]
        one, fac1 = BR.host_boundary_flux(lib, geo, zs[1:2], pv, u=u, mask=mask)      # one field: the bits of the batch
        assert one[0].tobytes() == out[1].tobytes() and fac1[0].tobytes() == fac[1].tobytes()


def test_divergence_theorem_2d(lib):
    """p = 2, u = x^2 + y^2 / 2 + 0.3 x y is in P2 and its normal derivative is integrated exactly by Simpson: total flux
    int Laplace u = 3 |Omega| = 12 at every level; through the left, right, top, bottom side 4, 4, 2, 2; each side measures 2."""
    f = lambda x: x[:, 0] ** 2 + 0.5 * x[:, 1] ** 2 + 0.3 * x[:, 0] * x[:, 1]
    for L in (1, 2, 3):
        g = BR.HostMesh(kind="fem2d", L=L)
        try:
            u = f(g.x)
            out, sums, _ = _exact(lib, g, u)
            print("fem2d L=%d: flux %.17g (12), measure %.17g (8), bar %.3e" % (L, out[0], out[2], KTOL * sums[0]))
            assert abs(out[0] - 12.0) <= KTOL * sums[0] and abs(out[2] - 8.0) <= KTOL * 8.0
            c = g.F["centre"]
            sides = {"left": (c[:, 0] < -0.999, 4.0), "right": (c[:, 0] > 0.999, 4.0), "top": (c[:, 1] > 0.999, 2.0),
                     "bottom": (c[:, 1] < -0.999, 2.0)}
            for side, (mask, want) in sides.items():
                out, sums, fac = _exact(lib, g, u, mask=mask)
                print("fem2d L=%d %s: flux %.17g (%g), measure %.17g (2)" % (L, side, out[0], want, out[2]))
                assert abs(out[0] - want) <= KTOL * sums[0] and abs(out[2] - 2.0) <= KTOL * 2.0
        finally:
            g.close()


def test_divergence_theorem_on_the_l_shape(lib):
    g = BR.HostMesh("fem2d_L2_Lshape")
    try:
        u = g.x[:, 0] ** 2 + 0.5 * g.x[:, 1] ** 2 + 0.3 * g.x[:, 0] * g.x[:, 1]
        out, sums, _ = _exact(lib, g, u)
        print("L shape: area %.17g (3), flux %.17g (9), measure %.17g (8)" % (g.w.sum(), out[0], out[2]))
        assert abs(g.w.sum() - 3.0) <= 3.0 * KTOL
        assert abs(out[0] - 9.0) <= KTOL * sums[0] and abs(out[2] - 8.0) <= KTOL * 8.0
        # the two facets that meet at the re-entrant corner (0, 0) point into the missing quarter
        c, n = g.F["centre"], g.F["normal"]
        at_corner = (np.abs(c).min(axis=1) < 1e-12) & (np.abs(c).max(axis=1) < 0.5 + 1e-12) & (c.min(axis=1) > -1e-12)
        assert at_corner.sum() == 2 and (n[at_corner].sum(axis=1) > 0.999).all()
    finally:
        g.close()


@pytest.mark.parametrize("L,k", [(1, 2), (2, 2), (1, 3), (2, 3)])
def test_divergence_theorem_3d(lib, L, k):
    """u = x^2 + y^2 / 2 - z^2 / 4 + x y z is in Q_k for k >= 2: flux int Laplace u = 2.5 * 8 = 20."""
    g = BR.HostMesh(kind="fem3d", L=L, k=k)
    try:
        x, y, z = g.x.T
        out, sums, _ = _exact(lib, g, x ** 2 + 0.5 * y ** 2 - 0.25 * z ** 2 + x * y * z)
        print("fem3d L=%d k=%d: flux %.17g (20), measure %.17g (24), bar %.3e" % (L, k, out[0], out[2], KTOL * sums[0]))
        assert abs(out[0] - 20.0) <= KTOL * sums[0] and abs(out[2] - 24.0) <= KTOL * 24.0
    finally:
        g.close()


def test_harmonic_fields_have_no_net_flux(lib):
    """3-D k = 1, u = x y + z and 1-D, u = 1.5 x: flux 0 while sum omega |sigma . n| > 0."""
    for g, f in ((BR.HostMesh("fem3d_L2_k1"), lambda x: x[:, 0] * x[:, 1] + x[:, 2]), (BR.HostMesh("fem1d_L2"), lambda x: 1.5 * x[:, 0])):
        try:
            out, sums, _ = _exact(lib, g, f(g.x))
            print("%s: flux %.3e, sum omega |sigma . n| %.17g" % (g.name, out[0], sums[0]))
            assert sums[0] > 1.0 and abs(out[0]) <= KTOL * sums[0]
        finally:
            g.close()


def test_selection_and_non_finite_input(lib, geo):
    zs = _fields(geo, 3, 410)
    pn = ER.exponent("array", geo.x)
    clean, clean_fac = BR.host_boundary_flux(lib, geo, zs, pn)
    none, none_fac = BR.host_boundary_flux(lib, geo, zs, pn, mask=np.zeros(geo.nf, dtype=bool))
    assert np.array_equal(none, np.zeros((3, 5))) and np.array_equal(none_fac, np.zeros((3, geo.nf)))      # an empty selection
    every, _ = BR.host_boundary_flux(lib, geo, zs, pn, mask=np.ones(geo.nf, dtype=bool))
    assert every.tobytes() == clean.tobytes()
    last = geo.F["nodes"][-1, -1]
    for bad in (np.nan, np.inf, -np.inf):
        broken = [z.copy() for z in zs]
        broken[1][last, 0] = bad
        out, fac = BR.host_boundary_flux(lib, geo, broken, pn)
        assert np.isnan(out[1]).all() and np.isnan(fac[1, -1])
        assert out[0].tobytes() == clean[0].tobytes() and out[2].tobytes() == clean[2].tobytes()
        without = np.ones(geo.nf, dtype=bool)
        without[geo.F["element"] == geo.F["element"][-1]] = False         # the facets of that element left out: nothing is seen
        out, _ = BR.host_boundary_flux(lib, geo, broken, pn, mask=without)
        ref, _ = BR.host_boundary_flux(lib, geo, zs, pn, mask=without)
        assert np.isfinite(out).all() and out.tobytes() == ref.tobytes()
    other = [z.copy() for z in zs]
    other[1][last, 1] = np.nan                                            # another column
    interior = np.setdiff1d(np.arange(geo.n // geo.block), geo.F["element"])
    print("%s: %d elements without a boundary facet" % (geo.name, len(interior)))
    if len(interior):
        other[1][interior[0] * geo.block, 0] = np.nan                     # a node of an element that has no boundary facet
    out, fac = BR.host_boundary_flux(lib, geo, other, pn)
    assert out.tobytes() == clean.tobytes() and fac.tobytes() == clean_fac.tobytes()
    for bad in (0.5, np.nan, np.inf):                                     # the exponent at a selected node
        pb = pn.copy()
        pb[last] = bad
        out, _ = BR.host_boundary_flux(lib, geo, zs, pb)
        assert np.isnan(out).all()


def test_hand_made_geometries_in_either_orientation():
    """M.boundary on native geometries made by hand: a 1-D element and a Q1 box whose first row is the UPPER corner, and a
    clockwise triangle.  Normals point outward, measures are those of the sides."""
    import mgb_amd as M
    eye = lambda n: [sp.identity(n, format="csr")]
    geo = lambda x, block: M.Geometry(dict(kind="hand", L=1, dim=x.shape[1], block=block), x, np.ones(len(x)), {"full": eye(len(x))},
                                      {}, eye(len(x)), eye(len(x)))
    b = M.boundary(geo(np.array([[1.0], [-1.0]]), 2))
    assert np.array_equal(b.normal, [[1.0], [-1.0]]) and np.array_equal(b.nodes, [[0], [1]]) and np.array_equal(b.measure, [1.0, 1.0])
    lo, hi = np.array([1.0, -1.0, 2.0]), np.array([-1.0, 1.0, -1.0])
    x = np.array([[lo[d] + (hi[d] - lo[d]) * idx for d, idx in enumerate((i, j, m))] for m in (0, 1) for j in (0, 1) for i in (0, 1)])
    b = M.boundary(geo(x, 8))
    assert len(b) == 6 and np.array_equal(b.normal, [[1, 0, 0], [-1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]])
    assert np.allclose(b.measure, [6, 6, 6, 6, 4, 4], rtol=KTOL) and np.allclose(b.weights.sum(axis=1), b.measure, rtol=KTOL)
    assert np.allclose(b.centre, [[1, 0, .5], [-1, 0, .5], [0, -1, .5], [0, 1, .5], [0, 0, 2], [0, 0, -1]], atol=KTOL)
    v = np.array([[0.0, 0.0], [0.0, 3.0], [4.0, 0.0]])                    # clockwise
    x = np.vstack([v, (v + np.roll(v, -1, axis=0)) / 2, v.mean(axis=0)])
    b = M.boundary(geo(x, 7))
    assert np.allclose(b.measure, [3, 5, 4], rtol=KTOL) and np.allclose(b.normal, [[-1, 0], [0.6, 0.8], [0, -1]], atol=KTOL)
    assert np.array_equal(b.nodes, [[0, 3, 1], [1, 4, 2], [2, 5, 0]]) and np.allclose(b.weights[1], [5 / 6, 20 / 6, 5 / 6], rtol=KTOL)


def _hand_geo(lib, x, block, full):
    """A host mgb_geo of one level from x and an optional finest full subspace (scipy)."""
    from mgb_amd import _lib
    x = _lib.f64(x)
    h = C.c_void_p()
    _lib.call("mgb_geo_create", x.shape[0], x.shape[1], 1, block, _lib.dptr(x), _lib.dptr(np.ones(len(x))), C.byref(h))
    if full is not None:
        S = sp.csr_matrix(full, dtype=np.float64)
        S.sort_indices()
        rp, ci, va = _lib.i32(S.indptr), _lib.i32(S.indices), _lib.f64(S.data)
        _lib.call("mgb_geo_set_matrix", h, b"sub:full:0", S.shape[0], S.shape[1], _lib.iptr(rp), _lib.iptr(ci), _lib.dptr(va))
    return h


def test_geometries_that_are_refused(lib):
    from mgb_amd import _lib
    import mgb_amd as M
    dims = lambda h: lib.mgb_geo_boundary_dims(h, None, None, None)
    x = np.array([[-1.0], [0.0], [0.0], [1.0]])
    dofs = lambda cols, m: sp.csr_matrix((np.ones(len(cols)), (np.arange(len(cols)), cols)), shape=(len(cols), m))
    cases = {"fine": (x, dofs([0, 1, 1, 2], 3), 0), "no full subspace": (x, None, MGB_E_ARG),
             "two entries in a row": (x, sp.csr_matrix(np.array([[1, 0, 0], [0, 1, 1], [0, 1, 0], [0, 0, 1.0]])), MGB_E_ARG),
             "an entry that is not 1": (x, dofs([0, 1, 1, 2], 3) * 0.5, MGB_E_ARG),
             "too few rows": (x, dofs([0, 1, 1], 3), MGB_E_ARG),
             "three elements at one dof": (np.array([[-1.0], [0.0], [0.0], [1.0], [0.0], [0.5]]), dofs([0, 1, 1, 2, 1, 3], 4), MGB_E_ARG)}
    for name, (xx, full, want) in cases.items():
        h = _hand_geo(lib, xx, 2, full)
        try:
            rc = dims(h)
            print("%s: status %d %s" % (name, rc, lib.mgb_last_error() if rc else b""))
            assert rc == want, name
            if name == "three elements at one dof":
                assert b"non-manifold" in lib.mgb_last_error()
                assert lib.mgb_geo_boundary_get(h, None, None, None, None, None, None) == MGB_E_ARG
        finally:
            _lib.call("mgb_geo_destroy", h)
    eye = [sp.identity(4, format="csr")]
    with pytest.raises(M.MGBError, match="full subspace"):
        M.boundary(M.Geometry(dict(kind="hand", L=1, dim=1, block=2), x, np.ones(4), {}, {}, eye, eye))


def test_argument_errors(lib, geo):
    from mgb_amd import _lib
    z = np.zeros((geo.n, 2))
    H = lambda **kw: BR.host_boundary_flux(lib, geo, [z], kw.pop("p", 2.0), rc_only=True, **kw)
    assert H() == 0
    for p in (0.5, np.nan, np.inf, -2.0):
        assert H(p=p) == MGB_E_ARG
    assert H(u=2) == MGB_E_ARG and H(u=-1) == MGB_E_ARG and H(u=1) == 0
    assert H(B=0) == MGB_E_ARG and H(B=-3) == MGB_E_ARG
    assert H(S=0) == MGB_E_ARG
    out = np.zeros((1, 5))
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z))
    null = (_lib.c_dbl_p * 1)(None)
    F = lib.mgb_geo_boundary_flux_host
    assert F(None, 1, table, 2, 0, 2.0, None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert F(geo.handle, 1, None, 2, 0, 2.0, None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert F(geo.handle, 1, null, 2, 0, 2.0, None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert F(geo.handle, 1, table, 2, 0, 2.0, None, None, None, None) == MGB_E_ARG
    assert F(geo.handle, 1, table, 2, 0, 2.0, None, None, None, _lib.dptr(out)) == 0      # mask and per-facet output may be null
    assert lib.mgb_geo_boundary_dims(None, None, None, None) == MGB_E_ARG
    assert lib.mgb_geo_boundary_get(None, None, None, None, None, None, None) == MGB_E_ARG
    h = C.c_void_p()
    assert lib.mgb_boundary_create(None, geo.handle, C.byref(h)) == MGB_E_ARG and lib.mgb_boundary_create(None, None, None) == MGB_E_ARG
    assert lib.mgb_boundary_dims(None, None, None, None) == MGB_E_ARG
    assert lib.mgb_boundary_get(None, None, None, None, None, None, None) == MGB_E_ARG
    assert lib.mgb_boundary_flux(None, 1, None, 2, 0, 2.0, None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert lib.mgb_boundary_destroy(None) == 0


def test_python_surface_rejects_what_it_cannot_take():
    import mgb_amd as M
    g = M.fem2d(2)
    z = np.zeros((g.x.shape[0], 2))
    with pytest.raises(TypeError, match="geometry"):
        M.boundary_flux(g, 2.0, z=z)                                      # a native geometry has no device locator
    with pytest.raises(TypeError):
        M.boundary_flux(np.zeros(3), 2.0)
    with pytest.raises(TypeError, match="Geometry"):
        M.boundary(np.zeros(3))
    b = M.boundary(g)
    assert M._boundary_selection(None, b, "boundary_flux") is None
    m = M._boundary_selection(lambda c: c[0] > 0.999, b, "boundary_flux")
    assert m.dtype == np.uint8 and m.shape == (len(b),) and m.sum() == 2
    assert np.array_equal(M._boundary_selection(b.centre[:, 0] > 0.999, b, "boundary_flux"), m)
    for bad in (np.ones(len(b)), np.ones(len(b) + 1, dtype=bool), np.ones((len(b), 1), dtype=bool), 1):
        with pytest.raises(ValueError, match="where"):
            M._boundary_selection(bad, b, "boundary_flux")
    r = M.BoundaryFlux(1.0, 2.0, 3.0, 0.5, 0.25)
    assert M.mpi_to_native(r) is r and r.ts is None and r.facets is None  # host data already: passed through
    assert {"boundary", "boundary_flux", "Boundary", "BoundaryFlux"} <= set(M.__all__)
