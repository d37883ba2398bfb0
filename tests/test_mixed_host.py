"""CPU tests of mixed boundary conditions: the Dirichlet subspace on part of the boundary
(csrc/mixed.hpp through M.dirichlet_on and mgb_geo_dirichlet_on), the incidence table and the host restatement of the Neumann
load (csrc/boundary.hpp: load_row, the routine the gfx950 kernel also runs, through mgb_geo_boundary_load_host) against the
numpy / fsum yardstick tests/mixed_reference.py, and the argument errors that need no GPU.

Bars: subspace matrices bitwise on values and equal in pattern after dropping stored zeros; a load row within KTOL = 1e-12 of its
own absolute sum  sum omega |h| / w  (the bar of test_boundary_host.py)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import boundary_reference as BR
import mixed_reference as MR

MGB_E_ARG = -1
KTOL = MR.KTOL

GEOMETRIES = {"fem1d_L2": ("fem1d", 2, None, None), "fem1d_L3": ("fem1d", 3, None, None), "fem2d_L2": ("fem2d", 2, None, None),
              "fem2d_L3": ("fem2d", 3, None, None), "fem2d_L2_Lshape": ("fem2d", 2, None, BR.L_SHAPE),
              "fem3d_L1_k1": ("fem3d", 1, 1, None), "fem3d_L1_k2": ("fem3d", 1, 2, None), "fem3d_L1_k3": ("fem3d", 1, 3, None),
              "fem3d_L2_k1": ("fem3d", 2, 1, None), "fem3d_L2_k2": ("fem3d", 2, 2, None), "fem3d_L2_k3": ("fem3d", 2, 3, None)}


def native(name):
    import mgb_amd as M
    kind, L, k, K = GEOMETRIES[name]
    return M.fem1d(L) if kind == "fem1d" else M.fem2d(L, K) if kind == "fem2d" else M.fem3d(L, k)


def selections(F):
    c = F["centre"]
    lo, hi = c[:, 0].min(), c[:, 0].max()
    one = np.zeros(len(c), dtype=bool)
    one[len(c) // 2] = True
    return {"one_side": c[:, 0] < lo + 1e-9, "two_sides": (c[:, 0] < lo + 1e-9) | (c[:, 0] > hi - 1e-9), "one_facet": one}


@pytest.fixture(scope="module", params=list(GEOMETRIES))
def geo(request, lib):
    g = native(request.param)
    return request.param, g, BR.facets(g)


def test_subspaces_against_the_column_rule(geo):
    import mgb_amd as M
    name, g, F = geo
    L = len(g.refine)
    for tag, sel in selections(F).items():
        got = M.dirichlet_on(g, sel, tag)
        assert got == tag and len(g.subspaces[tag]) == L
        want = MR.mixed_subspaces(g, sel, F)
        rows = MR.pinned_rows(F, sel)
        print("%s %s: %d pinned rows, columns per level %s of %s" % (name, tag, len(rows), [S.shape[1] for S in g.subspaces[tag]],
                                                                     [S.shape[1] for S in g.subspaces["full"]]))
        for l in range(L):
            S = g.subspaces[tag][l]
            assert MR.same_matrix(S, want[l]), (name, tag, l)
            assert S[rows].count_nonzero() == 0                          # every kept column vanishes on the selected rows
        full = sp.csr_matrix(g.subspaces["full"][L - 1])
        touched = np.unique(full[rows].indices[full[rows].data != 0.0])  # the columns the selected rows touch: exactly the pinned ones
        kept = np.setdiff1d(np.arange(full.shape[1]), touched)
        assert g.subspaces[tag][L - 1].shape[1] == len(kept) and MR.same_matrix(g.subspaces[tag][L - 1], full[:, kept])
    # a callable on the facet centre selects the same facets as the array
    lo = F["centre"][:, 0].min()
    M.dirichlet_on(g, lambda c: c[0] < lo + 1e-9, "by_callable")
    assert all(MR.same_matrix(a, b) for a, b in zip(g.subspaces["by_callable"], g.subspaces["one_side"]))


def test_every_facet_is_dirichlet_and_none_is_full(geo):
    import mgb_amd as M
    name, g, F = geo
    nf = len(F["element"])
    M.dirichlet_on(g, np.ones(nf, dtype=bool), "every")
    M.dirichlet_on(g, np.zeros(nf, dtype=bool), "nothing")
    for l in range(len(g.refine)):
        assert g.subspaces["every"][l].shape == g.subspaces["dirichlet"][l].shape      # the empty coarsest level of k = 1 included
        assert MR.same_matrix(g.subspaces["every"][l], g.subspaces["dirichlet"][l]), (name, l)
        assert MR.same_matrix(g.subspaces["nothing"][l], g.subspaces["full"][l]), (name, l)


def test_counts_of_one_side():
    """The side x = min leaves 8 / 28 / 104 columns on fem2d L=3 and 48 / 294 on fem3d L=2 k=3."""
    import mgb_amd as M
    for g, want in ((M.fem2d(3), [8, 28, 104]), (M.fem3d(2, 3), [48, 294])):
        M.dirichlet_on(g, lambda c: c[0] < -0.999, "left")
        assert [S.shape[1] for S in g.subspaces["left"]] == want


def test_stored_zeros_stay_and_do_not_count(lib):
    """A stored zero in a pinned row does not drop its column, and a kept column keeps its stored zeros."""
    from mgb_amd import _lib
    x = np.array([[-1.0], [0.0], [0.0], [1.0]])
    full = sp.csr_matrix((np.array([1.0, 1.0, 1.0, 1.0]), (np.arange(4), [0, 1, 1, 2])), shape=(4, 3))
    coarse = sp.csr_matrix((np.array([1.0, 0.0, 0.5, 0.5, 0.5, 0.5, 0.0, 1.0]), ([0, 0, 1, 1, 2, 2, 3, 3], [0, 1, 0, 1, 0, 1, 0, 1])), shape=(4, 2))
    h = C.c_void_p()
    _lib.call("mgb_geo_create", 4, 1, 2, 2, _lib.dptr(_lib.f64(x)), _lib.dptr(np.ones(4)), C.byref(h))
    try:
        for l, S in ((0, coarse), (1, full)):
            rp, ci, va = _lib.i32(S.indptr), _lib.i32(S.indices), _lib.f64(S.data)
            _lib.call("mgb_geo_set_matrix", h, ("sub:full:%d" % l).encode(), 4, S.shape[1], _lib.iptr(rp), _lib.iptr(ci), _lib.dptr(va))
        mask = np.array([1, 0], dtype=np.uint8)                          # the facet at x = -1: row 0
        assert lib.mgb_geo_dirichlet_on(h, b"left", _lib.u8ptr(mask)) == 0
        import mgb_amd as M
        S0, S1 = M._geo_matrix(h, "sub:left:0"), M._geo_matrix(h, "sub:left:1")
        assert S0.shape == (4, 1) and np.array_equal(S0.indptr, [0, 1, 2, 3, 4]) and np.array_equal(S0.data, [0.0, 0.5, 0.5, 1.0])
        assert S1.shape == (4, 2) and np.array_equal(S1.toarray(), [[0, 0], [1, 0], [1, 0], [0, 1]])
    finally:
        _lib.call("mgb_geo_destroy", h)


# ------------------------------------------------------------------------------------------------------------ Neumann load
def host_load(lib, handle, nb, fields, mask=None):
    from mgb_amd import _lib
    hv = _lib.f64(fields)
    B = hv.shape[0]
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    out = np.full((B, nb), 7.0)                                           # prefilled: an unwritten word shows
    assert lib.mgb_geo_boundary_load_host(handle, B, _lib.dptr(hv), _lib.u8ptr(m), _lib.dptr(out)) == 0, lib.mgb_last_error()
    return out


def host_incidence(lib, handle):
    from mgb_amd import _lib
    nb, ninc = C.c_int(), C.c_int()
    assert lib.mgb_geo_boundary_incidence(handle, C.byref(nb), C.byref(ninc), None, None, None) == 0
    rows, start, idx = np.empty(nb.value, dtype=np.int32), np.empty(nb.value + 1, dtype=np.int32), np.empty(ninc.value, dtype=np.int32)
    assert lib.mgb_geo_boundary_incidence(handle, None, None, _lib.iptr(rows), _lib.iptr(start), _lib.iptr(idx)) == 0
    return rows, start, idx


def check_mesh(lib, name, handle, F, w, per_row, measure):
    nf, q = F["nodes"].shape
    rows, start, idx = host_incidence(lib, handle)
    r_ref, s_ref, i_ref = MR.incidence(F)
    assert np.array_equal(rows, r_ref) and np.array_equal(start, s_ref) and np.array_equal(idx, i_ref)
    assert (np.diff(rows) > 0).all() and start[0] == 0 and start[-1] == nf * q
    if per_row is not None:
        assert (np.diff(start) == per_row).all()
    nb = len(rows)
    rng = np.random.default_rng(7)
    fields = rng.standard_normal((3, nf, q))
    half = rng.random(nf) < 0.5
    half[0] = True
    for mask in (None, half):
        out = host_load(lib, handle, nb, fields, mask)
        for b in range(3):
            _, want, ab = MR.load(F, w, fields[b], mask)
            MR.check_load("%s field %d%s" % (name, b, "" if mask is None else " masked"), out[b], want, ab)
            assert np.array_equal(out[b][ab == 0.0], np.zeros((ab == 0.0).sum()))      # no selected incidence: exactly 0
        one = host_load(lib, handle, nb, fields[1:2], mask)
        assert one[0].tobytes() == out[1].tobytes()
    ones = host_load(lib, handle, nb, np.ones((1, nf, q)))[0]             # sum_r w_r l_r = int_Gamma 1 = the measure
    total = float(np.sum(w[rows] * ones))
    print("%s: sum w l for h = 1 is %.17g (%g)" % (name, total, measure))
    assert abs(total - measure) <= KTOL * measure
    dirty = fields.copy()
    dirty[:, ~half] = np.nan                                              # a masked-out NaN is not seen
    assert host_load(lib, handle, nb, dirty, half).tobytes() == host_load(lib, handle, nb, fields, half).tobytes()
    bad = host_load(lib, handle, nb, dirty)                               # ... an unmasked one is
    assert np.isnan(bad).any() == (not half.all())
    none = host_load(lib, handle, nb, fields, np.zeros(nf, dtype=bool))
    assert np.array_equal(none, np.zeros((3, nb)))


def test_load_on_a_hand_made_triangle(lib):
    """One P2 triangle with the bubble node: three boundary facets, every vertex row in two of them."""
    import mgb_amd as M
    from mgb_amd import _lib
    v = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 3.0]])
    x = np.vstack([v, (v + np.roll(v, -1, axis=0)) / 2, v.mean(axis=0)])
    w = np.array([0.3, 0.4, 0.5, 1.1, 1.2, 1.3, 1.2])
    eye = [sp.identity(7, format="csr")]
    g = M.Geometry(dict(kind="hand", L=1, dim=2, block=7), x, w, {"full": eye}, {}, eye, eye)
    F = BR.facets(g)
    assert F["nodes"].shape == (3, 3)
    h = C.c_void_p()
    _lib.call("mgb_geo_create", 7, 2, 1, 7, _lib.dptr(_lib.f64(x)), _lib.dptr(w), C.byref(h))
    try:
        S = eye[0]
        _lib.call("mgb_geo_set_matrix", h, b"sub:full:0", 7, 7, _lib.iptr(_lib.i32(S.indptr)), _lib.iptr(_lib.i32(S.indices)), _lib.dptr(_lib.f64(S.data)))
        rows, start, _ = host_incidence(lib, h)
        assert np.array_equal(rows, np.arange(6)) and np.array_equal(np.diff(start), [2, 2, 2, 1, 1, 1])
        check_mesh(lib, "triangle", h, F, w, None, 12.0)
    finally:
        _lib.call("mgb_geo_destroy", h)


@pytest.mark.parametrize("name,per_row,measure", [("fem1d_L2", 1, 2.0), ("fem2d_L2", None, 8.0), ("fem2d_L2_Lshape", None, 8.0),
                                                  ("fem3d_L1_k1", 3, 24.0), ("fem3d_L2_k3", None, 24.0)])
def test_load_against_fsum(lib, name, per_row, measure):
    kind, L, k, K = GEOMETRIES[name]
    g = BR.HostMesh(kind=kind, L=L, k=k, K=K)
    try:
        if name == "fem3d_L1_k1":
            assert g.n == 8 and g.nf == 6                                 # one cube: each corner row in three facets
        check_mesh(lib, name, g.handle, g.F, g.w, per_row, measure)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------------------ errors
def test_refused_names_and_geometries(lib):
    import mgb_amd as M
    from mgb_amd import _lib
    g = BR.HostMesh("fem2d_L2")
    try:
        for name in (b"full", b"dirichlet", b"fixed", b"", b"a:b"):
            assert lib.mgb_geo_dirichlet_on(g.handle, name, None) == MGB_E_ARG, name
        assert lib.mgb_geo_dirichlet_on(g.handle, None, None) == MGB_E_ARG and lib.mgb_geo_dirichlet_on(None, b"m", None) == MGB_E_ARG
        assert lib.mgb_geo_dirichlet_on(g.handle, b"m", None) == 0
        assert lib.mgb_geo_dirichlet_on(g.handle, b"m", None) == MGB_E_ARG and b"already" in lib.mgb_last_error()
        r, c, nz = C.c_int(), C.c_int(), C.c_int()
        for l in range(2):                                                # NULL mask = every facet = dirichlet
            assert lib.mgb_geo_matrix_info(g.handle, ("sub:m:%d" % l).encode(), C.byref(r), C.byref(c), C.byref(nz)) == 0
            assert MR.same_matrix(M._geo_matrix(g.handle, "sub:m:%d" % l), g.py.subspaces["dirichlet"][l])
        out = np.zeros((1, 16))
        hv = np.zeros((1, g.nf, g.q))
        L_ = lib.mgb_geo_boundary_load_host
        assert L_(None, 1, _lib.dptr(hv), None, _lib.dptr(out)) == MGB_E_ARG and L_(g.handle, 1, None, None, _lib.dptr(out)) == MGB_E_ARG
        assert L_(g.handle, 1, _lib.dptr(hv), None, None) == MGB_E_ARG and L_(g.handle, 0, _lib.dptr(hv), None, _lib.dptr(out)) == MGB_E_ARG
        assert lib.mgb_geo_boundary_incidence(None, None, None, None, None, None) == MGB_E_ARG
        assert lib.mgb_boundary_incidence(None, None, None, None, None, None) == MGB_E_ARG
        assert lib.mgb_boundary_load(None, 1, _lib.dptr(hv), None, None) == MGB_E_ARG
        assert lib.mgb_boundary_load_add(None, None, 0, 1.0, None, 1, 0) == MGB_E_ARG
        assert lib.mgb_amg_add_cost_rows(None, None, None, 0, 1.0, 0) == MGB_E_ARG
    finally:
        g.close()
    x = np.array([[-1.0], [0.0], [0.0], [1.0]])
    full = sp.csr_matrix((np.ones(4), (np.arange(4), [0, 1, 1, 2])), shape=(4, 3))
    rp, ci, va = _lib.i32(full.indptr), _lib.i32(full.indices), _lib.f64(full.data)
    for levels, put, want in ((1, [], MGB_E_ARG), (2, [1], MGB_E_ARG), (2, [0, 1], 0), (1, [0], 0)):      # no full subspace; a level missing
        h = C.c_void_p()
        _lib.call("mgb_geo_create", 4, 1, levels, 2, _lib.dptr(_lib.f64(x)), _lib.dptr(np.ones(4)), C.byref(h))
        try:
            for l in put:
                _lib.call("mgb_geo_set_matrix", h, ("sub:full:%d" % l).encode(), 4, 3, _lib.iptr(rp), _lib.iptr(ci), _lib.dptr(va))
            rc = lib.mgb_geo_dirichlet_on(h, b"m", None)
            print("levels %d, full at %r: status %d %s" % (levels, put, rc, lib.mgb_last_error() if rc else b""))
            assert rc == want
            assert (lib.mgb_geo_matrix_info(h, b"sub:m:0", None, None, None) == 0) == (want == 0)      # nothing added when refused
        finally:
            _lib.call("mgb_geo_destroy", h)


def test_python_surface_rejects_what_it_cannot_take():
    import mgb_amd as M
    g = M.fem2d(2)
    b = M.boundary(g)
    left = b.centre[:, 0] < -0.999
    assert {"dirichlet_on", "neumann_load"} <= set(M.__all__)
    with pytest.raises(ValueError, match="None"):
        M.dirichlet_on(g, None)
    for name in ("full", "dirichlet", "fixed", "", "a:b"):
        with pytest.raises(ValueError, match="name"):
            M.dirichlet_on(g, left, name)
    assert M.dirichlet_on(g, left) == "mixed" and "mixed" in g.subspaces
    with pytest.raises(ValueError, match="name"):
        M.dirichlet_on(g, left)                                           # already present
    with pytest.raises(ValueError, match="where"):
        M.dirichlet_on(g, np.ones(len(b)), "other")
    with pytest.raises(TypeError, match="Geometry"):
        M.dirichlet_on(np.zeros(3), left)
    eye = [sp.identity(4, format="csr")]
    with pytest.raises(M.MGBError, match="full subspace"):
        M.dirichlet_on(M.Geometry(dict(kind="hand", L=1, dim=1, block=2), np.array([[-1.0], [0.0], [0.0], [1.0]]), np.ones(4), {}, {},
                                  eye, eye), np.ones(2, dtype=bool))
    # neumann without dirichlet: refused before anything else is looked at
    with pytest.raises(ValueError, match="dirichlet"):
        M.amgb(g, neumann=0.5)
    with pytest.raises(ValueError, match="dirichlet"):
        M.parabolic_solve(g, neumann=lambda x: 0.5)
    # non-finite h on a selected facet; a masked-out NaN is not seen
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            M.neumann_load(g, bad)
        with pytest.raises(ValueError, match="finite"):
            M.neumann_load(g, lambda x: bad if x[0] > 0.999 else 1.0)
    hv = np.ones(b.nodes.shape)
    hv[left] = np.nan
    with pytest.raises(ValueError, match="finite"):
        M.neumann_load(g, hv)
    vals, mask, ts = M._neumann_data(g, hv, ~left, None)
    assert vals.shape == (1,) + b.nodes.shape and np.array_equal(mask, (~left).astype(np.uint8)) and ts is None
    with pytest.raises(TypeError, match="geometry"):
        M.neumann_load(g, hv, where=~left)                                # passes the data checks; a native geometry has no device
    with pytest.raises(ValueError, match="ts"):
        M.neumann_load(g, lambda t, x: t)
    with pytest.raises(TypeError, match="h"):
        M.neumann_load(g, lambda t, x, y: t)
    for shape in ((len(b),), (len(b), 2), (2, len(b), 2), (0,) + b.nodes.shape):
        with pytest.raises(ValueError, match="shape"):
            M.neumann_load(g, np.zeros(shape))
    vals, _, ts = M._neumann_data(g, lambda t, x: t + x[1], None, [0.5, 1.5])
    assert vals.shape == (2,) + b.nodes.shape and np.array_equal(ts, [0.5, 1.5])
    assert np.array_equal(vals[1], 1.5 + g.x[b.nodes][:, :, 1])
    assert np.array_equal(M._neumann_data(g, 0.25, None, None)[0], np.full((1,) + b.nodes.shape, 0.25))
