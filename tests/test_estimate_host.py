"""Interior facets, the host restatement of the error indicators (mgb_geo_interior_* / mgb_geo_estimate_host, csrc/boundary.hpp and
csrc/estimate.hpp), mark() and refine_triangles() on the CPU against the yardstick tests/estimate_reference.py (DESIGN.md section
4j).  Bars: KTOL = 1e-12 times the magnitude for a sum or a per-element value, KTOL relative for a maximum; facet tables bit for
bit."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import boundary_reference as BR
import energy_reference as ER
import estimate_reference as XR

MGB_E_ARG = -1
KTOL = XR.KTOL
INDICATOR_SHAPES = ("fem1d_L1", "fem1d_L2", "fem2d_L2", "fem2d_L2_Lshape", "fem2d_L4", "fem3d_L2_k1", "fem3d_L2_k3", "fem3d_L1_k3")
_MESHES = {}


def mesh(shape):
    if shape not in _MESHES:
        _MESHES[shape] = XR.Mesh(shape)
    return _MESHES[shape]


@pytest.fixture(scope="module")
def M():
    import mgb_amd
    return mgb_amd


# ------------------------------------------------------------------------------------------------ interior facets
@pytest.mark.parametrize("shape", list(XR.SHAPES))
def test_interior_facets_against_the_yardstick(lib, M, shape):
    g = mesh(shape)
    H = XR.host_interior(lib, g)
    assert g.nif == XR.SHAPES[shape][4] == len(H["elements"])              # fem1d L=2: 3, fem2d L=2: 8, fem3d L=2: 12 -- by dof sets
    for key, got in H.items():
        want = np.asarray(g.I[key]).reshape(got.shape)
        if got.dtype.kind == "i":
            assert np.array_equal(got, want), key
        else:
            assert got.tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes(), key
    I = M.interior(g.py)                                                   # the public view, cached on the geometry
    assert I is M.interior(g.py) and len(I) == g.nif
    for key, name in (("elements", "elements"), ("nodes", "nodes"), ("weights", "weights"), ("normal", "normal"), ("measure", "measure"),
                      ("centre", "centre"), ("element_facets", "element_facets")):
        assert getattr(I, name).tobytes() == H[key].tobytes()
    table, el = H["element_facets"], H["elements"]
    assert ((table >= 0) | (table <= -1)).all() and (table < g.nif).all() and (table >= -g.nf).all()      # no hole
    for f in range(g.nif):
        assert sorted(zip(*np.nonzero(table == f)))[0][0] == el[f, 0] and (table == f).sum() == 2 and el[f, 0] < el[f, 1]
    for f in range(g.nf):
        assert (table == -1 - f).sum() == 1 and table[g.F["element"][f]].tolist().count(-1 - f) == 1
    firsts = [(int(el[f, 0]), int(np.flatnonzero(table[el[f, 0]] == f)[0])) for f in range(g.nif)]
    assert firsts == sorted(firsts)
    k = g.k if g.dim == 3 else {1: 1, 2: 0}[g.dim]
    lfs = BR.local_facets(g.dim, k)
    for f in range(g.nif):
        a, b = H["nodes"][f]
        assert g.x[a].tobytes() == g.x[b].tobytes()                        # matched nodes: the same point, bit for bit
        eb = int(el[f, 1])
        lb = int(np.flatnonzero(table[eb] == f)[-1])
        _, nb, measure, _ = XR._facet_geometry(g.x[eb * g.block:(eb + 1) * g.block], g.dim, k, lb, lfs[lb][0])
        assert np.array_equal(nb, -H["normal"][f]) and abs(measure - H["measure"][f]) <= KTOL * measure      # n_A = -n_B


def test_the_boundary_list_is_unchanged_bit_for_bit(M):
    with open(os.path.join(os.path.dirname(__file__), "golden", "boundary_lists_sha256.json")) as fh:
        want = json.load(fh)                                               # recorded before the builder was shared
    for shape, digest in want.items():
        b = M.boundary(mesh(shape).py)
        got = hashlib.sha256(b"".join(a.tobytes() for a in (b.element, b.nodes, b.weights, b.normal, b.measure, b.centre))).hexdigest()
        assert got == digest, shape


# ------------------------------------------------------------------------------------------------ the indicator
@pytest.mark.parametrize("p", ER.P_VALUES)
@pytest.mark.parametrize("shape", INDICATOR_SHAPES)
def test_host_indicator_against_the_yardstick(lib, shape, p):
    g = mesh(shape)
    pv = ER.exponent(p, g.x)
    rng = np.random.default_rng(700)
    z = rng.standard_normal((g.n, 3))
    f, h, free = rng.standard_normal(g.n), rng.standard_normal((g.nf, g.q)), rng.random(g.nf) < 0.6
    for r in XR.R_VALUES:
        for u, scale, fv, hv, fr in ((0, None, f, h, free), (2, 1.0, None, None, None), (0, None, None, h, None), (1, 0.75, f, None, None)):
            name = "%s p=%s r=%g u=%d scale=%s" % (shape, p, r, u, scale)
            R = XR.host_estimate(lib, g, z, pv, f=fv, u=u, r=r, scale=scale, h=hv, mask=fr)
            Y = XR.indicators(g.ops, g.w, g.F, g.I, z[:, u], pv, f=fv, r=r, scale=scale, h=hv, mask=fr)
            XR.check(name, Y, R["parts"], R["totals"], R["J"], R["N"])
            flux = ER.host_energy(lib, g, [z], pv, u=u, s=(u + 1) % 3)[1][0]
            assert R["sigma"].tobytes() == flux.tobytes()                 # Sigma is the flux of the energy module, bit for bit


def quadratic(g, lam):
    if g.block in (2, 8):                                                  # elements of degree 1 hold a linear u
        u = g.x @ np.array([1.0, -2.0, 0.5][:g.dim]) + 0.25
        return np.column_stack([u, np.ones(g.n)]), None
    return np.column_stack([(g.x ** 2).sum(axis=1), np.ones(g.n)]), np.full(g.n, lam * 2.0 * g.dim)


@pytest.mark.parametrize("scale", [None, 1.0])
@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem2d_L3", "fem3d_L2_k1", "fem3d_L3_k2", "fem3d_L3_k3"])
def test_closed_form_zero_residual(lib, shape, scale):
    """(a) p = 2, u = |x|^2, f = 2 dim lambda (a linear u with f = 0 where the elements have degree 1: fem1d, fem3d k = 1)."""
    g = mesh(shape)
    z, f = quadratic(g, 2.0 if scale is None else scale)
    for r in XR.R_VALUES:
        R = XR.host_estimate(lib, g, z, 2.0, f=f, r=r, scale=scale)
        Y = XR.indicators(g.ops, g.w, g.F, g.I, z[:, 0], 2.0, f=f, r=r, scale=scale)
        print("%s r=%g: largest part %.3e, magnitude %.3e" % (shape, r, R["parts"].max(), Y["parts_mag"].max()))
        assert (R["parts"] <= KTOL * Y["parts_mag"]).all() and (R["totals"][:3] <= KTOL * Y["totals_mag"]).all()
        # a facet on which sigma . n vanishes has magnitude 0 in the yardstick, whose sigma is exactly 0 there; the library's
        # gradient is a sum that cancels to a few ulp of the field, so J itself is held to the largest facet magnitude
        assert (R["J"] <= KTOL * Y["J_mag"].max()).all()


@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem2d_L3", "fem3d_L2_k3"])
def test_closed_form_one_element(lib, shape):
    """(b) u = a . x on one element, 0 elsewhere, p = 2."""
    g = mesh(shape)
    e0, a = g.nel // 2, np.array([1.0, -2.0, 0.5][:g.dim])
    sl = slice(e0 * g.block, (e0 + 1) * g.block)
    z = np.zeros((g.n, 2))
    z[sl, 0] = g.x[sl] @ a
    for r, scale in ((2.0, None), (1.5, 1.0), (1.0, 3.0)):
        lam = 2.0 if scale is None else scale
        R = XR.host_estimate(lib, g, z, 2.0, r=r, scale=scale)
        Y = XR.indicators(g.ops, g.w, g.F, g.I, z[:, 0], 2.0, r=r, scale=scale)
        XR.check("%s one element r=%g" % (shape, r), Y, R["parts"], R["totals"], R["J"], R["N"])
        assert (R["parts"][:, 0] <= KTOL * Y["parts_mag"][:, 0]).all() and (np.delete(R["parts"][:, 0], e0) == 0.0).all()
        on = (g.I["elements"] == e0).any(axis=1)
        J = np.where(on, g.I["measure"] * np.abs(lam * (g.I["normal"] @ a)) ** r, 0.0)
        assert (np.abs(R["J"] - J) <= 8 * KTOL * J).all() and (R["J"][~on] == 0.0).all() and (J[on] > 0.0).any()
        for e in range(g.nel):
            he = math.fsum(g.w[e * g.block:(e + 1) * g.block]) ** (1.0 / g.dim)
            want = 0.5 * he * math.fsum(J[t] for t in g.I["element_facets"][e] if t >= 0)
            assert abs(R["parts"][e, 1] - want) <= 8 * KTOL * want
        assert (R["parts"][:, 2] == 0.0).all() and (R["N"] == 0.0).all()


@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem3d_L2_k1", "fem3d_L2_k3"])
def test_closed_form_neumann(lib, shape):
    """(c) u = x, p = 2, Neumann data on the facets of x = 1: h = -lambda gives 0, h = 0 gives N_F = |F| lambda^r."""
    g = mesh(shape)
    z = np.column_stack([g.x[:, 0], np.ones(g.n)])
    right = g.F["centre"][:, 0] > 0.999
    assert right.any() and not right.all()
    for r, scale in ((2.0, None), (1.5, 0.5)):
        lam = 2.0 if scale is None else scale
        h = np.full((g.nf, g.q), -lam)
        R = XR.host_estimate(lib, g, z, 2.0, r=r, scale=scale, h=h, mask=right)
        Y = XR.indicators(g.ops, g.w, g.F, g.I, z[:, 0], 2.0, r=r, scale=scale, h=h, mask=right)
        assert (R["N"] <= KTOL * Y["N_mag"]).all() and (R["parts"][:, 2] <= KTOL * Y["parts_mag"][:, 2]).all()
        R = XR.host_estimate(lib, g, z, 2.0, r=r, scale=scale, h=np.zeros((g.nf, g.q)), mask=right)
        want = np.where(right, g.F["measure"] * lam ** r, 0.0)
        assert (np.abs(R["N"] - want) <= 8 * KTOL * want).all()


@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem2d_L3", "fem3d_L2_k1", "fem3d_L2_k3"])
def test_nan_stays_where_it_feeds(lib, shape):
    """(d), (e)."""
    g = mesh(shape)
    e0 = g.nel // 2
    rng = np.random.default_rng(710)
    z, h, free = rng.standard_normal((g.n, 2)), rng.standard_normal((g.nf, g.q)), rng.random(g.nf) < 0.6
    f = np.full(g.n, 0.2)
    clean = XR.host_estimate(lib, g, z, 1.5, f=f, h=h, mask=free)
    zn = z.copy()
    zn[e0 * g.block, 0] = np.nan
    R = XR.host_estimate(lib, g, zn, 1.5, f=f, h=h, mask=free)
    Y = XR.indicators(g.ops, g.w, g.F, g.I, zn[:, 0], 1.5, f=f, h=h, mask=free)
    XR.check("%s NaN u" % shape, Y, R["parts"], R["totals"], R["J"], R["N"])
    hit = np.zeros(g.nel, dtype=bool)
    hit[e0] = True
    hit[g.I["elements"][(g.I["elements"] == e0).any(axis=1)].reshape(-1).astype(int)] = True
    eta = R["parts"].sum(axis=1)
    assert np.array_equal(np.isnan(eta), hit) and np.isnan(R["parts"][e0, 0]) and np.isnan(R["parts"][hit, 1]).all()
    assert not np.isnan(np.delete(R["parts"][:, 0], e0)).any() and R["parts"][~hit].tobytes() == clean["parts"][~hit].tobytes()
    assert np.isnan(R["totals"][[0, 1, 3, 4]]).all()
    for name, bad in (("f", dict(f=np.where(np.arange(g.n) == e0 * g.block + 1, np.inf, f), h=h)),
                      ("h", dict(f=f, h=np.where(np.arange(g.nf)[:, None] == np.flatnonzero(free)[0], np.nan, h)))):
        R = XR.host_estimate(lib, g, z, 1.5, mask=free, **bad)
        Y = XR.indicators(g.ops, g.w, g.F, g.I, z[:, 0], 1.5, mask=free, **bad)
        XR.check("%s non-finite %s" % (shape, name), Y, R["parts"], R["totals"], R["J"], R["N"])
        assert np.isnan(R["parts"]).sum() == 1 and np.isnan(R["totals"][3])
    hn = h.copy()
    hn[~free] = np.nan                                                    # (e) not seen behind the mask
    seen = XR.host_estimate(lib, g, z, 1.5, f=f, h=hn, mask=free)
    assert all(seen[k].tobytes() == clean[k].tobytes() for k in ("parts", "totals", "J", "N"))


def test_refused_inputs(lib, M):
    from mgb_amd import _lib
    g = mesh("fem2d_L2")
    z = np.random.default_rng(720).standard_normal((g.n, 3))
    for bad in (dict(S=0), dict(u=3), dict(u=-1), dict(p=0.5), dict(p=math.nan), dict(p=np.where(np.arange(g.n) == 4, 0.5, 2.0)), dict(r=0.99),
                dict(r=math.nan), dict(r=math.inf), dict(scale=math.inf), dict(scale=math.nan)):
        kw = dict(p=2.0)
        kw.update(bad)
        rc, parts, out = XR.host_estimate(lib, g, z, kw.pop("p"), rc_only=True, **kw)
        assert rc == MGB_E_ARG and (parts == 7.0).all() and (out == 7.0).all(), bad
    out, eta = np.full(5, 7.0), np.full((g.nel, 3), 7.0)
    args = (3, 0, 2.0, None, None, 2.0, 0, 1.0, None, None)
    assert lib.mgb_geo_estimate_host(None, _lib.dptr(z), *args, _lib.dptr(eta), None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert lib.mgb_geo_estimate_host(g.handle, None, *args, _lib.dptr(eta), None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert lib.mgb_geo_estimate_host(g.handle, _lib.dptr(z), *args, None, None, None, None, _lib.dptr(out)) == MGB_E_ARG
    assert lib.mgb_geo_estimate_host(g.handle, _lib.dptr(z), *args, _lib.dptr(eta), None, None, None, None) == MGB_E_ARG
    assert lib.mgb_geo_interior_dims(None, None, None, None, None, None) == MGB_E_ARG
    assert lib.mgb_geo_interior_get(None, None, None, None, None, None, None, None) == MGB_E_ARG
    assert (eta == 7.0).all() and (out == 7.0).all()
    # the Python layer, as far as it goes without a device
    with pytest.raises(ValueError, match="dirichlet"):
        M.estimate(g.py, 2.0, z=z, neumann=1.0)
    with pytest.raises(TypeError, match="ParabolicSOL"):
        M.estimate(M.ParabolicSOL(g.py, np.zeros(1), [z]), 2.0)
    with pytest.raises(TypeError):
        M.estimate(g.py, 2.0, z=z)                                         # a native geometry
    with pytest.raises(TypeError):
        M.estimate(z, 2.0)
    with pytest.raises(TypeError):
        M.interior("mesh")


def test_a_mesh_whose_sides_do_not_match_is_refused(lib):
    """Two triangles that share their corner dofs on an edge but not the dof of its midpoint."""
    import ctypes as C
    import scipy.sparse as sp
    from mgb_amd import _lib
    g = XR.Mesh("fem2d_L2")
    try:
        full = sp.csr_matrix(g.py.subspaces["full"][-1])
        f0 = 0
        b = int(g.I["nodes"][f0, 1, 1])                                    # the midpoint row of the second side: give it a dof of its own
        cols = full.indices.copy()
        cols[full.indptr[b]] = full.shape[1]
        S = sp.csr_matrix((full.data, cols, full.indptr), shape=(full.shape[0], full.shape[1] + 1))
        rp, ci, va = _lib.i32(S.indptr), _lib.i32(S.indices), _lib.f64(S.data)
        assert lib.mgb_geo_set_matrix(g.handle, b"sub:full:1", S.shape[0], S.shape[1], _lib.iptr(rp), _lib.iptr(ci), _lib.dptr(va)) == 0
        nif = C.c_int(-7)
        assert lib.mgb_geo_interior_dims(g.handle, C.byref(nif), None, None, None, None) == MGB_E_ARG and nif.value == -7
        assert b"matched" in lib.mgb_last_error()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ mark
def test_mark(M):
    v = np.array([1.0, 4.0, 4.0, 0.0, 1.0, 2.0])
    assert M.mark(v, 0.5).tolist() == [1, 2]                               # exact ties go to the lower index
    assert M.mark(v, 1.0 / 3.0).tolist() == [1]
    assert M.mark(v, 0.34).tolist() == [1, 2]
    assert M.mark(v, 1.0).tolist() == [1, 2, 5, 0, 4]                      # everything non-zero, then the shortest prefix
    assert M.mark(np.array([1e-3, 100.0, 1e-3]), 0.9).tolist() == [1]      # a single dominant entry
    assert M.mark(np.ones(4), 0.5).tolist() == [0, 1] and M.mark(np.ones(4), 0.51).tolist() == [0, 1, 2]
    assert M.mark(np.zeros(3)).size == 0 and M.mark(np.zeros(0)).size == 0 and M.mark([3.0]).tolist() == [0]
    rng = np.random.default_rng(730)
    for theta in (0.1, 0.5, 0.9, 1.0):
        for _ in range(20):
            w = rng.random(rng.integers(1, 40)) ** 4
            w[rng.random(w.size) < 0.2] = 0.0
            marked = M.mark(w, theta)
            assert XR.dorfler_ok(w, marked, theta) and len(set(marked.tolist())) == len(marked)
            assert (np.diff(w[marked]) <= 0.0).all()
    for theta in (0.0, -0.5, 1.0001, math.nan):
        with pytest.raises(ValueError, match="theta"):
            M.mark(v, theta)
    for bad in ([1.0, math.nan], [math.inf, 1.0], [1.0, -1.0]):
        with pytest.raises(ValueError):
            M.mark(bad)


# ------------------------------------------------------------------------------------------------ refine_triangles
SQUARE = np.array([[-1, -1], [1, -1], [-1, 1], [1, -1], [1, 1], [-1, 1]], dtype=float)
# a hand-made mesh with an obtuse triangle (the first one: about 127 degrees at (1, 0.5)) around the point (1, 0.5)
OBTUSE = np.array([[0, 0], [3, 0], [1, 0.5], [3, 0], [3, 2], [1, 0.5], [3, 2], [0, 2], [1, 0.5], [0, 2], [0, 0], [1, 0.5]], dtype=float)
MESHES = {"square": (SQUARE, 8.0, 4.0), "lshape": (BR.L_SHAPE, 8.0, 3.0), "obtuse": (OBTUSE, 10.0, 6.0)}


def corner_triangles(K):
    return [t for t, tri in enumerate(XR.triangles(K)) if (np.abs(tri).sum(axis=1) == 0.0).any()]


def check_refinement(M, K0, K, marked, perimeter, area, angle0):
    XR.check_conforming(K)
    assert (XR.orientation(K) > 0.0).all() and abs(0.5 * XR.orientation(K).sum() - area) <= KTOL
    b = M.boundary(M.fem2d(1, K))                                          # a hanging node would add boundary facets
    assert abs(math.fsum(b.measure) - perimeter) <= KTOL * 8
    assert XR.smallest_angle(K) >= 0.5 * angle0
    old, new = XR.triangles(K0), XR.triangles(K)
    have = {tri.tobytes() for tri in new}
    kept = [t for t in range(len(old)) if old[t].tobytes() in have]
    assert not set(kept) & set(int(t) for t in marked)                     # no marked triangle survives
    order = [next(i for i, tri in enumerate(new) if tri.tobytes() == old[t].tobytes()) for t in kept]
    assert order == sorted(order)                                          # the untouched keep their bits and their relative order
    assert len(new) >= len(old) + (1 if len(marked) else 0)


@pytest.mark.parametrize("name", list(MESHES))
def test_refine_triangles(M, name):
    K0, perimeter, area = MESHES[name]
    angle0 = XR.smallest_angle(K0)
    m = len(K0) // 3
    assert M.refine_triangles(K0, []).tobytes() == np.ascontiguousarray(K0).tobytes()
    assert M.refine_triangles(K0, np.zeros(0, dtype=int)).tobytes() == np.ascontiguousarray(K0).tobytes()
    sets = [[t] for t in range(m)] + [list(range(m))]
    if name == "lshape":
        sets.append(corner_triangles(K0))
    for marked in sets:
        K = M.refine_triangles(K0, marked)
        check_refinement(M, K0, K, marked, perimeter, area, angle0)
    K = K0
    for round_ in range(3):                                                # three rounds in a row, towards the corner / first vertex
        marked = corner_triangles(K) if name != "obtuse" else [0, len(K) // 3 - 1]
        if name == "square":
            marked = [0]
        Kn = M.refine_triangles(K, marked)
        check_refinement(M, K, Kn, marked, perimeter, area, angle0)
        K = Kn
    for bad in (np.zeros((4, 2)), np.zeros((6, 3)), np.zeros(6)):
        with pytest.raises(ValueError):
            M.refine_triangles(bad, [0])
    with pytest.raises(ValueError):
        M.refine_triangles(K0, [m])
    with pytest.raises(ValueError):
        M.refine_triangles(K0, [-1])
    with pytest.raises(TypeError):
        M.refine_triangles(K0, [0.5])
