"""boundary_flux() on the device (csrc/boundary.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-node routine and against the numpy yardstick tests/boundary_reference.py.

Shapes (facet nodes): fem1d L=2 (2: one almost idle workgroup), fem2d L=2 (24: q = 3 does not divide 256), fem3d L=1 k=3 (96: the
largest element block), fem3d L=2 k=1 (96: q = 4), fem3d L=2 k=3 (384: 24 facets of 16 nodes, 16 facets per workgroup -- the
cross-workgroup pass and a partly idle last workgroup) and fem2d L=2 on the L-shaped K (48: a re-entrant corner).

Bars (tests/boundary_reference.py): a sum within KTOL = 1e-12 times its absolute sum, a per-facet value within KTOL times the
facet's own absolute sum, a maximum within KTOL relative; bit for bit where the contract says so (a batch against its fields one
by one, a call repeated, a mask against a callable, the fields next to a non-finite one)."""
import ctypes as C

import numpy as np
import pytest

import boundary_reference as BR
import energy_reference as ER

pytestmark = pytest.mark.gpu
MGB_E_ARG = -1
KTOL = BR.KTOL


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


class Mesh:
    """A device geometry of BR.SHAPES with the host handle of the same mesh and the numpy pieces of the yardstick."""

    def __init__(self, M, shape):
        kind, L, k, K, count = BR.SHAPES[shape]
        self.name = shape
        self.geo = M.fem1d_mpi(L) if kind == "fem1d" else (M.fem2d_mpi(L, K) if kind == "fem2d" else M.fem3d_mpi(L, k))
        self.host = BR.HostMesh(shape)
        self.x, self.n, self.dim, self.block, self.ops, self.F = (getattr(self.host, a) for a in ("x", "n", "dim", "block", "ops", "F"))
        self.nf, self.q = self.host.nf, self.host.q
        assert np.array_equal(self.geo.x.to_numpy().reshape(self.n, -1), self.x) and self.nf * self.q == count
        b = M.boundary(self.geo)                                          # the device geometry's facets are the yardstick's
        assert np.array_equal(b.nodes, self.F["nodes"]) and np.abs(b.weights - self.F["weights"]).max() <= KTOL

    def fields(self, B, seed):
        """B distinct random (n, 3) fields, broken across elements: a wrong stride, row or pointer shows."""
        rng = np.random.default_rng(seed)
        return [rng.standard_normal((self.n, 3)) for _ in range(B)]

    def half(self, seed):
        m = np.random.default_rng(seed).random(self.nf) < 0.5
        m[0] = True
        return m


_MESHES = {}


def mesh(M, shape):
    if shape not in _MESHES:
        _MESHES[shape] = Mesh(M, shape)
    return _MESHES[shape]


def rows(r):
    """(B, 5) in the column order of the C ABI from a BoundaryFlux."""
    return np.column_stack([np.atleast_1d(v) for v in (r.flux, r.trace, r.measure, r.normal_max, r.tangential_max)])


def batch(M, m, zs, p, **kw):
    """boundary_flux() of the fields zs in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(m.geo, np.arange(float(len(zs))), [M.HPCMatrix(z) for z in zs])
    r = M.boundary_flux(sol, p, **kw)
    assert np.array_equal(r.ts, sol.ts) and all(np.shape(v) == (len(zs),) for v in (r.flux, r.trace, r.measure, r.normal_max, r.tangential_max))
    assert (r.facets is None) == (not kw.get("per_facet")) and (r.facets is None or r.facets.shape == (len(zs), m.nf))
    return rows(r), r.facets


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", ER.P_VALUES)
@pytest.mark.parametrize("shape", list(BR.SHAPES))
def test_device_against_host_and_numpy(M, lib, shape, p, B):
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    zs = m.fields(B, 500 + B)
    for u, mask in ((0, None), (2, m.half(7))):
        name = "%s p=%s B=%d u=%d%s" % (shape, p, B, u, "" if mask is None else " masked")
        if B == 1:
            r = M.boundary_flux(m.geo, pv, u=u, z=zs[0], where=mask, per_facet=True)
            assert all(isinstance(v, float) for v in (r.flux, r.trace, r.measure, r.normal_max, r.tangential_max)) and r.ts is None
            assert r.facets.shape == (m.nf,)
            got, fac = rows(r), r.facets.reshape(1, -1)
        else:
            got, fac = batch(M, m, zs, pv, u=u, where=mask, per_facet=True)
        host, host_fac = BR.host_boundary_flux(lib, m.host, zs, pv, u=u, mask=mask)
        ref = [BR.boundary_flux(m.ops, m.F, zs[b][:, u], pv, mask) for b in range(B)]
        want, sums = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
        BR.check(name + " device against numpy", got, want, sums)
        BR.check(name + " device against host", got, host, sums)
        for b in range(B):
            BR.check_facets(name + " device against numpy", fac[b], ref[b][2], ref[b][3])
            BR.check_facets(name + " device against host", fac[b], host_fac[b], ref[b][3])
            gap = abs(fac[b].sum() - got[b, 0])
            print("%s: per-facet values sum to the flux within %.3e (bar %.3e)" % (name, gap, KTOL * sums[b, 0]))
            assert gap <= KTOL * sums[b, 0]


@pytest.mark.parametrize("p", [1.5, "array"])
@pytest.mark.parametrize("shape", list(BR.SHAPES))
def test_batch_is_the_singles_and_a_call_repeats(M, shape, p):
    """The reduction order may not depend on the batch index or on B: three fields in one call give, bit for bit, the results of
    three calls, with and without a selection, and so does the same call made again."""
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    zs = m.fields(3, 510)
    for mask in (None, m.half(8)):
        got, fac = batch(M, m, zs, pv, u=1, where=mask, per_facet=True)
        for b in range(3):
            single = M.boundary_flux(m.geo, pv, u=1, z=M.HPCMatrix(zs[b]), where=mask, per_facet=True)
            assert got[b].tobytes() == rows(single)[0].tobytes(), (b, got[b], rows(single)[0])
            assert fac[b].tobytes() == single.facets.tobytes()
        again, fac2 = batch(M, m, zs, pv, u=1, where=mask, per_facet=True)
        assert again.tobytes() == got.tobytes() and fac2.tobytes() == fac.tobytes()
        swapped, _ = batch(M, m, zs[::-1], pv, u=1, where=mask)
        assert swapped[::-1].tobytes() == got.tobytes()                   # with or without the per-facet output


@pytest.mark.parametrize("shape", list(BR.SHAPES))
def test_non_finite_input(M, shape):
    """One NaN or Inf at a boundary node of one field: that field is all NaN, its neighbours in the batch keep their bits.  A NaN
    where no selected facet looks -- another column, an element without a boundary facet, the facets of an element left out by
    the mask -- changes nothing."""
    m = mesh(M, shape)
    zs = m.fields(3, 520)
    pn = ER.exponent("array", m.x)
    clean, clean_fac = batch(M, m, zs, pn, per_facet=True)
    assert np.isfinite(clean).all() and np.isfinite(clean_fac).all()
    first, last = m.F["nodes"][0, 0], m.F["nodes"][-1, -1]
    for node, bad, which in ((last, np.nan, 1), (first, np.inf, 0), (last, -np.inf, 2)):
        broken = [z.copy() for z in zs]
        broken[which][node, 0] = bad
        got, fac = batch(M, m, broken, pn, per_facet=True)
        assert np.isnan(got[which]).all() and np.isnan(fac[which]).any(), (node, bad, which, got)
        for other in set(range(3)) - {which}:
            assert got[other].tobytes() == clean[other].tobytes() and fac[other].tobytes() == clean_fac[other].tobytes()
        single = M.boundary_flux(m.geo, pn, z=broken[which])
        assert np.isnan(rows(single)).all()
        without = m.F["element"] != m.F["element"][0 if node == first else -1]
        got, _ = batch(M, m, broken, pn, where=without)
        ref, _ = batch(M, m, zs, pn, where=without)
        assert got.tobytes() == ref.tobytes() and (np.isfinite(got).all() or not without.any())
    other = [z.copy() for z in zs]
    other[1][last, 1] = np.nan
    interior = np.setdiff1d(np.arange(m.n // m.block), m.F["element"])
    if len(interior):
        other[1][interior[0] * m.block, 0] = np.nan
    got, fac = batch(M, m, other, pn, per_facet=True)
    assert got.tobytes() == clean.tobytes() and fac.tobytes() == clean_fac.tobytes()
    pb = pn.copy()
    pb[last] = np.nan                                                     # the exponent: only the C ABI lets a bad one through
    loc, backend = M._locator_of(m.geo)
    zv, pv, out = M.HPCVector(zs[0], backend), M.HPCVector(pb, backend), np.zeros((1, 5))
    from mgb_amd import _lib
    M.call("mgb_boundary_flux", m.geo._boundary_dev, 1, (C.c_void_p * 1)(zv.handle.value), 3, 0, 2.0, pv.handle, None, None, _lib.dptr(out))
    assert np.isnan(out).all()


@pytest.mark.parametrize("shape", list(BR.SHAPES))
def test_selection(M, shape):
    """where= as a mask and as a callable give the same bits; an empty selection gives five zeros; every facet selected is no
    selection; the two halves of a split add up to the whole within the bar."""
    m = mesh(M, shape)
    z = m.fields(1, 530)[0]
    side = lambda c: c[0] > 0.0
    mask = m.F["centre"][:, 0] > 0.0
    assert 0 < mask.sum() < m.nf
    a = M.boundary_flux(m.geo, 1.5, z=z, where=side, per_facet=True)
    b = M.boundary_flux(m.geo, 1.5, z=z, where=mask, per_facet=True)
    assert rows(a).tobytes() == rows(b).tobytes() and a.facets.tobytes() == b.facets.tobytes()
    assert np.array_equal(a.facets[~mask], np.zeros((~mask).sum())) and (a.facets[mask] != 0.0).all()
    none = M.boundary_flux(m.geo, 1.5, z=z, where=lambda c: False, per_facet=True)
    assert np.array_equal(rows(none), np.zeros((1, 5))) and np.array_equal(none.facets, np.zeros(m.nf))
    whole = M.boundary_flux(m.geo, 1.5, z=z, per_facet=True)
    every = M.boundary_flux(m.geo, 1.5, z=z, where=np.ones(m.nf, dtype=bool), per_facet=True)
    assert rows(whole).tobytes() == rows(every).tobytes() and whole.facets.tobytes() == every.facets.tobytes()
    rest = M.boundary_flux(m.geo, 1.5, z=z, where=~mask)
    _, sums, _, _ = BR.boundary_flux(m.ops, m.F, z[:, 0], 1.5)
    print("%s: the two sides add up to the whole within %.3e (bar %.3e)" % (shape, abs(a.flux + rest.flux - whole.flux), KTOL * sums[0]))
    assert abs(a.flux + rest.flux - whole.flux) <= KTOL * sums[0] and abs(a.measure + rest.measure - whole.measure) <= KTOL * sums[2]
    assert whole.normal_max == max(a.normal_max, rest.normal_max) and whole.tangential_max == max(a.tangential_max, rest.tangential_max)
    assert np.array_equal(a.facets[mask], whole.facets[mask])             # a facet's value does not depend on the selection


@pytest.mark.parametrize("p", [1.0, 2.0, "array"])
@pytest.mark.parametrize("shape", list(BR.SHAPES))
def test_per_facet_values_are_the_sums_of_the_flux_rows(M, shape, p):
    """Each facet's value is sum_j omega_j (sigma_j . n) with sigma the rows of M.flux() -- the same arithmetic on the device."""
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    z = m.fields(1, 540)[0]
    r = M.boundary_flux(m.geo, pv, z=z, per_facet=True)
    sigma = M.flux(m.geo, pv, z=z).to_numpy()
    sn = (sigma[m.F["nodes"]] * m.F["normal"][:, None, :]).sum(axis=2)
    want = (m.F["weights"] * sn).sum(axis=1)
    bar = (m.F["weights"] * np.abs(sn)).sum(axis=1)
    BR.check_facets("%s p=%s facets against the flux rows" % (shape, p), r.facets, want, bar)
    assert abs(r.facets.sum() - r.flux) <= KTOL * bar.sum()
    assert abs(r.normal_max - np.abs(sn).max()) <= KTOL * r.normal_max


def test_known_answers(M):
    """The divergence theorem on fields the elements hold exactly (test_boundary_host.py has the reasoning): flux 12 on the
    square at L = 1, 2, 3 with 4, 4, 2, 2 through the sides; 9 on the L shape; 20 on the cube for k = 2, 3; 0 for u = x y + z (k = 1)
    and u = 1.5 x (1-D).  The absolute sums of the bars are the yardstick's."""
    quad = lambda x: x[:, 0] ** 2 + 0.5 * x[:, 1] ** 2 + 0.3 * x[:, 0] * x[:, 1]
    cubic = lambda x: x[:, 0] ** 2 + 0.5 * x[:, 1] ** 2 - 0.25 * x[:, 2] ** 2 + x[:, 0] * x[:, 1] * x[:, 2]
    cases = [("fem2d", L, None, None, quad, 12.0, 8.0) for L in (1, 2, 3)] + [("fem2d", 2, None, BR.L_SHAPE, quad, 9.0, 8.0)]
    cases += [("fem3d", L, k, None, cubic, 20.0, 24.0) for L, k in ((1, 2), (2, 2), (1, 3), (2, 3))]
    cases += [("fem3d", 2, 1, None, lambda x: x[:, 0] * x[:, 1] + x[:, 2], 0.0, 24.0), ("fem1d", 2, None, None, lambda x: 1.5 * x[:, 0], 0.0, 2.0)]
    for kind, L, k, K, f, flux, measure in cases:
        geo = M.fem1d_mpi(L) if kind == "fem1d" else (M.fem2d_mpi(L, K) if kind == "fem2d" else M.fem3d_mpi(L, k))
        host = BR.HostMesh(kind=kind, L=L, k=k, K=K)
        try:
            u = f(host.x)
            _, sums, _, _ = BR.boundary_flux(host.ops, host.F, u, 2.0)
            r = M.boundary_flux(geo, 2.0, z=u)
            print("%s L=%d n=%d: flux %.17g (%g), measure %.17g (%g), bar %.3e" % (kind, L, len(u), r.flux, flux, r.measure, measure, KTOL * sums[0]))
            assert sums[0] > 1.0 and abs(r.flux - flux) <= KTOL * sums[0] and abs(r.measure - measure) <= KTOL * measure
            assert abs(r.trace - (host.F["weights"] * u[host.F["nodes"]]).sum()) <= KTOL * sums[1]
            if kind == "fem2d" and L == 3:
                sides = {"left": (lambda c: c[0] < -0.999, 4.0), "right": (lambda c: c[0] > 0.999, 4.0),
                         "top": (lambda c: c[1] > 0.999, 2.0), "bottom": (lambda c: c[1] < -0.999, 2.0)}
                for side, (where, want) in sides.items():
                    r = M.boundary_flux(geo, 2.0, z=u, where=where)
                    _, part, _, _ = BR.boundary_flux(host.ops, host.F, u, 2.0, [where(c) for c in host.F["centre"]])
                    print("fem2d L=3 %s: flux %.17g (%g), measure %.17g (2), bar %.3e" % (side, r.flux, want, r.measure, KTOL * part[0]))
                    assert abs(r.flux - want) <= KTOL * part[0] and abs(r.measure - 2.0) <= KTOL * 2.0
        finally:
            host.close()


def test_stationary_solution(M):
    sol = M.fem2d_mpi_solve(L=3, p=1.5)
    r = M.boundary_flux(sol, 1.5, per_facet=True)
    nat = M.mpi_to_native(sol)
    ops = ER.operators(nat.geometry)
    F = BR.facets(nat.geometry)
    want, sums, pf, pfa = BR.boundary_flux(ops, F, nat.z[:, 0], 1.5)
    BR.check("fem2d L=3 p=1.5 solved", rows(r), want, sums)
    BR.check_facets("fem2d L=3 p=1.5 solved", r.facets, pf, pfa)
    forcing = np.array([M.DEFAULT_F[2](xi)[0] for xi in nat.geometry.x])
    print("fem2d L=3 p=1.5 solved: flux %.17g trace %.17g measure %.17g normal_max %.6g tangential_max %.6g"
          % (r.flux, r.trace, r.measure, r.normal_max, r.tangential_max))
    print("fem2d L=3 p=1.5 solved: balance p * flux = %.6g against int f = %.6g (measured, not a bar)" % (1.5 * r.flux, nat.geometry.w @ forcing))
    assert M.mpi_to_native(r) is r


def test_parabolic_solution(M):
    """One call on the five snapshots equals five single calls, bit for bit; ts is carried."""
    sol = M.parabolic_solve(M.fem1d_mpi(3), h=0.25, p=2.0)
    r = M.boundary_flux(sol, 2.0, per_facet=True)
    assert len(sol.u) == 5 and np.array_equal(r.ts, sol.ts) and r.facets.shape == (5, 2)
    for name in ("flux", "trace", "measure", "normal_max", "tangential_max"):
        v = getattr(r, name)
        assert isinstance(v, np.ndarray) and v.shape == (5,) and np.isfinite(v).all()
        print("parabolic fem1d L=3 p=2 %-14s %s" % (name, " ".join("%.12g" % t for t in v)))
    singles = np.vstack([rows(M.boundary_flux(sol.geometry, 2.0, z=uk)) for uk in sol.u])
    assert rows(r).tobytes() == singles.tobytes()
    assert np.array_equal(r.measure, np.full(5, 2.0)) and np.array_equal(r.tangential_max, np.zeros(5))


def test_errors(M, lib):
    from mgb_amd import _lib
    m = mesh(M, "fem1d_L2")
    g, n = m.geo, m.n
    z = m.fields(1, 550)[0]
    for bad in (0.5, np.nan, np.inf, -1.0, np.full(n, 0.5), np.r_[np.full(n - 1, 2.0), np.nan], np.full(n + 1, 2.0), lambda x: 0.0):
        with pytest.raises(ValueError, match="p"):
            M.boundary_flux(g, bad, z=z)
    for kw in (dict(u=3), dict(u=-4)):
        with pytest.raises(ValueError, match="column"):
            M.boundary_flux(g, 2.0, z=z, **kw)
    with pytest.raises(TypeError, match="column"):
        M.boundary_flux(g, 2.0, z=z, u=0.5)
    with pytest.raises(ValueError, match="z"):
        M.boundary_flux(g, 2.0)                                           # a Geometry needs z=
    with pytest.raises(ValueError, match="z"):
        M.boundary_flux(g, 2.0, z=z[:-1])
    for bad in (np.ones(m.nf), np.ones(m.nf + 1, dtype=bool)):
        with pytest.raises(ValueError, match="where"):
            M.boundary_flux(g, 2.0, z=z, where=bad)
    sol = M.ParabolicSOL(g, np.arange(3.0), [M.HPCMatrix(z)] * 3)
    with pytest.raises(ValueError, match="z="):
        M.boundary_flux(sol, 2.0, z=z)
    assert M.boundary_flux(g, 2.0, z=z, u=-1).flux == M.boundary_flux(g, 2.0, z=z, u=2).flux
    # the C ABI: MGB_E_ARG before anything is launched
    loc, backend = M._locator_of(g)
    bd = g._boundary_dev
    nf, q, dim = C.c_int(), C.c_int(), C.c_int()
    assert lib.mgb_boundary_dims(bd, C.byref(nf), C.byref(q), C.byref(dim)) == 0 and (nf.value, q.value, dim.value) == (2, 1, 1)
    nodes, normal = np.empty((2, 1), dtype=np.int32), np.empty((2, 1))
    assert lib.mgb_boundary_get(bd, None, _lib.iptr(nodes), None, _lib.dptr(normal), None, None) == 0
    assert np.array_equal(nodes, m.F["nodes"]) and np.array_equal(normal, m.F["normal"])
    zv, short = M.HPCVector(z, backend), M.HPCVector(np.zeros(3 * n - 1), backend)
    out = np.zeros((3, 5))
    table = lambda *vs: (C.c_void_p * len(vs))(*[v.handle.value for v in vs])
    E = lambda B, tab, S, u, p, pn: lib.mgb_boundary_flux(bd, B, tab, S, u, p, pn, None, None, _lib.dptr(out))
    assert E(1, table(zv), 3, 0, 2.0, None) == 0
    for p in (0.5, np.nan, np.inf):
        assert E(1, table(zv), 3, 0, p, None) == MGB_E_ARG
    assert E(1, table(zv), 3, 3, 2.0, None) == MGB_E_ARG and E(1, table(zv), 3, -1, 2.0, None) == MGB_E_ARG
    assert E(0, table(zv), 3, 0, 2.0, None) == MGB_E_ARG and E(-1, table(zv), 3, 0, 2.0, None) == MGB_E_ARG
    assert E(1, table(short), 3, 0, 2.0, None) == MGB_E_ARG and E(2, table(zv, short), 3, 0, 2.0, None) == MGB_E_ARG
    assert E(1, table(zv), 2, 0, 2.0, None) == MGB_E_ARG                   # 3 n values are not n x 2
    assert E(1, table(zv), 3, 0, 2.0, short.handle) == MGB_E_ARG
    assert E(1, (C.c_void_p * 1)(None), 3, 0, 2.0, None) == MGB_E_ARG and E(1, None, 3, 0, 2.0, None) == MGB_E_ARG
    assert lib.mgb_boundary_flux(bd, 1, table(zv), 3, 0, 2.0, None, None, None, None) == MGB_E_ARG
    h = C.c_void_p()
    other = BR.HostMesh("fem2d_L2")
    try:
        assert lib.mgb_boundary_create(loc, other.handle, C.byref(h)) == MGB_E_ARG      # the locator of another geometry
        assert lib.mgb_boundary_create(loc, None, C.byref(h)) == MGB_E_ARG and lib.mgb_boundary_create(loc, m.host.handle, None) == MGB_E_ARG
    finally:
        other.close()
    backend.synchronize()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    n = g.x.shape[0]
    z = M.HPCMatrix(np.ones((n, 2)), be)
    assert M.boundary_flux(g, 2.0, z=z).flux == 0.0                       # fine while the context is one rank
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.boundary_flux(g, 2.0, z=z)
        out = np.zeros((1, 5))
        assert lib.mgb_boundary_flux(g._boundary_dev, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 2.0, None, None, None,
                                     _lib.dptr(out)) == MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
