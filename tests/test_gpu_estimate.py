"""estimate(), adapt() on the device (csrc/estimate.hip; contract in include/mgb_hip.h) against the host
restatement of the same routines and against the numpy / fsum yardstick tests/estimate_reference.py.

Shapes (each grouping rule once): fem1d L=1 (2 elements, 1 interior facet: one almost idle workgroup), fem1d L=2 (4 elements, 3
interior facets), fem2d L=2 (8 elements; block 7 and q = 3 divide nothing), fem2d L=2 on the L shape (24), fem2d L=4 (128 elements
= 3 workgroups of 36 + a partly idle one; 176 interior facets at 85 per workgroup: a partly idle third), fem3d L=2 k=1 (block 8,
q 4), fem3d L=2 k=3 (block 64: 4 elements per workgroup, 2 workgroups; q 16), fem3d L=1 k=3 (no interior facet: no facet launch
without Neumann data).

Bars (tests/estimate_reference.py): a sum or a per-element value within KTOL = 1e-12 times its magnitude, a maximum within KTOL
relative; bit for bit where the contract says so (a call repeated, the flux used inside, a masked-out NaN)."""
import ctypes as C
import math

import numpy as np
import pytest

import boundary_reference as BR
import energy_reference as ER
import estimate_reference as XR
import mgb_oracle as O
import mixed_reference as MR

pytestmark = pytest.mark.gpu
MGB_E_ARG = -1
KTOL = XR.KTOL
GPU_SHAPES = ("fem1d_L1", "fem1d_L2", "fem2d_L2", "fem2d_L2_Lshape", "fem2d_L4", "fem3d_L2_k1", "fem3d_L2_k3", "fem3d_L1_k3")


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


class Mesh:
    """A device geometry of XR.SHAPES with the host handle of the same mesh and the numpy pieces of the yardstick."""

    def __init__(self, M, shape):
        kind, L, k, K, nif = XR.SHAPES[shape]
        self.name, self.L = shape, L
        self.geo = M.fem1d_mpi(L) if kind == "fem1d" else (M.fem2d_mpi(L, K) if kind == "fem2d" else M.fem3d_mpi(L, k))
        self.host = XR.Mesh(shape)
        for a in ("x", "w", "n", "dim", "block", "ops", "F", "I", "nf", "q", "nif", "nel"):
            setattr(self, a, getattr(self.host, a))
        assert np.array_equal(self.geo.x.to_numpy().reshape(self.n, -1), self.x) and self.nif == nif
        I = M.interior(self.geo)                                          # the device geometry's facets are the yardstick's
        assert len(I) == nif and np.array_equal(I.nodes, self.I["nodes"].reshape(I.nodes.shape))
        assert np.array_equal(I.element_facets, self.I["element_facets"]) and I.normal.tobytes() == self.I["normal"].reshape(I.normal.shape).tobytes()

    def field(self, seed):
        return np.random.default_rng(seed).standard_normal((self.n, 3))

    def free(self, seed):
        m = np.random.default_rng(seed).random(self.nf) < 0.6
        m[0] = True
        return m


_MESHES = {}


def mesh(M, shape):
    if shape not in _MESHES:
        _MESHES[shape] = Mesh(M, shape)
    return _MESHES[shape]


def columns(ind):
    return np.array(ind.columns)


def compare(name, m, lib, ind, z, pv, u=0, f=None, r=2.0, scale=None, h=None, free=None):
    """The device result `ind` against the host restatement and the yardstick; returns the yardstick."""
    H = XR.host_estimate(lib, m.host, z, pv, f=f, u=u, r=r, scale=scale, h=h, mask=free)
    Y = XR.indicators(m.ops, m.w, m.F, m.I, z[:, u], pv, f=f, r=r, scale=scale, h=h, mask=free)
    XR.check(name + " device against numpy", Y, ind.parts, columns(ind))
    XR.check(name + " device against host", dict(Y, parts=H["parts"], totals=H["totals"]), ind.parts, columns(ind))
    assert ind.parts.shape == (m.nel, 3) and ind.eta.shape == (m.nel,) and ind.r == r
    want, mags = Y["totals"], Y["totals_mag"]

    def close(got, ref, bar):
        return (math.isnan(got) and math.isnan(ref)) or abs(got - ref) <= bar

    assert close(ind.volume, want[0], KTOL * mags[0]) and close(ind.jump, want[1], KTOL * mags[1]) and close(ind.neumann, want[2], KTOL * mags[2])
    assert close(ind.total ** r, math.fsum(want[:3]), 4 * KTOL * math.fsum(mags))
    assert close(ind.eta_max ** r, want[3], 4 * KTOL * want[3]) and close(ind.jump_max, want[4], KTOL * want[4])
    cw, cm = XR.coarse(Y["parts"], m.dim, m.L), XR.coarse(Y["parts_mag"], m.dim, m.L)
    got = ind.coarse(m.L)
    assert got.shape == cw.shape and np.array_equal(np.isnan(got), np.isnan(cw))
    ok = ~np.isnan(cw)
    print("%s: coarse off by %.3e" % (name, np.abs(got - cw)[ok].max() if ok.any() else 0.0))
    assert (np.abs(got - cw)[ok] <= KTOL * cm[ok]).all()
    return Y


@pytest.mark.parametrize("p", ER.P_VALUES)
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_device_against_host_and_numpy(M, lib, shape, p):
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    z = m.field(900)
    rng = np.random.default_rng(901)
    f, h, free = rng.standard_normal(m.n), rng.standard_normal((m.nf, m.q)), m.free(902)
    for r in XR.R_VALUES:
        for u, scale, fv, hv, fr in ((0, None, f, h, free), (2, 1.0, None, None, None), (0, None, None, h, np.ones(m.nf, dtype=bool)),
                                     (0, 0.75, f, None, None)):
            name = "%s p=%s r=%g u=%d scale=%s%s%s" % (shape, p, r, u, scale, " f" if fv is not None else "", "" if hv is None else " neumann")
            kw = {} if hv is None else dict(dirichlet=~fr, neumann=hv)
            ind = M.estimate(m.geo, pv, f=fv, u=u, z=z, r=r, scale=scale, **kw)
            compare(name, m, lib, ind, z, pv, u=u, f=fv, r=r, scale=scale, h=hv, free=fr)


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_a_call_repeats_bit_for_bit(M, shape):
    m = mesh(M, shape)
    z, pv = M.HPCMatrix(m.field(910)), ER.exponent("array", m.x)
    h, free = np.random.default_rng(911).standard_normal((m.nf, m.q)), m.free(912)
    a = M.estimate(m.geo, pv, f=0.3, z=z, r=1.5, dirichlet=~free, neumann=h)
    M.estimate(m.geo, 2.0, z=z)                                            # another call in between reuses the buffers
    b = M.estimate(m.geo, pv, f=0.3, z=z, r=1.5, dirichlet=~free, neumann=h)
    assert a.parts.tobytes() == b.parts.tobytes() and columns(a).tobytes() == columns(b).tobytes()


@pytest.mark.parametrize("p,r", [(1.5, 2.0), (3.0, 1.0), ("array", 2.0)])
@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem2d_L4"])
def test_the_flux_used_inside_is_flux(M, shape, p, r):
    """The jump numbers replayed on the host, operation by operation, from the bits of M.flux(): any other Sigma inside the call
    would show.  1-D and 2-D, r = 1 and 2: sqrt and the products are correctly rounded on both sides."""
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    z = m.field(920)
    ind = M.estimate(m.geo, pv, z=z, r=r)
    sigma = M.flux(m.geo, pv, z=z).to_numpy().reshape(m.n, m.dim)
    lam = np.broadcast_to(np.asarray(pv, dtype=float), (m.n,))
    J = np.zeros(m.nif)
    for F in range(m.nif):
        s = 0.0
        for j in range(m.q):
            a, b = m.I["nodes"][F, 0, j], m.I["nodes"][F, 1, j]
            d = 0.0
            for k in range(m.dim):
                d = d + (sigma[a, k] - sigma[b, k]) * m.I["normal"][F, k]
            aj = abs(lam[a] * d)
            s = s + m.I["weights"][F, j] * (aj * aj if r == 2.0 else aj)
        J[F] = s
    want = np.zeros(m.nel)
    for e in range(m.nel):
        ws = 0.0
        for i in range(e * m.block, (e + 1) * m.block):
            ws = ws + m.w[i]
        he, js = (ws if m.dim == 1 else np.sqrt(ws)), 0.0
        for t in m.I["element_facets"][e]:
            if t >= 0:
                js = js + J[t]
        want[e] = (0.5 * he) * js
    assert ind.parts[:, 1].tobytes() == want.tobytes()


def quadratic(m, lam):
    """(z, f) of the zero-residual closed form (a): u = |x|^2, f = 2 dim lambda where the elements hold quadratics, a linear u with
    f = 0 on the elements of degree 1 (fem1d, fem3d k = 1)."""
    if m.block in (2, 8):
        u = m.x @ np.array([1.0, -2.0, 0.5][:m.dim]) + 0.25
        return np.column_stack([u, np.ones(m.n)]), None
    return np.column_stack([(m.x ** 2).sum(axis=1), np.ones(m.n)]), np.full(m.n, lam * 2.0 * m.dim)


@pytest.mark.parametrize("scale", [None, 1.0])
@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem2d_L4", "fem3d_L2_k1", "fem3d_L3_k2", "fem3d_L3_k3"])
def test_closed_form_zero_residual(M, lib, shape, scale):
    m = mesh(M, shape)
    lam = 2.0 if scale is None else scale
    z, f = quadratic(m, lam)
    for r in XR.R_VALUES:
        ind = M.estimate(m.geo, 2.0, f=f, z=z, r=r, scale=scale)
        Y = XR.indicators(m.ops, m.w, m.F, m.I, z[:, 0], 2.0, f=f, r=r, scale=scale)
        print("%s r=%g: largest part %.3e, magnitude %.3e" % (shape, r, ind.parts.max(), Y["parts_mag"].max()))
        assert (ind.parts <= KTOL * Y["parts_mag"]).all() and (columns(ind)[:3] <= KTOL * Y["totals_mag"]).all()


@pytest.mark.parametrize("shape", ["fem2d_L2", "fem2d_L4", "fem3d_L2_k3", "fem1d_L2"])
def test_closed_form_one_element(M, lib, shape):
    """(b) u = a . x on one element, 0 elsewhere, p = 2: no volume term; J_F = |F| |lambda a . n_F|^r on that element's interior
    facets only, shared half and half with the neighbours."""
    m = mesh(M, shape)
    e0, a = m.nel // 2, np.array([1.0, -2.0, 0.5][:m.dim])
    sl = slice(e0 * m.block, (e0 + 1) * m.block)
    z = np.zeros((m.n, 2))
    z[sl, 0] = m.x[sl] @ a
    for r, scale in ((2.0, None), (1.5, 1.0), (1.0, 3.0)):
        lam = 2.0 if scale is None else scale
        ind = M.estimate(m.geo, 2.0, z=z, r=r, scale=scale)
        Y = compare("%s one element r=%g" % (shape, r), m, lib, ind, z, 2.0, r=r, scale=scale)
        assert (ind.parts[:, 0] <= KTOL * Y["parts_mag"][:, 0]).all() and (np.delete(ind.parts[:, 0], e0) == 0.0).all()
        J = np.zeros(m.nif)
        for F in np.flatnonzero((m.I["elements"] == e0).any(axis=1)):
            J[F] = m.I["measure"][F] * abs(lam * (a @ m.I["normal"][F])) ** r
        for e in range(m.nel):
            he = math.fsum(m.w[e * m.block:(e + 1) * m.block]) ** (1.0 / m.dim)
            want = 0.5 * he * math.fsum(J[t] for t in m.I["element_facets"][e] if t >= 0)
            assert abs(ind.parts[e, 1] - want) <= 8 * KTOL * want and (want > 0.0 or ind.parts[e, 1] == 0.0)
        assert ind.neumann == 0.0 and (ind.parts[:, 2] == 0.0).all()


@pytest.mark.parametrize("shape", ["fem1d_L2", "fem2d_L2", "fem3d_L2_k1", "fem3d_L2_k3"])
def test_closed_form_neumann(M, lib, shape):
    """(c) u = x, p = 2, Neumann data on the facets of x = 1: h = -lambda gives 0, h = 0 gives N_F = |F| lambda^r."""
    m = mesh(M, shape)
    z = np.column_stack([m.x[:, 0], np.ones(m.n)])
    right = m.F["centre"][:, 0] > 0.999
    assert right.any() and not right.all()
    for r, scale in ((2.0, None), (1.5, 0.5)):
        lam = 2.0 if scale is None else scale
        ind = M.estimate(m.geo, 2.0, z=z, r=r, scale=scale, dirichlet=~right, neumann=-lam)
        Y = XR.indicators(m.ops, m.w, m.F, m.I, z[:, 0], 2.0, r=r, scale=scale, h=np.full((m.nf, m.q), -lam), mask=right)
        assert (ind.parts[:, 2] <= KTOL * Y["parts_mag"][:, 2]).all() and ind.neumann <= KTOL * Y["totals_mag"][2]
        ind = M.estimate(m.geo, 2.0, z=z, r=r, scale=scale, dirichlet=~right)              # dirichlet= alone: h = 0 on the rest
        for e in range(m.nel):
            he = math.fsum(m.w[e * m.block:(e + 1) * m.block]) ** (1.0 / m.dim)
            want = he * math.fsum(m.F["measure"][-1 - t] * lam ** r for t in m.I["element_facets"][e] if t < 0 and right[-1 - t])
            assert abs(ind.parts[e, 2] - want) <= 8 * KTOL * want
        assert ind.neumann > 0.0


@pytest.mark.parametrize("shape", ["fem2d_L2", "fem2d_L4", "fem3d_L2_k3", "fem1d_L2"])
def test_nan_stays_where_it_feeds(M, lib, shape):
    """(d) a NaN in one element's u: that element and its facet neighbours, and the totals; (e) a NaN h on a facet the mask leaves
    out is not seen."""
    m = mesh(M, shape)
    e0 = m.nel // 2
    z = m.field(930)
    h, free = np.random.default_rng(931).standard_normal((m.nf, m.q)), m.free(932)
    clean = M.estimate(m.geo, 1.5, f=0.2, z=z, dirichlet=~free, neumann=h)
    zn = z.copy()
    zn[e0 * m.block, 0] = np.nan
    ind = M.estimate(m.geo, 1.5, f=0.2, z=zn, dirichlet=~free, neumann=h)
    compare("%s NaN u" % shape, m, lib, ind, zn, 1.5, f=np.full(m.n, 0.2), h=h, free=free)
    pairs = m.I["elements"][(m.I["elements"] == e0).any(axis=1)]
    hit = np.zeros(m.nel, dtype=bool)
    hit[e0] = True
    hit[pairs.reshape(-1).astype(int)] = True
    assert np.array_equal(np.isnan(ind.eta), hit) and np.isnan(ind.parts[e0, 0]) and np.isnan(ind.parts[hit, 1]).all()
    assert not np.isnan(np.delete(ind.parts[:, 0], e0)).any()
    assert ind.parts[~hit].tobytes() == clean.parts[~hit].tobytes()
    assert all(np.isnan(v) for v in (ind.volume, ind.jump, ind.total, ind.eta_max, ind.jump_max))
    hn = h.copy()
    hn[~free] = np.nan
    seen = M.estimate(m.geo, 1.5, f=0.2, z=z, dirichlet=~free, neumann=hn)
    assert seen.parts.tobytes() == clean.parts.tobytes() and columns(seen).tobytes() == columns(clean).tobytes()


def test_argument_errors(M, lib):
    from mgb_amd import _lib
    m = mesh(M, "fem2d_L2")
    z = M.HPCMatrix(m.field(940))
    free = m.free(941)
    with pytest.raises(ValueError, match="dirichlet"):
        M.estimate(m.geo, 2.0, z=z, neumann=1.0)
    with pytest.raises(TypeError, match="ParabolicSOL"):
        M.estimate(M.ParabolicSOL(m.geo, np.zeros(1), [z]), 2.0)
    with pytest.raises(TypeError):
        M.estimate(M.fem2d(2), 2.0, z=np.zeros((m.n, 2)))
    with pytest.raises(TypeError):
        M.estimate("sol", 2.0)
    for kw in (dict(r=0.5), dict(r=math.inf), dict(r="2"), dict(scale=math.nan), dict(u=3), dict(f=np.zeros(5)), dict(dirichlet=np.zeros(3, dtype=bool))):
        with pytest.raises(ValueError):
            M.estimate(m.geo, 2.0, z=z, **kw)
    for p in (0.5, math.nan):
        with pytest.raises(ValueError):
            M.estimate(m.geo, p, z=z)
    with pytest.raises(ValueError):
        M.estimate(m.geo, 2.0, z=np.zeros((m.n + 1, 2)))
    with pytest.raises(ValueError):
        M.estimate(m.geo, 2.0)
    with pytest.raises(ValueError, match="finite"):
        M.estimate(m.geo, 2.0, z=z, dirichlet=~free, neumann=np.full((m.nf, m.q), np.nan))
    # the C ABI refuses before anything is launched or written
    M.estimate(m.geo, 2.0, z=z)
    bd, be = m.geo._boundary_dev, m.geo.x.backend
    eta, short, other = M.HPCVector(np.full(3 * m.nel, 7.0), be), M.HPCVector(np.full(3 * m.nel - 1, 7.0), be), M.HPCVector(np.zeros(m.n), be)
    out = np.full(5, 7.0)

    def rc(zh=z._v.handle, S=3, u=0, p=2.0, pn=None, f=None, r=2.0, own=0, scale=1.0, e=eta.handle, o=out):
        return lib.mgb_estimate(bd, zh, S, u, p, pn, f, r, own, scale, None, None, e, None if o is None else _lib.dptr(o))

    assert rc() == 0
    eta = M.HPCVector(np.full(3 * m.nel, 7.0), be)
    out[:] = 7.0
    for bad in (dict(S=0), dict(S=2), dict(u=3), dict(u=-1), dict(p=0.5), dict(p=math.nan), dict(r=0.99), dict(r=math.inf),
                dict(own=1, scale=math.inf), dict(e=short.handle), dict(e=None), dict(zh=None), dict(o=None), dict(pn=short.handle),
                dict(f=short.handle), dict(e=z._v.handle, S=1), dict(zh=other.handle)):
        kw = dict(e=eta.handle)
        kw.update(bad)
        assert rc(**kw) == MGB_E_ARG, bad
    assert (eta.to_numpy() == 7.0).all() and (out == 7.0).all()
    assert lib.mgb_estimate(None, z._v.handle, 3, 0, 2.0, None, None, 2.0, 0, 1.0, None, None, eta.handle, _lib.dptr(out)) == MGB_E_ARG


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    n = g.x.shape[0]
    z = M.HPCMatrix(np.ones((n, 2)), be)
    assert M.estimate(g, 2.0, z=z).total == 0.0                           # fine while the context is one rank
    eta, out = M.HPCVector(np.full(3 * (n // 2), 7.0), be), np.full(5, 7.0)
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.estimate(g, 2.0, z=z)
        assert lib.mgb_estimate(g._boundary_dev, z._v.handle, 2, 0, 2.0, None, None, 2.0, 0, 1.0, None, None, eta.handle,
                                _lib.dptr(out)) == MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
    assert (eta.to_numpy() == 7.0).all() and (out == 7.0).all()


def solve_yardstick(M, sol, p, f=0.5, h=None, free=None, r=2.0, z=None):
    """the yardstick on the solution's own z, or on another z of the same geometry"""
    g = sol.geometry
    z = M.mpi_to_native(sol).z if z is None else z
    F = BR.facets(g)
    I = XR.interior_facets(g, F)
    w = g.w.to_numpy() if hasattr(g.w, "to_numpy") else np.asarray(g.w)
    return XR.indicators(ER.operators(g), w, F, I, z[:, 0], p, f=np.full(len(w), f), r=r, h=h, mask=free), F


_TOTALS = {}


@pytest.mark.parametrize("p", [2.0, 1.5])
@pytest.mark.parametrize("L", [2, 3])
def test_solves(M, L, p):
    """estimate(sol) of the default fem2d problem against the yardstick on the same z.  On the CPU oracle's solutions the
    yardstick gives total = 4.014 (L = 2), 1.499 (L = 3) at p = 2 and 3.134, 1.345 at p = 1.5: a factor 2.3 to spare."""
    sol = M.fem2d_mpi_solve(L=L, p=p)
    ind = M.estimate(sol, p, f=0.5)
    Y, _ = solve_yardstick(M, sol, p)
    XR.check("solve L=%d p=%g" % (L, p), Y, ind.parts, columns(ind))
    print("solve L=%d p=%g: total %.6f" % (L, p, ind.total))
    assert M.estimate(sol, p, f=M.DEFAULT_F[2]).parts.tobytes() == ind.parts.tobytes()      # amgb's f: its first entry
    _TOTALS[(L, p)] = ind.total
    if (2, p) in _TOTALS and (3, p) in _TOTALS:
        assert _TOTALS[(3, p)] < _TOTALS[(2, p)]


def test_mixed_solve(M):
    left, h2d, p = (lambda c: c[0] < -0.999), (lambda x: 0.3 + 0.2 * x[1]), 1.5
    sol = M.fem2d_mpi_solve(L=2, p=p, dirichlet=left, neumann=h2d)
    ind = M.estimate(sol, p, f=0.5, dirichlet=left, neumann=h2d)
    F = BR.facets(sol.geometry)
    sel = np.array([bool(left(c)) for c in F["centre"]])
    Y, _ = solve_yardstick(M, sol, p, h=MR.facet_values(F, sol.geometry.x.to_numpy(), h2d), free=~sel)
    XR.check("mixed solve", Y, ind.parts, columns(ind))
    assert ind.neumann > 0.0


def test_adapt_on_the_l_shape(M):
    """On the CPU oracle's solves the same loop gives 6, 10, 14 triangles (168, 280, 392 rows) and totals 1.891, 1.462, 1.252;
    the marked sets are ties of the symmetric L shape and are not compared.  Every step's z is held to the oracle's solve on the
    mesh the device loop produced, and its total to the yardstick on that oracle z."""
    L, p, theta = 2, 2.0, 0.5
    steps = M.adapt(BR.L_SHAPE, L, p, 2, theta=theta)
    assert len(steps) == 3
    counts = []
    for k, (K, sol, ind) in enumerate(steps):
        counts.append(len(K) // 3)
        XR.check_conforming(K)
        assert (XR.orientation(K) > 0).all() and abs(0.5 * XR.orientation(K).sum() - 3.0) <= KTOL
        assert len(sol.geometry.w) == 7 * 4 * counts[-1] and ind.parts.shape == (4 * counts[-1], 3)
        Y, _ = solve_yardstick(M, sol, p)
        XR.check("adapt step %d" % k, Y, ind.parts, columns(ind))
        print("adapt step %d: %d triangles, %d rows, total %.6f" % (k, counts[-1], len(sol.geometry.w), ind.total))
        # the oracle on the mesh the device loop produced (the marked sets are ties): z at the bound of every whole solve, and
        # the total within the yardstick's own bar of the yardstick on the oracle's z
        zo = O.fem2d_solve(L=L, K=K, p=p).z
        z = M.mpi_to_native(sol).z
        err = np.linalg.norm(z - zo) / np.linalg.norm(zo)
        Yo, _ = solve_yardstick(M, sol, p, z=zo)
        total_o = math.fsum(Yo["totals"][:3]) ** 0.5
        print("adapt step %d: z against the oracle %.3e, total on the oracle's z %.6f (device %.6f)" % (k, err, total_o, ind.total))
        assert z.shape == zo.shape and err < 1e-10
        assert abs(ind.total ** 2 - math.fsum(Yo["totals"][:3])) <= 4 * KTOL * math.fsum(Yo["totals_mag"])
        values = ind.coarse(L)
        marked = M.mark(values, theta)
        assert XR.dorfler_ok(values, marked, theta)
        if k + 1 < len(steps):
            assert steps[k + 1][0].tobytes() == M.refine_triangles(K, marked).tobytes()
    assert counts[0] == 6 and counts[0] < counts[1] < counts[2]
    K = steps[-1][0]
    area = np.abs(XR.orientation(K))
    smallest = XR.triangles(K)[area <= area.min() * (1 + 1e-12)]
    assert any((np.abs(t).sum(axis=1) == 0.0).any() for t in smallest)      # a triangle of the smallest area touches (0, 0)
