"""energy() and flux() on the device (csrc/energy.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-node routine and against the numpy yardstick tests/energy_reference.py.

Shapes are those of test_gpu_parabolic_time.py, for the same reasons: fem1d L=2 (n = 8), fem2d L=2 (n = 56), fem3d L=1 (Q3: the
largest element block, n = 64 is below one workgroup) and fem2d L=4 (n = 896, three and a half workgroups of 256: the
cross-workgroup pass of the reduction and a partly idle last workgroup).

Bars (tests/energy_reference.py): sums and extrema within KTOL = 1e-12 relative, flux within KTOL relative to flux_max; bit for
bit where the contract says so (a batch against its fields one by one, the flux at p = 2 against the gradient, the fields next to
a non-finite one)."""
import ctypes as C

import numpy as np
import pytest

import energy_reference as ER

pytestmark = pytest.mark.gpu
MGB_E_ARG = -1
SHAPES = {"fem1d_L2": 8, "fem2d_L2": 56, "fem3d_L1": 64, "fem2d_L4": 896}


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


class Mesh:
    """A device geometry of SHAPES with the host handle of the same mesh and the numpy pieces of the yardstick."""

    def __init__(self, M, shape):
        kind, L, _ = ER.GEOMETRIES[shape]
        self.name = shape
        self.geo = getattr(M, kind + "_mpi")(L)
        self.host = ER.HostGeo(shape)
        self.x, self.w = self.geo.x.to_numpy().reshape(self.host.n, -1), self.geo.w.to_numpy()
        self.n, self.dim, self.block = self.host.n, self.host.dim, self.host.block
        self.ops = ER.operators(self.geo)
        assert self.n == SHAPES[shape] and np.array_equal(self.x, self.host.x) and np.array_equal(self.w, self.host.w)

    def fields(self, B, seed):
        """B distinct random (n, 3) fields, broken across elements, and (B, n) forcing: a wrong stride or pointer shows."""
        rng = np.random.default_rng(seed)
        return [rng.standard_normal((self.n, 3)) for _ in range(B)], rng.standard_normal((B, self.n))

    def grad_p(self, u, p):
        g = ER.gradient(self.ops, u)
        return np.sqrt((g * g).sum(axis=1)) ** p


_MESHES = {}


def mesh(M, shape):
    if shape not in _MESHES:
        _MESHES[shape] = Mesh(M, shape)
    return _MESHES[shape]


def rows(e):
    """(B, 5) in the column order of the C ABI from an Energy."""
    return np.column_stack([np.atleast_1d(v) for v in (e.gradient, e.load, e.slack_gap, e.flux_max, -np.asarray(e.margin))])


def batch(M, m, zs, p, f=None, **kw):
    """energy() of the fields zs in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(m.geo, np.arange(float(len(zs))), [M.HPCMatrix(z) for z in zs])
    e = M.energy(sol, p, f=f, **kw)
    assert np.array_equal(e.ts, sol.ts) and all(np.shape(v) == (len(zs),) for v in (e.gradient, e.load, e.total, e.slack_gap,
                                                                                    e.margin, e.flux_max))
    assert np.array_equal(e.total, e.gradient + e.load, equal_nan=True)
    return rows(e)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("p", ER.P_VALUES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_against_host_and_numpy(M, lib, shape, p, B):
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    zs, f = m.fields(B, 300 + B)
    name = "%s p=%s B=%d" % (shape, p, B)
    if B == 1:
        e = M.energy(m.geo, pv, f=f[0], z=zs[0])
        assert all(isinstance(v, float) for v in (e.gradient, e.load, e.total, e.slack_gap, e.margin, e.flux_max)) and e.ts is None
        assert e.total == e.gradient + e.load
        got = rows(e)
    else:
        got = batch(M, m, zs, pv, f=f)
    host, host_flux = ER.host_energy(lib, m.host, zs, pv, f=f)
    want = np.array([ER.energy(m.ops, m.w, zs[b], pv, f[b]) for b in range(B)])
    ER.check(name + " device against numpy", got, want)
    ER.check(name + " device against host", got, host)
    for b in range(B):
        fl = M.flux(m.geo, pv, z=zs[b])
        assert isinstance(fl, M.HPCMatrix) and fl.shape == (m.n, m.dim)
        fl = fl.to_numpy()
        ER.check_flux(name + " flux against numpy", fl, ER.flux(m.ops, zs[b][:, 0], pv), want[b, 3])
        ER.check_flux(name + " flux against host", fl, host_flux[b], want[b, 3])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_flux_at_p_2_is_the_gradient_bit_for_bit(M, shape):
    """At p = 2 the flux is the gradient, untouched.  The only other public gradient on the device is interpolate()'s, which at a
    node evaluates the lowest element containing the point: the node's own element for a SUBSET of the nodes only (at least one
    per element, all interior ones among them).  On that subset the two agree in every bit; the other nodes are held to numpy's
    gradient at 1e-12.  And inside the flux kernel: under an array p(x), whatever the other
    nodes' exponents are, the rows with p_i = 2 carry the bits of the p = 2 flux and the rows with p_i = 1 those of the p = 1
    flux; a scalar 2 and a constant array of 2 are the same."""
    m = mesh(M, shape)
    z = m.fields(1, 350)[0][0]
    pn = ER.exponent("array", m.x)
    assert (pn == 2.0).sum() >= 1 and (pn == 1.0).sum() >= 1
    f2, f1, fa = (M.flux(m.geo, pv, z=z).to_numpy() for pv in (2.0, 1.0, pn))
    _, grads, elem = M.interpolate(m.geo, m.x, z=z[:, 0].copy(), grad=True, return_element=True)
    own = elem == np.arange(m.n) // m.block
    print("%s: %d of %d nodes are located in their own element; the flux at p = 2 differs from the gradient at %d of them"
          % (shape, own.sum(), m.n, (f2[own] != grads[own, 0, :]).any(axis=1).sum()))
    assert own.sum() >= m.n // m.block
    assert np.array_equal(f2[own], grads[own, 0, :])
    assert np.array_equal(fa[pn == 2.0], f2[pn == 2.0]) and np.array_equal(fa[pn == 1.0], f1[pn == 1.0])
    assert np.array_equal(M.flux(m.geo, np.full(m.n, 2.0), z=z).to_numpy(), f2)
    ER.check_flux(shape + " gradient against numpy", f2, ER.gradient(m.ops, z[:, 0]), np.abs(f2).max())


@pytest.mark.parametrize("p", [1.5, "array"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_batch_is_the_singles(M, shape, p):
    """The reduction order may not depend on the batch index or on B: three fields in one call give, bit for bit, the results of
    three calls -- with per-field forcing, with one shared forcing row and without forcing."""
    m = mesh(M, shape)
    pv = ER.exponent(p, m.x)
    zs, f = m.fields(3, 310)
    for kind in ("per field", "shared", "none"):
        fb = {"per field": f, "shared": f[1], "none": None}[kind]
        got = batch(M, m, zs, pv, f=fb, u=1, s=0)
        for b in range(3):
            fk = None if fb is None else (fb[b] if kind == "per field" else fb)
            single = rows(M.energy(m.geo, pv, f=fk, z=M.HPCMatrix(zs[b]), u=1, s=0))
            assert got[b].tobytes() == single[0].tobytes(), (kind, b, got[b], single[0])
    again = batch(M, m, zs[::-1], pv, f=f[::-1], u=1, s=0)
    assert again[::-1].tobytes() == batch(M, m, zs, pv, f=f, u=1, s=0).tobytes()


@pytest.mark.parametrize("p", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_zero_gradient(M, shape, p):
    """u constant on one element: flux rows exactly 0 there (not NaN, not Inf), energy contribution 0.  The gradient is
    ElemBasis's sum over the nodal values, so it is exactly 0 where every product is: for the constant 0 on every element kind
    and, in 1-D (derivative weights -1, 1), for any constant -- see test_energy_host.py."""
    m = mesh(M, shape)
    e_last = m.n // m.block - 1
    for const in (0.0, 0.625) if m.dim == 1 else (0.0,):
        for e in (0, e_last):
            z = m.fields(1, 320)[0][0]
            sl = slice(e * m.block, (e + 1) * m.block)
            z[sl, 0] = const
            fl = M.flux(m.geo, p, z=z).to_numpy()
            assert np.array_equal(fl[sl], np.zeros((m.block, m.dim))) and np.isfinite(fl).all()
            w0 = m.w.copy()
            w0[sl] = 0.0                                                  # the yardstick without the element: it contributes 0
            got = M.energy(m.geo, p, z=z)
            want = ER.energy(m.ops, w0, z, p)[0]
            print("%s p=%g element %d constant %g: gradient energy %.17g, without the element %.17g" % (shape, p, e, const, got.gradient, want))
            assert np.isfinite(rows(got)).all() and abs(got.gradient - want) <= ER.KTOL * want


@pytest.mark.parametrize("case", ["node_0", "last_node", "nothing"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_margin_placement(M, shape, case):
    """The single node outside the cone at node 0, at node n - 1, at none (test_gpu_parabolic_time.py:
    test_placement_of_the_violation): the margin is negative exactly in the first two, and it is numpy's."""
    p = 1.5
    m = mesh(M, shape)
    rng = np.random.default_rng(5)
    u = rng.standard_normal(m.n)
    u /= m.grad_p(u, 1.0).max()                                           # largest gradient 1: P <= 1 next to a margin of 1/2, so
    P = m.grad_p(u, p)                                                    # P - s keeps its digits and KTOL on the margin is fair
    s = P + 0.5 + rng.random(m.n)
    j = {"node_0": 0, "last_node": m.n - 1, "nothing": None}[case]
    if j is not None:
        s[j] = P[j] - 0.5
    z = np.column_stack([u, s])
    e = M.energy(m.geo, p, z=z)
    want = ER.energy(m.ops, m.w, z, p)
    print("%s %s: margin %.17g (numpy %.17g), slack gap %.17g" % (shape, case, e.margin, -want[4], e.slack_gap))
    assert (e.margin < 0.0) == (j is not None)
    assert abs(e.margin + want[4]) <= ER.KTOL * abs(want[4])
    if j is not None:
        assert abs(e.margin + 0.5) <= ER.KTOL
    ER.check("%s %s" % (shape, case), rows(e), want)


def test_non_finite_input(M):
    """A NaN or an Inf at u[n - 1], u[300] or s[7] makes that field's results NaN -- never a dropped term, never a silent max --;
    the other two fields of the batch keep their bits."""
    m = mesh(M, "fem2d_L4")
    zs, f = m.fields(3, 330)
    clean = batch(M, m, zs, 1.5, f=f)
    assert np.isfinite(clean).all()
    for (row, col), bad in (((m.n - 1, 0), np.nan), ((300, 0), np.inf), ((7, 2), -np.inf), ((7, 2), np.nan), ((300, 0), -np.inf)):
        for which in (0, 1, 2):
            broken = [z.copy() for z in zs]
            broken[which][row, col] = bad
            got = batch(M, m, broken, 1.5, f=f)
            assert np.isnan(got[which]).all(), (row, col, bad, which, got)
            for other in set(range(3)) - {which}:
                assert got[other].tobytes() == clean[other].tobytes()
        single = M.energy(m.geo, 1.5, f=f[0], z=broken[2])
        assert all(np.isnan(v) for v in (single.gradient, single.load, single.total, single.slack_gap, single.margin, single.flux_max))
    fb = f.copy()
    fb[1, m.n - 1] = np.nan                                               # ... and in the forcing
    got = batch(M, m, zs, 1.5, f=fb)
    assert np.isnan(got[1]).all() and got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()


def test_stationary_solution(M):
    sol = M.fem2d_mpi_solve(L=3, p=1.5)
    dim = 2
    forcing = lambda x: M.DEFAULT_F[dim](x)[0]                             # the forcing component of the default f
    e = M.energy(sol, 1.5, f=forcing)
    nat = M.mpi_to_native(sol)
    ops = ER.operators(nat.geometry)
    fx = np.array([forcing(xi) for xi in nat.geometry.x])
    want = ER.energy(ops, nat.geometry.w, nat.z, 1.5, fx)
    print("fem2d L=3 p=1.5: gradient %.17g load %.17g total %.17g (numpy %.17g) slack gap %.17g margin %.6e flux_max %.17g"
          % (e.gradient, e.load, e.total, want[0] + want[1], e.slack_gap, e.margin, e.flux_max))
    assert abs(e.total - (want[0] + want[1])) <= ER.KTOL * abs(want[0] + want[1])
    assert abs(e.gradient - want[0]) <= ER.KTOL * want[0] and abs(e.load - want[1]) <= ER.KTOL * abs(want[1])
    assert abs(e.flux_max - want[3]) <= ER.KTOL * want[3]
    # the solve leaves s within about 1 / t of |grad u|^p, so s - P cancels almost all digits: sign, not value, is what holds
    print("fem2d L=3 p=1.5: slack gap off numpy's by %.3e, margin by %.3e" % (abs(e.slack_gap - want[2]), abs(e.margin + want[4])))
    assert e.margin > 0.0 and e.slack_gap >= 0.0
    assert M.mpi_to_native(e) is e
    fl = M.flux(sol, 1.5)
    assert isinstance(fl, M.HPCMatrix) and fl.shape == nat.geometry.x.shape
    print("fem2d L=3 p=1.5: flux off numpy's by %.3e (flux_max %.6e)" % (np.abs(fl.to_numpy() - ER.flux(ops, nat.z[:, 0], 1.5)).max(), want[3]))


def test_parabolic_solution(M):
    """One call on the five snapshots equals five single calls, bit for bit.  The energies are printed, not held to decay: what
    the discrete scheme provably decreases is the slack energy plus the step term, up to the barrier tolerance."""
    sol = M.parabolic_solve(M.fem1d_mpi(3), h=0.25, p=2.0)
    e = M.energy(sol, 2.0, f=0.5, s=2)
    assert len(sol.u) == 5 and np.array_equal(e.ts, sol.ts)
    for name in ("gradient", "load", "total", "slack_gap", "margin", "flux_max"):
        v = getattr(e, name)
        assert isinstance(v, np.ndarray) and v.shape == (5,) and np.isfinite(v).all()
        print("parabolic fem1d L=3 p=2 %-10s %s" % (name, " ".join("%.12g" % t for t in v)))
    singles = np.vstack([rows(M.energy(sol.geometry, 2.0, f=0.5, s=2, z=uk)) for uk in sol.u])
    assert rows(e).tobytes() == singles.tobytes()
    x = sol.geometry.x.to_numpy().reshape(-1, 1)
    timed = M.energy(sol, 2.0, f=lambda t, xi: 0.5 + t * xi[0], s=2)
    table = np.array([[0.5 + t * xi[0] for xi in x] for t in sol.ts])
    assert rows(M.energy(sol, 2.0, f=table, s=2)).tobytes() == rows(timed).tobytes()
    assert np.array_equal(timed.gradient, e.gradient) and timed.load[0] == e.load[0] and not np.array_equal(timed.load[1:], e.load[1:])
    for k in (0, -1, 2):
        fk = M.flux(sol, 2.0, k=k).to_numpy()
        assert np.array_equal(fk, M.flux(sol.geometry, 2.0, z=sol.u[k]).to_numpy()) and fk.shape == (x.shape[0], 1)


def test_errors(M, lib):
    from mgb_amd import _lib
    m = mesh(M, "fem1d_L2")
    g, n = m.geo, m.n
    z = m.fields(1, 340)[0][0]
    for bad in (0.5, np.nan, np.inf, -1.0, np.full(n, 0.5), np.r_[np.full(n - 1, 2.0), np.nan], np.full(n + 1, 2.0), lambda x: 0.0):
        with pytest.raises(ValueError, match="p"):
            M.energy(g, bad, z=z)
        with pytest.raises(ValueError, match="p"):
            M.flux(g, bad, z=z)
    with pytest.raises(ValueError, match="same column"):
        M.energy(g, 2.0, z=z, u=1, s=1)
    with pytest.raises(ValueError, match="same column"):
        M.energy(g, 2.0, z=z, u=2)                                        # s = -1 is column 2
    for kw in (dict(u=3), dict(s=-4), dict(s=3)):
        with pytest.raises(ValueError, match="column"):
            M.energy(g, 2.0, z=z, **kw)
    with pytest.raises(TypeError, match="column"):
        M.energy(g, 2.0, z=z, u=0.5)
    with pytest.raises(ValueError, match="z"):
        M.energy(g, 2.0)                                                  # a Geometry needs z=
    with pytest.raises(ValueError, match="column"):
        M.energy(g, 2.0, z=z[:, :1])                                      # no slack column
    with pytest.raises(ValueError, match="f"):
        M.energy(g, 2.0, z=z, f=np.zeros(n + 1))
    with pytest.raises(TypeError, match="f"):
        M.energy(g, 2.0, z=z, f=lambda t, x: 0.0)                         # f(t, x) goes with a ParabolicSOL
    sol = M.ParabolicSOL(g, np.arange(3.0), [M.HPCMatrix(z)] * 3)
    for bad in (np.zeros((2, n)), np.zeros((4, n)), np.zeros((3, n + 1))):
        with pytest.raises(ValueError, match="f"):
            M.energy(sol, 2.0, f=bad)                                     # three snapshots need three rows
    with pytest.raises(ValueError, match="z="):
        M.energy(sol, 2.0, z=z)
    with pytest.raises(ValueError, match="k"):
        M.flux(sol, 2.0, k=3)
    # the C ABI: MGB_E_ARG before anything is launched
    loc, backend = M._locator_of(g)
    zv, short = M.HPCVector(z, backend), M.HPCVector(np.zeros(3 * n - 1), backend)
    fv, out = M.HPCVector(np.zeros(n), backend), np.zeros((3, 5))
    table = lambda *vs: (C.c_void_p * len(vs))(*[v.handle.value for v in vs])
    E = lambda B, tab, S, u, s, p, pn, f, rows_: lib.mgb_geo_field_energy(loc, B, tab, S, u, s, p, pn, f, rows_, _lib.dptr(out))
    assert E(1, table(zv), 3, 0, 2, 2.0, None, fv.handle, 1) == 0
    for p in (0.5, np.nan, np.inf):
        assert E(1, table(zv), 3, 0, 2, p, None, None, 1) == MGB_E_ARG
    assert E(1, table(zv), 3, 3, 2, 2.0, None, None, 1) == MGB_E_ARG and E(1, table(zv), 3, -1, 2, 2.0, None, None, 1) == MGB_E_ARG
    assert E(1, table(zv), 3, 0, 3, 2.0, None, None, 1) == MGB_E_ARG and E(1, table(zv), 3, 0, -1, 2.0, None, None, 1) == MGB_E_ARG
    assert E(1, table(zv), 3, 1, 1, 2.0, None, None, 1) == MGB_E_ARG and b"same column" in lib.mgb_last_error()
    assert E(0, table(zv), 3, 0, 2, 2.0, None, None, 1) == MGB_E_ARG and E(-1, table(zv), 3, 0, 2, 2.0, None, None, 1) == MGB_E_ARG
    assert E(1, table(short), 3, 0, 2, 2.0, None, None, 1) == MGB_E_ARG
    assert E(2, table(zv, short), 3, 0, 2, 2.0, None, None, 1) == MGB_E_ARG
    assert E(1, table(zv), 2, 0, 1, 2.0, None, None, 1) == MGB_E_ARG       # 3 n values are not n x 2
    assert E(1, table(zv), 3, 0, 2, 2.0, short.handle, None, 1) == MGB_E_ARG
    assert E(1, table(zv), 3, 0, 2, 2.0, None, short.handle, 1) == MGB_E_ARG
    assert E(2, table(zv, zv), 3, 0, 2, 2.0, None, fv.handle, 2) == MGB_E_ARG      # two rows of forcing are 2 n values
    assert E(3, table(zv, zv, zv), 3, 0, 2, 2.0, None, fv.handle, 2) == MGB_E_ARG
    fl = M.HPCVector(n, backend)
    F = lambda zz, S, u, p, pn, o: lib.mgb_geo_field_flux(loc, zz.handle, S, u, p, pn, o.handle)
    assert F(zv, 3, 0, 2.0, None, fl) == 0
    assert F(zv, 3, 3, 2.0, None, fl) == MGB_E_ARG and F(zv, 3, 0, 0.5, None, fl) == MGB_E_ARG and F(zv, 3, 0, np.nan, None, fl) == MGB_E_ARG
    assert F(short, 3, 0, 2.0, None, fl) == MGB_E_ARG and F(zv, 3, 0, 2.0, None, short) == MGB_E_ARG
    assert F(zv, 3, 0, 2.0, short.handle, fl) == MGB_E_ARG
    backend.synchronize()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    n = g.x.shape[0]
    z = M.HPCMatrix(np.ones((n, 2)), be)
    assert M.energy(g, 2.0, z=z).gradient == 0.0                          # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.energy(g, 2.0, z=z)
        with pytest.raises(NotImplementedError, match="sharded"):
            M.flux(g, 2.0, z=z)
        out = np.zeros((1, 5))
        fl = M.HPCVector(n, be)
        assert lib.mgb_geo_field_energy(loc, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 1, 2.0, None, None, 1, _lib.dptr(out)) == MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
        assert lib.mgb_geo_field_flux(loc, z._v.handle, 2, 0, 2.0, None, fl.handle) == MGB_E_ARG
    finally:
        be.set_comm(0, 1, None)
