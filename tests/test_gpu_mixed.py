"""Mixed boundary conditions on the device: the Neumann load kernels (csrc/boundary.hip) against the host
restatement -- bitwise --, and amgb / parabolic_solve with dirichlet= and neumann= against the yardstick tests/mixed_reference.py
(mixed solves through the CPU oracle) and against two problems the discrete spaces hold exactly.

Bars: the load bitwise; solves at the project's solve bar ZTOL = 1e-10 relative l2 (tests/test_gpu_parity.py) on u and on all of
z; the exact cases max|u - u*| <= 1e-10 max|u*| (the oracle sits at 2e-15); parabolic snapshots at the bars of
test_gpu_parabolic_time.py (u 1e-10, all columns 1e-8)."""
import ctypes as C

import numpy as np
import pytest

import boundary_reference as BR
import mgb_oracle as O
import mixed_reference as MR

pytestmark = pytest.mark.gpu
MGB_E_ARG = -1
ZTOL = MR.ZTOL

# name -> (kind, L, k, K, nb): the distinct rows of the facet nodes; fem3d L=2 k=3 has more than 256 of them (two workgroups,
# the last partly idle), fem3d L=1 k=1 is one cube whose corner rows sit in three facets each
SHAPES = {"fem1d_L2": ("fem1d", 2, None, None, 2), "fem2d_L2": ("fem2d", 2, None, None, None),
          "fem2d_L2_Lshape": ("fem2d", 2, None, BR.L_SHAPE, None), "fem3d_L1_k1": ("fem3d", 1, 1, None, 8),
          "fem3d_L2_k3": ("fem3d", 2, 3, None, None)}
LEFT = lambda c: c[0] < -0.999


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


def device_geometry(M, kind, L, k=None, K=None):
    return M.fem1d_mpi(L) if kind == "fem1d" else M.fem2d_mpi(L, K) if kind == "fem2d" else M.fem3d_mpi(L, k)


_GEO = {}


def shape_geometry(M, name):
    if name not in _GEO:
        kind, L, k, K, _ = SHAPES[name]
        _GEO[name] = device_geometry(M, kind, L, k, K)
    return _GEO[name]


def host_load(lib, g, fields, mask):
    from mgb_amd import _lib
    nb = C.c_int()
    assert lib.mgb_geo_boundary_incidence(g._geo, C.byref(nb), None, None, None, None) == 0
    rows = np.empty(nb.value, dtype=np.int32)
    assert lib.mgb_geo_boundary_incidence(g._geo, None, None, _lib.iptr(rows), None, None) == 0
    hv = _lib.f64(fields)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    out = np.full((hv.shape[0], nb.value), 7.0)
    assert lib.mgb_geo_boundary_load_host(g._geo, hv.shape[0], _lib.dptr(hv), _lib.u8ptr(m), _lib.dptr(out)) == 0
    return rows, out


# ------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_load_kernel_matches_host_bitwise(M, lib, name, B, masked):
    g = shape_geometry(M, name)
    b = M.boundary(g)
    nf, q = b.nodes.shape
    rng = np.random.default_rng(21)
    fields = rng.standard_normal((B, nf, q))
    mask = None
    if masked:
        mask = rng.random(nf) < 0.5
        mask[0] = True
        fields[:, ~mask] = np.nan                                         # not read
    rows, want = host_load(lib, g, fields, mask)
    got = M.neumann_load(g, fields, where=mask)
    assert np.array_equal(got.rows, rows) and got.values.shape == (B, len(rows))
    if SHAPES[name][4] is not None:
        assert len(rows) == SHAPES[name][4]
    if name == "fem3d_L2_k3":
        assert 256 < len(rows) < 512
    vals = got.values.to_numpy()
    assert np.isfinite(vals).all() and vals.tobytes() == want.tobytes()
    again = M.neumann_load(g, fields, where=mask).values.to_numpy()      # a repeated call repeats
    assert again.tobytes() == vals.tobytes()
    for k in range(B):                                                    # a batch is its singles
        one = M.neumann_load(g, fields[k], where=mask)
        assert one.values.to_numpy().tobytes() == vals[k:k + 1].tobytes()
    dense = np.zeros(len(g.w))
    dense[rows] = vals[B - 1]
    assert got.dense(B - 1).to_numpy().tobytes() == dense.tobytes()
    w = g.w.to_numpy()
    _, ref, ab = MR.load(BR.facets(g), w, np.nan_to_num(fields[0]), mask)  # ... and the host restatement is within its bar of fsum
    MR.check_load(name, vals[0], ref, ab)


@pytest.mark.parametrize("name", list(SHAPES))
def test_load_add_into_a_vector_and_into_the_cost(M, name):
    g = shape_geometry(M, name)
    b = M.boundary(g)
    n, rng = len(g.w), np.random.default_rng(22)
    load = M.neumann_load(g, rng.standard_normal((2,) + b.nodes.shape))
    vals, rows = load.values.to_numpy(), load.rows
    y0 = rng.standard_normal(n)
    y = M.HPCVector(y0)
    load.add_to(y, 1)
    want = y0.copy()
    want[rows] += vals[1]
    assert y.to_numpy().tobytes() == want.tobytes()
    load.add_to(y, 0, alpha=-0.75)
    want[rows] = want[rows] + (-0.75) * vals[0]
    assert y.to_numpy().tobytes() == want.tobytes()
    y3 = M.HPCVector(np.tile(y0, 3))                                      # a strided target: row-major n x 3, column 2
    load.add_to(y3, 1, stride=3, offset=2)
    want3 = np.tile(y0, 3)
    want3[rows * 3 + 2] += vals[1]
    assert y3.to_numpy().tobytes() == want3.tobytes()
    A = M.AMG(g, p=1.5)
    c = rng.standard_normal((A.n, A.K))
    for col in (0, A.K - 1):
        A.set_c(c)
        A.add_cost_rows(load, col, k=1)
        want_c = c.copy()
        want_c[rows, col] += vals[1]
        got_c = A.get_c()
        assert got_c.tobytes() == want_c.tobytes()                        # every other entry untouched


def test_argument_errors(M, lib):
    from mgb_amd import _lib
    g = shape_geometry(M, "fem2d_L2")
    b = M.boundary(g)
    load = M.neumann_load(g, 1.0)
    nb, n = len(load.rows), len(g.w)
    bd, lv = g._boundary_dev, load.values._v.handle
    y, short, odd = M.HPCVector(n), M.HPCVector(int(load.rows[-1])), M.HPCVector(nb + 1)      # short: the last boundary row lies outside
    hv = np.ones((1,) + b.nodes.shape)
    assert lib.mgb_boundary_load(bd, 0, _lib.dptr(hv), None, lv) == MGB_E_ARG
    assert lib.mgb_boundary_load(bd, 2, _lib.dptr(hv), None, lv) == MGB_E_ARG            # out holds 1 x nb
    assert lib.mgb_boundary_load(bd, 1, None, None, lv) == MGB_E_ARG
    assert lib.mgb_boundary_load(bd, 1, _lib.dptr(hv), None, y.handle) == MGB_E_ARG
    for args in ((1, 1.0, y.handle, 1, 0), (-1, 1.0, y.handle, 1, 0), (0, np.nan, y.handle, 1, 0), (0, 1.0, y.handle, 0, 0),
                 (0, 1.0, y.handle, 2, 2), (0, 1.0, y.handle, 2, 0), (0, 1.0, y.handle, 1, -1), (0, 1.0, short.handle, 1, 0)):
        assert lib.mgb_boundary_load_add(bd, lv, *args) == MGB_E_ARG, args
    assert lib.mgb_boundary_load_add(bd, odd.handle, 0, 1.0, y.handle, 1, 0) == MGB_E_ARG   # nb + 1 is no multiple of nb
    assert np.array_equal(y.to_numpy(), np.zeros(n))                      # nothing was launched
    A = M.AMG(g, p=1.5)
    for k, alpha, col in ((1, 1.0, 0), (0, np.inf, 0), (0, 1.0, A.K), (0, 1.0, -1)):
        assert lib.mgb_amg_add_cost_rows(A.handle, bd, lv, k, alpha, col) == MGB_E_ARG
    other = M.fem2d_mpi(3)
    M.neumann_load(other, 1.0)
    assert lib.mgb_amg_add_cost_rows(A.handle, other._boundary_dev, lv, 0, 1.0, 0) == MGB_E_ARG
    with pytest.raises(ValueError, match="geometry"):
        A.add_cost_rows(M.neumann_load(other, 1.0), 0)
    with pytest.raises(ValueError, match="dirichlet"):
        M.amgb(g, neumann=1.0)
    with pytest.raises(ValueError, match="id"):
        M.amgb(g, p=2.0, dirichlet=LEFT, neumann=1.0, D=(("u", "dx"), ("u", "dy"), ("s", "id")), f=lambda x: np.array([0.0, 0.0, 1.0]))
    with pytest.raises(ValueError, match="dirichlet"):
        M.amgb(g, p=2.0, dirichlet=LEFT, state_variables=(("u", "full"), ("s", "full")))
    with pytest.raises(NotImplementedError, match="float32"):
        M.amgb(g, p=2.0, dirichlet=LEFT, T=np.float32)
    with pytest.raises(TypeError, match="neumann"):
        M.parabolic_solve(g, dirichlet=LEFT, neumann=1.0)


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem1d_mpi(2, backend=be)
    load = M.neumann_load(g, 1.0)                                         # fine while the context is one rank
    y = M.HPCVector(len(g.w), be)
    A = M.AMG(g, p=2.0)
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        for fn in (lambda: M.neumann_load(g, 1.0), lambda: M.dirichlet_on(g, LEFT, "m"), lambda: M.amgb(g, dirichlet=LEFT),
                   lambda: M.amgb(g, dirichlet=LEFT, neumann=1.0), lambda: M.parabolic_solve(g, dirichlet=LEFT),
                   lambda: M.parabolic_solve(g, dirichlet=LEFT, neumann=lambda x: 1.0)):
            with pytest.raises(NotImplementedError, match="sharded"):
                fn()
        hv = np.ones((1, 2, 1))
        assert lib.mgb_boundary_load(g._boundary_dev, 1, _lib.dptr(hv), None, load.values._v.handle) == MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
        assert lib.mgb_boundary_load_add(g._boundary_dev, load.values._v.handle, 0, 1.0, y.handle, 1, 0) == MGB_E_ARG
        assert lib.mgb_amg_add_cost_rows(A.handle, g._boundary_dev, load.values._v.handle, 0, 1.0, 0) == MGB_E_ARG
    finally:
        be.set_comm(0, 1, None)


# ------------------------------------------------------------------------------------------------------------ stationary
H_2D = lambda x: 0.3 + 0.2 * x[1]
# (kind, L, k, p, h): exactly the cases the oracle was checked to converge on
SOLVES = [("fem1d", 3, None, 1.5, lambda x: 0.7), ("fem2d", 2, None, 1.5, H_2D), ("fem2d", 2, None, 3.0, H_2D),
          ("fem2d", 3, None, 2.0, H_2D), ("fem3d", 2, 1, 1.5, 0.0)]


@pytest.mark.parametrize("kind,L,k,p,h", SOLVES, ids=["fem1d_L3_p1.5", "fem2d_L2_p1.5", "fem2d_L2_p3", "fem2d_L3_p2", "fem3d_L2_k1_p1.5"])
def test_solve_matches_oracle(M, kind, L, k, p, h):
    ref = MR.cached(("stationary", kind, L, k, p), lambda: MR.stationary(
        MR.oracle_geometry(kind, L, k), p, LEFT, h=(lambda x: 0.0) if not callable(h) else h))
    solve = getattr(M, kind + "_mpi_solve")
    sol = solve(L=L, p=p, dirichlet=LEFT, neumann=h, **({"k": k} if kind == "fem3d" else {}))
    z = M.mpi_to_native(sol).z
    gu, gz = MR.rel(z[:, 0], ref["z"][:, 0]), MR.rel(z, ref["z"])
    print("%s L=%d p=%g: newton steps %d (oracle %d), rel l2 gap u %.3e, z %.3e" % (kind, L, p, int(sol.SOL_main["its"].sum()),
                                                                                  ref["its"], gu, gz))
    rows = ref["dirichlet_rows"]
    assert len(rows) and z[rows, 0].tobytes() == ref["g"][rows, 0].tobytes()      # u on the Dirichlet rows equals g bitwise
    free = np.setdiff1d(np.unique(M.boundary(sol.geometry).nodes), rows)
    assert np.abs(z[free, 0] - ref["g"][free, 0]).max() > 1e-3                     # ... and the free boundary moved
    assert gu < ZTOL
    assert gz < ZTOL


def test_every_facet_selected_is_the_plain_solve(M):
    plain = M.fem2d_mpi_solve(L=2, p=1.5)
    mixed = M.fem2d_mpi_solve(L=2, p=1.5, dirichlet=lambda c: True)
    assert M.mpi_to_native(mixed).z.tobytes() == M.mpi_to_native(plain).z.tobytes()
    assert np.array_equal(mixed.SOL_main["its"], plain.SOL_main["its"])
    g = mixed.geometry                                                    # built once per geometry and selection
    names = set(g.subspaces)
    M.amgb(g, p=1.5, dirichlet=np.ones(len(M.boundary(g)), dtype=bool))
    assert set(g.subspaces) == names
    name = M.dirichlet_on(g, LEFT, "left")                                # an explicit name is found again, and usable directly
    a = M.amgb(g, p=2.0, dirichlet=LEFT)
    assert set(g.subspaces) == names | {"left"}
    b_ = M.amgb(g, p=2.0, state_variables=(("u", name), ("s", "full")))
    assert M.mpi_to_native(a).z.tobytes() == M.mpi_to_native(b_).z.tobytes()
    for l, S in enumerate(g.subspaces["left"]):
        assert isinstance(S, M.HPCSparseMatrix) and MR.same_matrix(S.host, MR.mixed_subspaces(g, np.array([LEFT(c) for c in M.boundary(g).centre]))[l])


U_2D = lambda x: x[0] ** 2 + 0.5 * x[1] ** 2 + 0.3 * x[0] * x[1]
GRAD_2D = lambda x: np.array([2.0 * x[0] + 0.3 * x[1], x[1] + 0.3 * x[0]])


@pytest.mark.parametrize("L", [1, 2, 3])
def test_exact_solution_2d(M, L):
    """p = 2, u* = x^2 + y^2 / 2 + 0.3 x y, f = (6, 0, 0, 1), Dirichlet u* on x = -1, h = -2 grad u* . n on the other sides: P2
    and Simpson hold this exactly.  The start is away from u* off the Dirichlet side."""
    g = M.fem2d_mpi(L)
    b, x = M.boundary(g), g.x.to_numpy()
    h = np.array([[-2.0 * GRAD_2D(x[i]) @ b.normal[f] for i in b.nodes[f]] for f in range(len(b))])
    sol = M.amgb(g, p=2.0, f=lambda xi: np.array([6.0, 0.0, 0.0, 1.0]), g=lambda xi: np.array([U_2D(xi) + 0.5 * (xi[0] + 1.0), 100.0]),
                 dirichlet=LEFT, neumann=h)
    u, want = M.mpi_to_native(sol).z[:, 0], np.array([U_2D(xi) for xi in x])
    gap = np.abs(u - want).max()
    print("fem2d L=%d: max|u - u*| = %.3e (bar %.3e)" % (L, gap, 1e-10 * np.abs(want).max()))
    assert gap <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("L", [2, 3])
def test_exact_solution_1d(M, L):
    """p = 2, f = (0, 0, 1), u(-1) = -1.5, h = -3 at x = 1: u* = 1.5 x."""
    sol = M.fem1d_mpi_solve(L=L, p=2.0, f=lambda xi: np.array([0.0, 0.0, 1.0]), g=lambda xi: np.array([1.5 * xi[0] + 0.5 * (xi[0] + 1.0), 10.0]),
                            dirichlet=LEFT, neumann=-3.0)
    u, want = M.mpi_to_native(sol).z[:, 0], 1.5 * sol.geometry.x.to_numpy()[:, 0]
    gap = np.abs(u - want).max()
    print("fem1d L=%d: max|u - u*| = %.3e (bar %.3e)" % (L, gap, 1e-10 * np.abs(want).max()))
    assert gap <= 1e-10 * np.abs(want).max()


# ------------------------------------------------------------------------------------------------------------ parabolic
TS = np.array([0.0, 0.25, 0.65, 0.75])
H_T = lambda t, x: 0.3 + t * x[1]


@pytest.mark.parametrize("p", [1.5, 2.0])
def test_parabolic_matches_reference_loop(M, p):
    u_ref, lift_ref = MR.cached(("parabolic", p), lambda: MR.parabolic(O.fem2d(2), p, TS, LEFT, H_T))
    g = M.fem2d_mpi(2)
    sol = M.parabolic_solve(g, p=p, ts=TS, dirichlet=LEFT, neumann=H_T)
    nat = M.mpi_to_native(sol)
    assert len(nat.u) == len(TS) and np.array_equal(sol.ts, TS)
    gaps = [(MR.rel(uk[:, 0], rk[:, 0]), MR.rel(uk, rk)) for uk, rk in zip(nat.u, u_ref)]
    print("fem2d L=2 p=%g lifts %r reference %r; snapshot gaps (u, all columns): %s" % (
        p, sol.lift.tolist(), lift_ref.tolist(), ", ".join("(%.2e, %.2e)" % ab for ab in gaps)))
    b = M.boundary(g)
    pinned = np.unique(b.nodes[np.array([LEFT(c) for c in b.centre])])
    for uk in nat.u[1:]:
        assert uk[pinned, 0].tobytes() == nat.u[0][pinned, 0].tobytes()  # u on the Dirichlet rows stays at g
    for (gu, ga), uk, rk in zip(gaps, nat.u, u_ref):
        assert uk.shape == rk.shape
        assert gu < 1e-10
        assert ga < 1e-8


def test_parabolic_static_load_is_the_constant_timed_load(M):
    g = M.fem2d_mpi(2)
    a = M.parabolic_solve(g, p=1.5, ts=TS, dirichlet=LEFT, neumann=lambda x: 0.3 + 0.5 * x[1])
    b = M.parabolic_solve(g, p=1.5, ts=TS, dirichlet=LEFT, neumann=lambda t, x: 0.3 + 0.5 * x[1])
    for ua, ub in zip(a.u, b.u):
        assert ua.to_numpy().tobytes() == ub.to_numpy().tobytes()
    assert np.array_equal(a.lift, b.lift)
    c = M.parabolic_solve(g, p=1.5, ts=TS, dirichlet=LEFT)                # no load: another solution
    assert MR.rel(c.u[-1].to_numpy()[:, 0], a.u[-1].to_numpy()[:, 0]) > 1e-3
