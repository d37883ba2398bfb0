"""sections() on the device (csrc/section.hip; contract in include/mgb_hip.h) against the host
restatement of the same per-item routine and against the numpy yardstick tests/section_reference.py.

Shapes, chosen for what can break: fem2d L=1 (one workgroup, mostly idle lanes), fem2d L=6 (2048 items, 8 workgroups: offsets
across workgroups), fem3d L=1 k=1 (6 items), L=2 k=3 (48 items, the 36-point rule, the K = 3 registers), L=5 k=1 (4096
elements, 24 576 items, 96 workgroups); a batch of 3 fields x 4 planes with a plane outside, a plane on element faces and a
NaN node in a cut element.  The finish launch beyond 256 workgroups is levelset::launch_finish, held by the isosurface tests.

Bars: against the host restatement counts, offsets and items equal, vertices, vertex values and both maxima BIT FOR BIT (both
sides run the same IEEE + - * / and sqrt with contraction off), the three sums within 1e-12 of the sum of their absolute terms
(at p = 1.5 the flow rate may also differ in pow: the same bar); against numpy the bars of tests/section_util.py.
Measured on an MI355X: 0 doubles of the pieces and no maximum differ from the host in any case; sums against the host
restatement at most 2.2e-4 of the bar; largest ratios to the yardstick's bars vertices 0.029, vertex values 0.006, sums 5.9e-4,
maxima 0.003."""
import ctypes as C

import numpy as np
import pytest

import section_util as SU
from section_util import PLANES2, PLANES3, smooth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_GEO = {}


def mesh(M, dim, L, k=0):
    """(device geometry, host mesh) of the same nodes."""
    if (dim, L, k) not in _GEO:
        geo, host = (M.fem2d_mpi(L) if dim == 2 else M.fem3d_mpi(L, k)), SU.host_mesh(dim, L, k)
        assert np.array_equal(geo.x.to_numpy().reshape(host.n, dim), host.x)
        _GEO[(dim, L, k)] = (geo, host)
    return _GEO[(dim, L, k)]


def batch(M, geo, fields, planes, **kw):
    """sections() of several fields in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(geo, np.arange(float(len(fields))), [M.HPCMatrix(np.asarray(z).reshape(len(z), -1)) for z in fields])
    sec = M.sections(sol, planes, **kw)
    assert np.array_equal(sec.ts, sol.ts)
    return sec


@pytest.mark.parametrize("p", [2.0, 1.5])
@pytest.mark.parametrize("dim,L,k", [(2, 1, 0), (2, 6, 0), (3, 1, 1), (3, 2, 3), (3, 5, 1)])
def test_device_against_host_and_numpy(M, lib, dim, L, k, p):
    geo, h = mesh(M, dim, L, k)
    assert SU.items_per_row(h) == {(2, 1): h.nel, (2, 6): 2048, (3, 1): 6, (3, 2): 48, (3, 5): 24576}[(dim, L)]
    z = np.stack([np.zeros(h.n), smooth(h.x)], axis=1)
    planes = PLANES2 if dim == 2 else PLANES3
    name = "fem%dd L=%d k=%d p=%g" % (dim, L, k, p)
    sec = M.sections(geo, planes, p=p, u=1, z=z)
    assert sec.rows.shape == (1, 7, 5) and sec.measure.shape == sec.integral.shape == sec.flux.shape == (7,) and sec.ts is None
    dev = SU.device_result(sec)
    host = SU.host_sections(lib, h, [z], planes, p=p, u=1)
    keys = ["gpu fem%dd L=%d k=%d" % (dim, L, k)]
    SU.same_as_host(name, dev, host, h, [z], planes, p=p, u=1, keys=keys)
    SU.against_reference(name + " device", dev, h, [z], planes, p=p, u=1, keys=keys)
    assert sec.hit[:4].all() and not sec.hit[4:].any() and (sec.count[:4] > 0).all()
    assert np.isnan(sec.mean[4:]).all() and np.array_equal(sec.mean[:4], sec.integral[:4] / sec.measure[:4])
    assert (sec.max[4:] == -np.inf).all() and (sec.min[4:] == np.inf).all() and (sec.min[:4] <= sec.max[:4]).all()
    d = dim
    pcs = sec.pieces(1)
    assert pcs.shape == (sec.count[1], d, d) and np.array_equal(pcs.reshape(-1, d * d), dev.row(0, 1)[0][:, :d * d])
    assert sec.values(1).shape == (sec.count[1], d) and np.array_equal(sec.values(1), dev.row(0, 1)[0][:, d * d:])
    assert np.array_equal(sec.items(1), dev.row(0, 1)[1]) and sec.items(1).dtype == np.int32
    assert np.array_equal(sec.elements(1), dev.row(0, 1)[1] // (6 if dim == 3 else 1)) and sec.elements(1).max() < h.nel
    # a plane that separates the domain: the tilted one has the closed-form measure
    full = 2 * np.sqrt(1.25) if dim == 2 else 4 * np.sqrt(1.3125)
    assert abs(sec.measure[1] - full) <= 1e-12 * full


def test_batch_with_a_plane_outside_a_plane_on_faces_and_a_nan_node(M, lib):
    """3 fields x 4 planes in one call: against the host, and bit for bit the twelve single calls; a repeated call and
    pieces=False return the same bits."""
    geo, h = mesh(M, 3, 2, 3)
    rng = np.random.default_rng(7)
    base = smooth(h.x)
    fields = [base.copy(), base + 0.8 * h.x[:, 1] ** 2, base + 0.1 * rng.standard_normal(h.n)]
    planes = [PLANES3[0], PLANES3[6], PLANES3[2], PLANES3[1]]      # z = 0.3, outside, element faces, tilted
    fields[0][64 * 7 + 21] = np.nan      # element 7 = (1, 1, 1): cut by z = 0.3 and by the tilted plane, above the faces x = 0
    sec = batch(M, geo, fields, planes)
    assert sec.measure.shape == sec.integral.shape == sec.flux.shape == sec.count.shape == sec.hit.shape == (3, 4)
    dev = SU.device_result(sec)
    host = SU.host_sections(lib, h, fields, planes)
    SU.same_as_host("batch 3 x 4", dev, host, h, fields, planes)
    SU.against_reference("batch 3 x 4 device", dev, h, fields, planes)
    assert np.isnan(sec.rows[0, [0, 2, 3]]).all() and np.isfinite(sec.rows[[1, 2]][:, [0, 2, 3]]).all()
    assert sec.hit[0, [0, 2, 3]].all() and (sec.count[0, [0, 2, 3]] > 0).all() and (sec.count[0, [0, 2, 3]] < sec.count[1, [0, 2, 3]]).all()
    assert not sec.hit[:, 1].any() and (sec.count[:, 1] == 0).all() and (sec.rows[:, 1, 3] == -np.inf).all()
    items = sec.items(3, 1)
    assert len(items) > len(np.unique(items)) > 0 and (items[1:] == items[:-1]).any() and (np.diff(items) >= 0).all()
    again = batch(M, geo, fields, planes)
    assert again.rows.tobytes() == sec.rows.tobytes() and again._piece.tobytes() == sec._piece.tobytes()
    assert np.array_equal(again._item, sec._item) and np.array_equal(again._offsets, sec._offsets)
    cheap = batch(M, geo, fields, planes, pieces=False)
    assert cheap.rows.tobytes() == sec.rows.tobytes() and np.array_equal(cheap.count, sec.count)
    with pytest.raises(ValueError, match="pieces=False"):
        cheap.pieces(0, 0)
    for b in range(3):
        for l in range(4):
            one = M.sections(geo, planes[l], z=fields[b])
            assert isinstance(one.measure, float) and isinstance(one.count, int) and isinstance(one.hit, bool)
            assert one.rows[0, 0].tobytes() == sec.rows[b, l].tobytes() and one.count == sec.count[b, l]
            assert one.pieces().tobytes() == sec.pieces(l, b).tobytes() and one.values().tobytes() == sec.values(l, b).tobytes()
            assert np.array_equal(one.items(), sec.items(l, b)) and np.array_equal(one.elements(), sec.elements(l, b))


def test_nan_in_an_uncut_element_and_inf_in_a_cut_one_2d(M, lib):
    geo, h = mesh(M, 2, 6)
    z = smooth(h.x)
    planes = [[1.0, 0.0, 0.3], [0.0, 1.0, -0.4]]
    clean = M.sections(geo, planes, z=z)
    cut = np.union1d(clean.elements(0), clean.elements(1))
    uncut = np.setdiff1d(np.arange(h.nel), cut)
    zu = z.copy()
    zu[uncut[0] * 7 + 6] = np.nan
    same = M.sections(geo, planes, z=zu)
    assert same.rows.tobytes() == clean.rows.tobytes() and same._piece.tobytes() == clean._piece.tobytes()
    zb = z.copy()
    e = int(np.setdiff1d(clean.elements(0), clean.elements(1))[0])
    zb[e * 7 + 3] = np.inf
    sec = M.sections(geo, planes, z=zb)
    dev, host = SU.device_result(sec), SU.host_sections(lib, h, [zb], planes)
    SU.same_as_host("inf node 2-D", dev, host, h, [zb], planes)
    SU.against_reference("inf node 2-D device", dev, h, [zb], planes)
    assert np.isnan(sec.rows[0, 0]).all() and sec.rows[0, 1].tobytes() == clean.rows[0, 1].tobytes()
    assert sec.count[0] == clean.count[0] - 1 and e not in sec.elements(0)
    # every cut item poisoned: nothing is emitted, the rows are NaN, and the planes still count as hitting the domain
    dead = M.sections(geo, planes + [[1.0, 0.0, 3.0]], z=np.full(h.n, np.nan))
    assert np.isnan(dead.rows[0, :2]).all() and (dead.count == 0).all() and np.isnan(dead.mean).all()
    assert dead.hit.tolist() == [True, True, False] and np.array_equal(dead.rows[0, 2], [0.0, 0.0, 0.0, -np.inf, -np.inf])


def test_argument_errors(M):
    geo, h = mesh(M, 3, 2, 3)
    z = smooth(h.x)
    pl = PLANES3[1]
    for kw, err in ((dict(planes=[0.0, 0.0, 0.0, 0.1]), ValueError), (dict(planes=[np.nan, 0.0, 1.0, 0.1]), ValueError),
                    (dict(planes=[0.0, 0.0, 1.0, np.inf]), ValueError), (dict(planes=[1.0, 0.0, 0.1]), ValueError),
                    (dict(planes=np.zeros((0, 4))), ValueError), (dict(planes=np.ones((2, 2, 4))), ValueError),
                    (dict(p=0.5), ValueError), (dict(p=np.nan), ValueError), (dict(p=np.inf), ValueError),
                    (dict(p=lambda x: 2.0), TypeError), (dict(p=np.full(h.n, 2.0)), TypeError), (dict(p="two"), TypeError),
                    (dict(u=1), ValueError), (dict(z=z[:-1]), ValueError)):
        with pytest.raises(err):
            M.sections(geo, **{**dict(planes=pl, z=z), **kw})
    with pytest.raises(TypeError, match=r"p\(x\) is not supported"):
        M.sections(geo, pl, p=lambda x: 2.0, z=z)
    with pytest.raises(TypeError):
        M.sections(z, pl)
    g1 = M.fem1d_mpi(3)
    with pytest.raises(ValueError, match="interpolate"):
        M.sections(g1, [1.0, 0.1], z=np.zeros(len(g1.w)))
    # the C entry point: MGB_E_ARG before anything is launched
    from mgb_amd import _lib
    loc, backend = M._locator_of(geo)
    zv = M.HPCVector(z, backend)
    other = M.HPCVector(z[:-1], backend)
    rows, counts, plane = np.empty(5), np.empty(1, dtype=np.int64), np.array(pl)
    lib = _lib.load()
    null_field = object()

    def rc(loc=loc, B=1, vec=zv, S=1, u=0, nc=1, pp=_lib.dptr(plane), p=2.0, out=_lib.dptr(rows),
           cnt=counts.ctypes.data_as(_lib.c_ll_p)):
        table = None if vec is None else (C.c_void_p * 1)(None if vec is null_field else vec.handle.value)
        return lib.mgb_geo_sections(loc, B, table, S, u, nc, pp, p, out, cnt, None)

    assert rc() == 0
    foreign = M.HPCVector(z, M.HPCBackend(0))      # the right length, on a second context of the same device
    bad = lambda row: _lib.dptr(np.array(row))
    for kw in (dict(loc=None), dict(vec=None), dict(vec=null_field), dict(pp=None), dict(out=None), dict(cnt=None), dict(B=0), dict(nc=0),
               dict(B=65536), dict(nc=65536), dict(S=0), dict(u=1), dict(u=-1), dict(p=0.5), dict(p=np.nan), dict(p=np.inf),
               dict(vec=other), dict(vec=foreign), dict(pp=bad([0.0, 0.0, 0.0, 0.1])), dict(pp=bad([np.inf, 0.0, 0.0, 0.1])),
               dict(pp=bad([1.0, 0.0, 0.0, np.nan]))):
        assert rc(**kw) == SU.MGB_E_ARG, kw
    assert rc(vec=foreign) == SU.MGB_E_ARG and b"another context" in lib.mgb_last_error()
    assert rc(p=0.5) == SU.MGB_E_ARG and b"p must be one finite real >= 1" in lib.mgb_last_error()
    assert rc(pp=bad([0.0, 0.0, 0.0, 0.1])) == SU.MGB_E_ARG and b"normal of every plane" in lib.mgb_last_error()
    loc1, backend1 = M._locator_of(g1)
    z1 = M.HPCVector(np.zeros(len(g1.w)), backend1)
    assert rc(loc=loc1, vec=z1) == SU.MGB_E_ARG and b"interpolate" in lib.mgb_last_error()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem3d_mpi(1, 1, backend=be)
    z = M.HPCMatrix(np.ones((8, 2)), be)
    pl = np.array([0.0, 0.0, 1.0, 0.25])
    assert abs(M.sections(g, pl, z=z).integral - 4.0) <= 1e-12 * 4.0      # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                            # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.sections(g, pl, z=z)
        rows, counts = np.zeros(5), np.zeros(1, dtype=np.int64)
        assert lib.mgb_geo_sections(loc, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 1, _lib.dptr(pl), 2.0, _lib.dptr(rows),
                                    counts.ctypes.data_as(_lib.c_ll_p), None) == SU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)


def test_solutions(M):
    """A fem3d solve, a 2-D p = 1.5 solve and a short parabolic run: shapes of every field, ts, the rows of the C entry point,
    and the snapshots of the run against their single calls."""
    from mgb_amd import _lib
    sol = M.fem3d_mpi_solve(L=2)
    planes = np.array([[1.0, 0.0, 0.0, -0.5], [1.0, 0.0, 0.0, 0.25], [1.0, 0.5, 0.25, 0.05]])
    sec = M.sections(sol, planes)
    for v in (sec.measure, sec.integral, sec.mean, sec.flux, sec.max, sec.min, sec.count, sec.hit):
        assert v.shape == (3,)
    print("fem3d L=2 solution: measure %s mean %s flux %s count %s" % (sec.measure, sec.mean, sec.flux, sec.count))
    assert sec.ts is None and sec.hit.all() and np.abs(sec.measure[:2] - 4.0).max() <= 1e-11
    assert (sec.min <= sec.mean).all() and (sec.mean <= sec.max).all()
    assert all(sec.pieces(l).shape == (sec.count[l], 3, 3) and sec.values(l).shape == (sec.count[l], 3) for l in range(3))
    loc, backend = M._locator_of(sol.geometry)
    zv, S = M._nodal_values(sol.geometry, sol.z, backend, "test")
    rows, counts = np.empty((3, 5)), np.empty(3, dtype=np.int64)
    _lib.call("mgb_geo_sections", loc, 1, (C.c_void_p * 1)(zv.handle.value), S, 0, 3, _lib.dptr(planes), 2.0, _lib.dptr(rows),
              counts.ctypes.data_as(_lib.c_ll_p), None)
    assert rows.tobytes() == sec.rows.tobytes() and np.array_equal(counts, sec.count)
    sol2 = M.fem2d_mpi_solve(L=3, p=1.5)
    lines = np.array([[1.0, 0.0, -0.5], [1.0, 0.0, 0.25], [1.0, 0.5, 0.05]])
    s2 = M.sections(sol2, lines, p=1.5)
    print("fem2d L=3 p=1.5 solution: measure %s mean %s flux %s count %s" % (s2.measure, s2.mean, s2.flux, s2.count))
    assert s2.hit.all() and np.abs(s2.measure[:2] - 2.0).max() <= 1e-11 and s2.pieces(2).shape == (s2.count[2], 2, 2)
    assert np.isfinite(s2.rows).all() and s2.values(2).shape == (s2.count[2], 2)
    par = M.parabolic_solve(M.fem3d_mpi(2, 1), h=0.5, p=2.0)
    assert len(par.u) == len(par.ts) == 3
    hist = M.sections(par, planes[:2], pieces=False)
    for v in (hist.measure, hist.integral, hist.mean, hist.flux, hist.count, hist.hit):
        assert v.shape == (len(par.ts), 2)
    print("3-D parabolic run: mean %s, flux %s" % (hist.mean.tolist(), hist.flux.tolist()))
    assert np.array_equal(hist.ts, par.ts)
    one = M.sections(par, planes[1])
    assert one.measure.shape == (3,) and one.rows[:, 0].tobytes() == hist.rows[:, 1].tobytes()
    assert one.pieces(0, 2).shape == (one.count[2], 3, 3)
    single = M.sections(par.geometry, planes[1], z=par.u[1])
    assert single.rows[0, 0].tobytes() == one.rows[1, 0].tobytes() and single.pieces().tobytes() == one.pieces(0, 1).tobytes()
