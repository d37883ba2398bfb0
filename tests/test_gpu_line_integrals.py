"""line_integrals() and project() on the device (csrc/ray.hip; contract in include/mgb_hip.h) against the
host restatement of the same per-segment routine and against the np.longdouble yardstick tests/ray_reference.py.

Shapes, chosen for what can break: m = 1, 63, 64, 65 and 300 segments (one lane, a wave short of one, a full wave, one lane in
a second workgroup, several workgroups with an idle tail) at the workgroup sizes 64, 128 and 256, on fem2d L=1 (2 elements),
fem2d L=4, the L shape, fem3d L=1 k=1, L=2 k=3 (the 64-term basis, the 6-point rule) and L=3 k=2.  The segments mix the named
degenerate ones (in faces, along edges, through vertices, within tau of a face, inside one element, outside) with seeded random
chords, one in eight wholly outside.

Bars: against the host restatement counts, offsets and piece elements equal, t0, t1, the piece integrals and all eight columns
BIT FOR BIT at p = 1 and 2 (both sides run the same IEEE + - * / and sqrt with contraction off); at p = 1.5 along and across
within 4 eps sum |terms| (pow) and everything else bit for bit; against numpy the bars of tests/ray_reference.py.
Measured on an MI355X: every count, offset, element, piece and column equal to the host's in every case; along / across at
p = 1.5 at most 0.546 of the pow bar; no ray undecided (0 of 300 per mesh, 0 of 70 in the batch, the 12 named degenerate rays
included); largest ratios to the yardstick's bars length 0.149, integral 0.014, along 0.004, across 0.008, max 0.010,
min 0.011, enter 0.024, leave 0.095, piece ends 0.121, piece integrals 0.057."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as MC
import ray_util as RU
import section_util as SU

smooth = RU.smooth
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


_GEO = {}


def mesh(M, kind, L, k=0):
    """(device geometry, host mesh) of the same nodes."""
    if (kind, L, k) not in _GEO:
        geo = M.fem3d_mpi(L, k) if kind == "fem3d" else M.fem2d_mpi(L, MC.LSHAPE if kind == "lshape" else None)
        host = RU.host_mesh(kind, L, k)
        assert np.array_equal(geo.x.to_numpy().reshape(host.n, host.dim), host.x)
        _GEO[(kind, L, k)] = (geo, host)
    return _GEO[(kind, L, k)]


def batch(M, geo, fields, a, b, **kw):
    """line_integrals() of several fields in ONE call: a ParabolicSOL is the public way to hand over a batch."""
    sol = M.ParabolicSOL(geo, np.arange(float(len(fields))), [M.HPCMatrix(np.asarray(z).reshape(len(z), -1)) for z in fields])
    res = M.line_integrals(sol, a, b, **kw)
    assert np.array_equal(res.ts, sol.ts)
    return res


@pytest.mark.parametrize("kind,L,k", RU.MESHES)
def test_device_against_host_and_numpy(M, lib, kind, L, k):
    """m = 300 at every exponent and workgroup size; the yardstick once per exponent."""
    geo, h = mesh(M, kind, L, k)
    a, b = RU.rays(h.dim, 300)
    z = np.stack([np.zeros(h.n), smooth(h.x)], axis=1)
    for p in (1.0, 1.5, 2.0):
        name = "%s p=%g" % (h.name, p)
        host = RU.host_line_integrals(lib, h, [z], a, b, p=p, u=1)
        first = None
        for wg in (None, 64, 128, 256):
            res = M.line_integrals(geo, a, b, p=p, u=1, z=z, pieces=True, workgroup=wg)
            dev = RU.device_result(res)
            RU.same_as_host("%s wg=%s" % (name, wg), dev, host, h, [z], a, b, p=p, u=1)
            if first is None:
                first = dev
                RU.against_reference(name + " device", dev, h, [z], a, b, p=p, u=1)
            else:      # the result does not depend on the workgroup size, pow included
                assert dev.rows.tobytes() == first.rows.tobytes() and dev.piece.tobytes() == first.piece.tobytes()
        assert res.rows.shape == (1, 300, 8) and res.length.shape == res.count.shape == res.mean.shape == (300,) and res.ts is None
        assert (res.across is None) == (h.dim == 3)
        hit = res.count > 0
        assert hit.any() and (~hit).any() and np.isnan(res.mean[~hit]).all() and np.isnan(res.enter[~hit]).all()
        assert np.array_equal(res.mean[hit], res.integral[hit] / res.length[hit]) and (res.min[hit] <= res.max[hit]).all()
        assert (res.max[~hit] == -np.inf).all() and (res.min[~hit] == np.inf).all() and (res.length[~hit] == 0).all()
        i = int(np.flatnonzero(hit)[-1])
        elems, t0, t1, integ = res.pieces(i)
        assert elems.dtype == np.int32 and len(elems) == res.count[i] and np.array_equal(elems, dev.row(0, i)[0])
        assert np.array_equal(np.stack([t0, t1, integ], axis=1), dev.row(0, i)[1]) and (t1 > t0).all()


@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("kind,L,k", RU.MESHES)
def test_partial_waves_and_workgroups(M, lib, kind, L, k, m):
    """Every mesh, exponent and workgroup size at the sizes around one wave."""
    geo, h = mesh(M, kind, L, k)
    a, b = RU.rays(h.dim, 65)
    a, b = a[65 - m:], b[65 - m:]      # the tail: random chords, and for m >= 54 the degenerate ones in front
    z = smooth(h.x)
    for p in (1.0, 1.5, 2.0):
        host = RU.host_line_integrals(lib, h, [z], a, b, p=p)
        for wg in (64, 128, 256):
            res = M.line_integrals(geo, a, b, p=p, z=z, pieces=True, workgroup=wg)
            RU.same_as_host("%s m=%d p=%g wg=%d" % (h.name, m, p, wg), RU.device_result(res), host, h, [z], a, b, p=p)
            assert res.length.shape == (m,)


def test_batch_with_a_nan_node_and_a_ray_outside(M, lib):
    """3 fields x 70 rays in one call: against the host, and bit for bit its three single calls; a repeated call and
    pieces=False return the same bits."""
    geo, h = mesh(M, "fem3d", 2, 3)
    a, b = RU.rays(3, 70)
    rng = np.random.default_rng(7)
    base = smooth(h.x)
    fields = [base.copy(), base + 0.8 * h.x[:, 1] ** 2, base + 0.1 * rng.standard_normal(h.n)]
    clean = RU.host_line_integrals(lib, h, [base], a, b)
    e = int(clean.row(0, 13)[0][0])      # an element that a random chord crosses
    fields[0][e * h.block + 21] = np.nan
    res = batch(M, geo, fields, a, b, pieces=True)
    assert res.length.shape == res.integral.shape == res.count.shape == res.mean.shape == (3, 70)
    dev = RU.device_result(res)
    host = RU.host_line_integrals(lib, h, fields, a, b)
    RU.same_as_host("batch 3 x 70", dev, host, h, fields, a, b)
    RU.against_reference("batch 3 x 70 device", dev, h, fields, a, b)
    crossed = np.array([e in dev.row(0, i)[0] for i in range(70)])
    assert crossed[13] and np.isnan(res.rows[0, crossed, 1:6]).all() and np.isfinite(res.rows[0, crossed][:, [0, 6, 7]]).all()
    assert np.isfinite(res.rows[1:, crossed]).all() and (res.count[:, 10] == 0).all() and (res.rows[:, 10, 4] == -np.inf).all()
    assert np.array_equal(res.count[0], res.count[1])
    again = batch(M, geo, fields, a, b, pieces=True)
    assert again.rows.tobytes() == res.rows.tobytes() and again._piece.tobytes() == res._piece.tobytes()
    assert np.array_equal(again._elem, res._elem) and np.array_equal(again._offsets, res._offsets)
    cheap = batch(M, geo, fields, a, b)
    assert cheap.rows.tobytes() == res.rows.tobytes() and np.array_equal(cheap.count, res.count)
    with pytest.raises(ValueError, match="pieces=False"):
        cheap.pieces(0, 0)
    for bi in range(3):
        one = M.line_integrals(geo, a, b, z=fields[bi], pieces=True)
        assert one.rows[0].tobytes() == res.rows[bi].tobytes() and np.array_equal(one.count, res.count[bi])
        for i in (0, 7, 13, 69):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(one.pieces(i), res.pieces(i, bi)))      # NaN integrals too
    single = M.line_integrals(geo, a[13], b[13], z=fields[1])
    assert single.rows[0, 0].tobytes() == res.rows[1, 13].tobytes() and single.length.shape == (1,)


def test_solutions(M):
    """A 2-D p = 1.5 solve (a gate against the plane section), a fem3d solve projected, and a five-snapshot parabolic run."""
    sol2 = M.fem2d_mpi_solve(L=3, p=1.5)
    line = np.array([1.0, 0.5, 0.05])
    n = line[:2]
    x0, tau = n * line[2] / (n @ n), np.array([n[1], -n[0]]) / np.sqrt(n @ n)
    a, b = (x0 - 4 * tau)[None], (x0 + 4 * tau)[None]
    sec = M.sections(sol2, line, p=1.5, pieces=False)
    gate = M.line_integrals(sol2, a, b, p=1.5)
    # the bars of both yardsticks on the solution's own nodal values, and the overlap
    h = RU.host_mesh("fem2d", 3)
    zc = np.asarray(M._to_cpu_array(sol2.z)).reshape(h.n, -1)[:, 0]
    R, S = RU.reference(h, zc, a, b, 1.5)[0], SU.reference(None, h, zc, line, 1.5)[0]
    assert not R.undecided
    for c_sec, c_ray, got, want in ((0, 0, gate.length[0], sec.measure), (1, 1, gate.integral[0], sec.integral), (2, 3, gate.across[0], sec.flux)):
        bar = float(SU.KTOL * S.abs_terms[c_sec] + R.bars[c_ray] + R.overlap * R.peak[c_ray])
        print("gate column %d: chord %.15g, section %.15g, gap %.3e, bar %.3e" % (c_ray, got, want, abs(got - want), bar))
        assert abs(got - want) <= bar
    sol3 = M.fem3d_mpi_solve(L=2, k=3)
    X, img = M.project(sol3, shape=(8, 8))
    assert X.shape == (8, 8, 2) and img.across is None
    for v in (img.length, img.integral, img.mean, img.along, img.max, img.min, img.enter, img.leave, img.count):
        assert v.shape == (8, 8)
    print("fem3d L=2 projection along z: mean in [%.6g, %.6g], max %.6g" % (img.mean.min(), img.mean.max(), img.max.max()))
    # every ray crosses [-1, 1]: length 2 within the yardstick's bar and its overlap, on the solution's own nodal values
    h3 = RU.host_mesh("fem3d", 2, 3)
    z3 = np.asarray(M._to_cpu_array(sol3.z)).reshape(h3.n, -1)[:, 0]
    pa = np.concatenate([X.reshape(-1, 2), np.full((64, 1), -1.0)], axis=1)
    pb = np.concatenate([X.reshape(-1, 2), np.full((64, 1), 1.0)], axis=1)
    for i, R in enumerate(RU.reference(h3, z3, pa, pb)):
        assert not R.undecided and abs(img.length.reshape(-1)[i] - 2.0) <= R.bars[0] + R.overlap, i
        assert abs(img.length.reshape(-1)[i] - R.rows[0]) <= R.bars[0] and abs(img.integral.reshape(-1)[i] - R.rows[1]) <= R.bars[1], i
    assert (img.min <= img.mean).all() and (img.mean <= img.max).all() and (img.count >= 2).all()
    Xx, side = M.project(sol3, axis=0, shape=(3, 5), pieces=True)
    assert Xx.shape == (3, 5, 2) and side.length.shape == (3, 5) and len(side.pieces(7)[0]) == side.count[1, 2]
    par = M.parabolic_solve(M.fem2d_mpi(3), h=0.25, p=2.0)
    assert len(par.u) == len(par.ts) == 5
    a, b = np.array([[-1.5, 0.1], [0.2, -0.3]]), np.array([[1.5, 0.3], [0.2, 0.9]])
    hist = M.line_integrals(par, a, b, pieces=True)
    for v in (hist.length, hist.integral, hist.mean, hist.along, hist.across, hist.max, hist.min, hist.enter, hist.leave, hist.count):
        assert v.shape == (5, 2)
    assert np.array_equal(hist.ts, par.ts) and hist.rows.shape == (5, 2, 8)
    one = M.line_integrals(par.geometry, a, b, z=par.u[3], pieces=True)
    assert one.rows[0].tobytes() == hist.rows[3].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(one.pieces(1), hist.pieces(1, 3)))
    _, prof = M.project(par, axis=1, shape=(6,))
    assert prof.mean.shape == (5, 6) and np.array_equal(prof.ts, par.ts)


def test_argument_errors(M):
    geo, h = mesh(M, "fem3d", 2, 3)
    z = smooth(h.x)
    a, b = RU.rays(3, 5)
    for kw, err in ((dict(a=a[:, :2]), ValueError), (dict(b=b[:4]), ValueError), (dict(a=np.zeros((2, 5, 3))), ValueError),
                    (dict(p=0.5), ValueError), (dict(p=np.nan), ValueError), (dict(p=np.inf), ValueError),
                    (dict(p=lambda x: 2.0), TypeError), (dict(p=np.full(h.n, 2.0)), TypeError), (dict(p="two"), TypeError),
                    (dict(u=1), ValueError), (dict(z=z[:-1]), ValueError), (dict(workgroup=32), ValueError), (dict(a="ab"), TypeError)):
        with pytest.raises(err):
            M.line_integrals(geo, **{**dict(a=a, b=b, z=z), **kw})
    with pytest.raises(TypeError):
        M.line_integrals(z, a, b)
    empty = M.line_integrals(geo, np.zeros((0, 3)), np.zeros((0, 3)), z=z, pieces=True)
    assert empty.length.shape == (0,) and empty.rows.shape == (1, 0, 8)
    for kw in (dict(axis=3), dict(shape=(4,)), dict(shape=(0, 4)), dict(axis=True)):
        with pytest.raises(ValueError):
            M.project(geo, z=z, **kw)
    with pytest.raises(TypeError):
        M.project(z)
    g1 = M.fem1d_mpi(3)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        M.line_integrals(g1, np.zeros((1, 1)), np.ones((1, 1)), z=np.zeros(len(g1.w)))
    with pytest.raises(ValueError, match="2-D or 3-D"):
        M.project(g1, z=np.zeros(len(g1.w)))
    # the C entry point: MGB_E_ARG before anything is launched
    from mgb_amd import _lib
    loc, backend = M._locator_of(geo)
    zv = M.HPCVector(z, backend)
    other = M.HPCVector(z[:-1], backend)
    rows, count = np.full((5, 8), 7.0), np.full(5, -7, dtype=np.int32)
    lib = _lib.load()
    null_field = object()

    def rc(loc=loc, B=1, vec=zv, S=1, u=0, m=5, pa=_lib.dptr(a), pb=_lib.dptr(b), p=2.0, wg=0, out=_lib.dptr(rows), cnt=_lib.iptr(count)):
        table = None if vec is None else (C.c_void_p * 1)(None if vec is null_field else vec.handle.value)
        return lib.mgb_geo_line_integrals(loc, B, table, S, u, m, pa, pb, p, wg, out, cnt, None)

    assert rc() == 0 and (count >= 0).all()
    rows[:], count[:] = 7.0, -7
    foreign = M.HPCVector(z, M.HPCBackend(0))      # the right length, on a second context of the same device
    for kw in (dict(loc=None), dict(vec=None), dict(vec=null_field), dict(pa=None), dict(pb=None), dict(out=None), dict(cnt=None),
               dict(B=0), dict(B=65536), dict(S=0), dict(u=1), dict(u=-1), dict(m=-1), dict(p=0.5), dict(p=np.nan), dict(p=np.inf),
               dict(wg=32), dict(wg=512), dict(wg=-64), dict(vec=other), dict(vec=foreign)):
        assert rc(**kw) == RU.MGB_E_ARG, kw
    assert (rows == 7.0).all() and (count == -7).all()      # nothing was written
    assert rc(vec=foreign) == RU.MGB_E_ARG and b"another context" in lib.mgb_last_error()
    assert rc(vec=other) == RU.MGB_E_ARG and b"n x S values" in lib.mgb_last_error()
    assert rc(wg=32) == RU.MGB_E_ARG and b"workgroup size" in lib.mgb_last_error()
    assert rc(m=0, pa=None, pb=None, out=None, cnt=None) == 0
    loc1, backend1 = M._locator_of(g1)
    z1 = M.HPCVector(np.zeros(len(g1.w)), backend1)
    assert rc(loc=loc1, vec=z1) == RU.MGB_E_ARG and b"2-D or 3-D geometry" in lib.mgb_last_error()


def test_sharded_contexts_are_refused(M, lib):
    from mgb_amd import _lib
    be = M.HPCBackend(0)
    g = M.fem3d_mpi(1, 1, backend=be)
    z = M.HPCMatrix(np.ones((8, 2)), be)
    a, b = np.array([[-2.0, 0.1, 0.2]]), np.array([[2.0, 0.1, 0.2]])
    R = RU.reference(RU.host_mesh("fem3d", 1, 1), np.ones(8), a, b)[0]
    assert abs(M.line_integrals(g, a, b, z=z).integral[0] - 2.0) <= R.bars[1] + R.overlap      # fine while the context is one rank
    loc, _ = M._locator_of(g)
    be.set_comm(0, 2, lambda ptr, count: None)                                   # rank 0 of 2: no collective is ever started here
    try:
        with pytest.raises(NotImplementedError, match="sharded"):
            M.line_integrals(g, a, b, z=z)
        rows, count = np.zeros(8), np.zeros(1, dtype=np.int32)
        assert lib.mgb_geo_line_integrals(loc, 1, (C.c_void_p * 1)(z._v.handle.value), 2, 0, 1, _lib.dptr(a), _lib.dptr(b), 2.0, 0,
                                          _lib.dptr(rows), _lib.iptr(count), None) == RU.MGB_E_ARG
        assert b"sharded" in lib.mgb_last_error()
    finally:
        be.set_comm(0, 1, None)
