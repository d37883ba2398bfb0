"""CPU tests of the host restatement mgb_geo_line_integrals_host (csrc/ray.hpp: integrate(), the routine the gfx950 kernels
also run) against the np.longdouble yardstick tests/ray_reference.py, plus the cross-check with the plane sections, non-finite
inputs, the batch, project() and the argument errors.

Bars (tests/ray_reference.py): counts and the sets of piece elements equal; every piece end within d_t, every piece integral and
all eight columns within their derived bars; a ratio above 0.5 fails.  Measured over all meshes and p = 1, 1.5, 2: no ray
undecided (0 of 72 per case, the 12 named degenerate rays included); largest ratios to the bars: length 0.095, integral 0.007,
along 0.003, across 0.004, max 0.008, min 0.011, enter 0.029, leave 0.041, piece ends 0.096, piece integrals 0.044 (with 300
rays per mesh: 0 undecided, length 0.149, leave 0.095, piece ends 0.121, piece integrals 0.057).  Sections cross-check: largest
ratio to the sum of both bars plus overlap x max|integrand| 0.834 (the overlap is systematic, see test_ray_reference.py)."""
import numpy as np
import pytest

import levelset_util as LU
import ray_reference as RR
import ray_util as RU
import section_util as SU

smooth = RU.smooth


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0])
@pytest.mark.parametrize("kind,L,k", RU.MESHES)
def test_host_against_numpy(lib, kind, L, k, p):
    g = RU.host_mesh(kind, L, k)
    a, b = RU.rays(g.dim, 72)
    z = np.stack([np.zeros(g.n), smooth(g.x)], axis=1)      # column 1 of 2: a wrong stride shows
    got = RU.host_line_integrals(lib, g, [z], a, b, p=p, u=1)
    RU.against_reference("%s p=%g" % (g.name, p), got, g, [z], a, b, p=p, u=1)
    assert got.rows.shape == (1, 72, 8) and len(got.piece) == got.offsets[-1]
    assert (got.count[0, 10:12] == 0).all() and (got.count[0, np.arange(72) % 8 == 1][2:] == 0).all()      # the rays outside
    if g.dim == 3:
        assert (got.rows[0, :, 3] == 0.0).all()


@pytest.mark.parametrize("kind,L,k", [("fem2d", 4, 0), ("lshape", 2, 0), ("fem3d", 3, 2)])
def test_degenerate_rays_are_integrated_once(lib, kind, L, k):
    """In a face, along an edge, through vertices, within tau of a face: what the pieces of a ray cover twice stays inside the
    yardstick's overlap, and what they cover is the chord."""
    g = RU.host_mesh(kind, L, k)
    a, b = RU.degenerate(g.dim)
    got = RU.host_line_integrals(lib, g, [np.ones(g.n)], a, b)
    ref = RU.reference(g, np.ones(g.n), a, b)
    for i, R in enumerate(ref):
        assert not R.undecided and got.count[0, i] == R.count, i
        elem, piece = got.row(0, i)
        assert len(np.unique(elem)) == len(elem)
        order = np.argsort(piece[:, 0], kind="stable")
        t0, t1 = piece[order, 0].astype(RR.LD), piece[order, 1].astype(RR.LD)
        ell = np.sqrt(((b[i] - a[i]) ** 2).sum())
        union, right = RR.LD(0), -np.inf      # what the pieces cover twice: the sum of their lengths less their union
        for lo, hi in zip(t0, t1):
            union += hi - max(lo, right) if hi > right else RR.LD(0)
            right = max(right, hi)
        twice = (t1 - t0).sum() - union
        assert twice * ell <= R.overlap + R.bars[0], (i, float(twice * ell), float(R.overlap))
        # u = 1: the integral is the length
        if R.count:
            assert abs(got.rows[0, i, 1] - got.rows[0, i, 0]) <= R.bars[0] + R.bars[1], i
    if kind == "fem3d":
        LD = RR.LD
        assert got.count[0, 7] == 4 and abs(got.rows[0, 7, 0] - 2 * np.sqrt(LD(3))) <= ref[7].bars[0] + ref[7].overlap      # the cube diagonal
        assert abs(got.rows[0, 0, 0] - np.hypot(LD(2), LD(1) / 12)) <= ref[0].bars[0] + ref[0].overlap                    # in the face z = 0


@pytest.mark.parametrize("p", [2.0, 1.5])
def test_chords_agree_with_plane_sections(lib, p):
    """2-D: the line n . x = c cut by mgb_geo_sections_host has measure, integral and flux equal to length, integral and across of
    the chord that spans the domain along it with n on its left, within the two sum bars and the overlap."""
    g = RU.host_mesh("fem2d", 4)
    z = smooth(g.x)
    planes = np.array(SU.PLANES2[:4] + [[1.0, 0.0, 2.0 ** -10], [1.0, 0.0, -2.0 ** -10]])      # the last two: just beside the edges in x = 0
    sec = SU.host_sections(lib, g, [z], planes, p=p, pieces=False)
    sref = SU.reference("ray cross-check", g, z, planes, p)
    n = planes[:, :2]
    nn = (n * n).sum(axis=1)
    x0 = n * (planes[:, 2] / nn)[:, None]
    tau = np.stack([n[:, 1], -n[:, 0]], axis=1) / np.sqrt(nn)[:, None]
    a, b = x0 - 4.0 * tau, x0 + 4.0 * tau
    got = RU.host_line_integrals(lib, g, [z], a, b, p=p, pieces=False)
    ref = RU.reference(g, z, a, b, p)
    worst = 0.0
    for l in range(len(planes)):
        R, S = ref[l], sref[l]
        # the line x = 0 lies in element edges, where the normal derivative of a broken field jumps: the cut takes it from the
        # side n points to, the chord from the lowest element, so only measure and integral are the same quantity there; the
        # lines 2^-10 on either side of it carry the flux comparison next to those edges
        for c_sec, c_ray in ((0, 0), (1, 1), (2, 3))[:2 if l == 2 else 3]:
            bar = float(SU.KTOL * S.abs_terms[c_sec] + R.bars[c_ray] + R.overlap * R.peak[c_ray])
            gap = abs(sec.rows[0, l, c_sec] - got.rows[0, l, c_ray])
            worst = max(worst, gap / bar)
            assert gap <= bar, (l, c_sec, gap, bar)
    print("sections cross-check p=%g: largest ratio to the sum of both bars %.3f" % (p, worst))


def test_non_finite_and_empty_segments(lib):
    g = RU.host_mesh("fem3d", 2, 3)
    z = smooth(g.x)
    nan, inf = np.nan, np.inf
    a = np.array([[nan, 0, 0], [0, inf, 0], [-0.5, 0.1, 0.2], [0.3, 0.3, 0.3], [-0.5, 0.1, 0.2], [0.1, -inf, 0.0], [-3.0, 0.1, 0.1]])
    b = np.array([[0.5, 0.1, 0], [0.5, 0.1, 0], [nan, 0.1, 0.2], [0.3, 0.3, 0.3], [0.5, 0.1, -inf], [0.1, inf, 0.0], [3.0, 0.1, 0.1]])
    got = RU.host_line_integrals(lib, g, [z], a, b)
    for i in range(6):
        assert got.count[0, i] == 0 and np.array_equal(got.rows[0, i, :6], [0, 0, 0, 0, -np.inf, np.inf]) and np.isnan(got.rows[0, i, 6:]).all(), i
    R = RU.reference(g, z, a[6:], b[6:])[0]      # the spanning chord: length 2 of 6, t from 1/3 to 2/3
    assert got.count[0, 6] == 2 and abs(got.rows[0, 6, 0] - 2) <= R.bars[0] + R.overlap and len(got.piece) == 2
    assert abs(got.rows[0, 6, 6] - RR.LD(1) / 3) <= R.bars[6] + R.overlap / 6 and abs(got.rows[0, 6, 7] - RR.LD(2) / 3) <= R.bars[7] + R.overlap / 6


@pytest.mark.parametrize("kind,L,k", [("fem2d", 3, 0), ("fem3d", 2, 3), ("fem3d", 2, 1)])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_nodes(lib, kind, L, k, bad):
    g = RU.host_mesh(kind, L, k)
    a, b = RU.rays(g.dim, 40)
    z = smooth(g.x)
    clean = RU.host_line_integrals(lib, g, [z, z + 0.1], a, b)
    crossed = np.unique(clean.elem)
    uncrossed = np.setdiff1d(np.arange(g.nel), crossed)
    assert len(crossed)
    if len(uncrossed):      # a node of an element that no ray owns a piece of: never read
        zu = z.copy()
        zu[uncrossed[0] * g.block:(uncrossed[0] + 1) * g.block] = bad
        got = RU.host_line_integrals(lib, g, [zu, z + 0.1], a, b)
        assert got.rows.tobytes() == clean.rows.tobytes() and got.piece.tobytes() == clean.piece.tobytes()
    first = 12 + int(np.flatnonzero(clean.count[0, 12:] > 0)[0])
    e = int(clean.row(0, first)[0][0])      # an element the first random ray with pieces crosses
    zb = z.copy()
    zb[e * g.block + g.block - 1] = bad
    got = RU.host_line_integrals(lib, g, [zb, z + 0.1], a, b)
    RU.against_reference("non-finite node %s" % g.name, got, g, [zb, z + 0.1], a, b)
    assert np.array_equal(got.count, clean.count) and np.array_equal(got.elem, clean.elem)
    assert got.rows[:, :, [0, 6, 7]].tobytes() == clean.rows[:, :, [0, 6, 7]].tobytes()
    assert got.rows[1].tobytes() == clean.rows[1].tobytes()
    hit = np.array([e in clean.row(0, i)[0] for i in range(40)])
    assert hit.any() and np.isnan(got.rows[0, hit, 1:6]).all()
    assert got.rows[0, ~hit].tobytes() == clean.rows[0, ~hit].tobytes()


def test_elements_of_negative_determinant(lib):
    g = LU.host_mesh("fem2d", 3, mixed=True)
    g.k, g.name = 0, "fem2d mixed L=3"
    a, b = RU.rays(2, 72)
    z = smooth(g.x)
    got = RU.host_line_integrals(lib, g, [z], a, b)
    RU.against_reference(g.name, got, g, [z], a, b)
    ref = RU.reference(g, z, a, b)
    assert abs(got.rows[0, 0, 0] - 2) <= ref[0].bars[0] + ref[0].overlap
    assert abs(got.rows[0, 7, 0] - 2 * np.sqrt(RR.LD(2))) <= ref[7].bars[0] + ref[7].overlap


def test_rows_do_not_depend_on_the_batch(lib):
    g = RU.host_mesh("fem3d", 2, 3)
    a, b = RU.rays(3, 40)
    rng = np.random.default_rng(3)
    fields = [smooth(g.x), rng.standard_normal(g.n), -smooth(g.x)]      # the second one broken across the elements
    got = RU.host_line_integrals(lib, g, fields, a, b, p=1.5)
    for bi in range(3):
        one = RU.host_line_integrals(lib, g, [fields[bi]], a, b, p=1.5)
        assert one.rows[0].tobytes() == got.rows[bi].tobytes() and np.array_equal(one.count[0], got.count[bi])
        s, e = got.offsets[bi * 40], got.offsets[(bi + 1) * 40]
        assert one.piece.tobytes() == got.piece[s:e].tobytes() and np.array_equal(one.elem, got.elem[s:e])
    # a ray alone, and in another place of another batch
    for i in (0, 7, 13, 39):
        one = RU.host_line_integrals(lib, g, [fields[1]], a[i:i + 1], b[i:i + 1], p=1.5)
        assert one.rows[0, 0].tobytes() == got.rows[1, i].tobytes() and one.piece.tobytes() == got.row(1, i)[1].tobytes()


def test_argument_errors(lib):
    from mgb_amd import _lib
    g3, g1 = RU.host_mesh("fem3d", 2, 1), LU.host_mesh("fem1d", 3)
    z3 = np.zeros((g3.n, 2))
    a, b = RU.rays(3, 5)
    ok = dict(a=a, b=b, rc_only=True)
    assert RU.host_line_integrals(lib, g3, [z3], **ok) == 0
    for kw, msg in ((dict(B=0), b"B must be 1..65535"), (dict(B=65536), b"B must be 1..65535"), (dict(S=0), b"S must be >= 1"),
                    (dict(u=2), b"column u outside"), (dict(u=-1), b"column u outside"), (dict(m=-1), b"m must be >= 0"),
                    (dict(p=0.5), b"p must be one finite real >= 1"), (dict(p=np.nan), b"p must be one finite real >= 1"),
                    (dict(p=np.inf), b"p must be one finite real >= 1")):
        assert RU.host_line_integrals(lib, g3, [z3], **{**ok, **kw}) == RU.MGB_E_ARG, kw
        err = lib.mgb_last_error()
        assert b"geo_line_integrals_host" in err and msg in err, (kw, err)
    rows, count = np.full((5, 8), 7.0), np.full(5, -7, dtype=np.int32)
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z3))
    call = lambda h, t, pa, pb, r, c, m=5: lib.mgb_geo_line_integrals_host(h, 1, t, 2, 0, m, pa, pb, 2.0, r, c, None, None, None, 0)
    full = (g3.handle, table, _lib.dptr(a), _lib.dptr(b), _lib.dptr(rows), _lib.iptr(count))
    assert call(*full) == 0
    for j in range(6):
        args = list(full)
        args[j] = None
        assert call(*args) == RU.MGB_E_ARG and b"null argument" in lib.mgb_last_error(), j
    assert call(g3.handle, (_lib.c_dbl_p * 1)(None), *full[2:]) == RU.MGB_E_ARG and b"null field" in lib.mgb_last_error()
    # m = 0 returns at once, whatever the arrays
    rows[:], count[:] = 7.0, -7
    assert call(g3.handle, table, None, None, None, None, m=0) == 0 and (rows == 7.0).all() and (count == -7).all()
    # offsets, pieces and elements come together; arrays that are too small
    piece, elem, offsets = np.empty((1, 3)), np.empty(1, dtype=np.int32), np.empty(6, dtype=np.int64)
    host = lambda op, pp, ep, cap: lib.mgb_geo_line_integrals_host(g3.handle, 1, table, 2, 0, 5, _lib.dptr(a), _lib.dptr(b), 2.0,
                                                                   _lib.dptr(rows), _lib.iptr(count), op, pp, ep, cap)
    ll = offsets.ctypes.data_as(_lib.c_ll_p)
    assert host(ll, _lib.dptr(piece), None, 1) == RU.MGB_E_ARG and b"come together" in lib.mgb_last_error()
    assert host(None, _lib.dptr(piece), _lib.iptr(elem), 1) == RU.MGB_E_ARG and b"come together" in lib.mgb_last_error()
    assert host(ll, _lib.dptr(piece), _lib.iptr(elem), -1) == RU.MGB_E_ARG and b"negative capacity" in lib.mgb_last_error()
    assert host(ll, _lib.dptr(piece), _lib.iptr(elem), 1) == RU.MGB_E_ARG and b"more pieces than the arrays hold" in lib.mgb_last_error()
    # a 1-D geometry
    z1, a1, b1 = np.zeros(g1.n), np.zeros((1, 1)), np.ones((1, 1))
    assert lib.mgb_geo_line_integrals_host(g1.handle, 1, (_lib.c_dbl_p * 1)(_lib.dptr(z1)), 1, 0, 1, _lib.dptr(a1), _lib.dptr(b1), 2.0,
                                           _lib.dptr(rows), _lib.iptr(count), None, None, None, 0) == RU.MGB_E_ARG
    assert b"2-D or 3-D geometry" in lib.mgb_last_error()


class _HostBacked:
    """line_integrals() with the device call replaced by the host restatement: what project() does on top of it -- the rays,
    the pixel centres, the reshaping -- is plain Python and runs without a GPU."""

    def __init__(self, lib, g, z):
        self.lib, self.g, self.z, self.calls = lib, g, z, 0

    def __call__(self, obj, a, b, p=2.0, **kw):
        import mgb_amd as M
        self.calls += 1
        got = RU.host_line_integrals(self.lib, self.g, [self.z], a, b, p=p, pieces=False)
        return M.LineIntegrals(got.rows, got.count, None, self.g.dim)


@pytest.mark.parametrize("kind,L,k,axis,shape", [("fem3d", 2, 2, -1, (5, 4)), ("fem3d", 2, 2, 0, (3, 6)), ("fem2d", 3, 0, 1, (7,))])
def test_project_against_single_rays(lib, monkeypatch, kind, L, k, axis, shape):
    import mgb_amd as M
    g = RU.host_mesh(kind, L, k)
    z = smooth(g.x)
    geo = M.Geometry({"dim": g.dim}, g.x, np.ones(g.n), {}, {}, [], [])
    fake = _HostBacked(lib, g, z)
    monkeypatch.setattr(M, "line_integrals", fake)
    X, res = M.project(geo, axis=axis, shape=shape, p=1.5)
    assert fake.calls == 1 and X.shape == shape + (g.dim - 1,)
    for name in ("length", "integral", "mean", "along", "max", "min", "enter", "leave", "count"):
        assert getattr(res, name).shape == shape, name
    assert (res.across is None) == (g.dim == 3)
    ax = axis % g.dim
    others = [d for d in range(g.dim) if d != ax]
    for idx in np.ndindex(*shape):
        # pixel centres: the fastest image axis is the first remaining coordinate
        centre = [-1.0 + (idx[len(shape) - 1 - j] + 0.5) * 2.0 / shape[len(shape) - 1 - j] for j in range(len(others))]
        assert np.allclose(X[idx], centre, rtol=0, atol=1e-15)
        a, b = np.empty(g.dim), np.empty(g.dim)
        a[others], b[others] = X[idx], X[idx]
        a[ax], b[ax] = -1.0, 1.0
        one = RU.host_line_integrals(lib, g, [z], a[None], b[None], p=1.5, pieces=False)
        assert res.length[idx] == one.rows[0, 0, 0] and res.integral[idx] == one.rows[0, 0, 1] and res.max[idx] == one.rows[0, 0, 4]
        R = RU.reference(g, z, a[None], b[None], 1.5)[0]
        assert res.count[idx] == one.count[0, 0] and abs(res.length[idx] - 2) <= R.bars[0] + R.overlap
        assert res.mean[idx] == one.rows[0, 0, 1] / one.rows[0, 0, 0] and res.min[idx] <= res.mean[idx] <= res.max[idx]


def test_object_file_shares_no_arithmetic_with_other_objects():
    """ray.hip is compiled with contraction off, most other files with it on.  An out-of-line copy of a function of interp.hpp,
    flowline.hpp or section.hpp in ray.o would be a weak symbol that the linker merges with theirs, so that the link order would
    decide whose bits both sides compute (DESIGN.md sections 4q, 4t).  Where the object file of the build is at hand it must
    define no weak function of the shared namespaces."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "multigridbarriermpi.jl_amd", "csrc", "_obj", "ray.o")
    if not os.path.exists(obj) or shutil.which("nm") is None:
        return      # a tree that was not built here (the objects do not travel): the GPU tests hold device and host to the same bits
    out = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    weak = [l for l in out.splitlines() if len(l.split()) > 2 and l.split()[1] in "WwVv"]
    shared = [l for l in weak if any("mgb::%s::" % ns in l for ns in ("interp", "flowline", "section", "ray", "levelset", "isosurface"))]
    assert not shared, shared


def test_python_names():
    import mgb_amd as M
    assert {"line_integrals", "project", "LineIntegrals"} <= set(M.__all__)
    assert M.LineIntegrals.__doc__ and M.line_integrals.__doc__ and M.project.__doc__
