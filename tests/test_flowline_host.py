"""CPU tests of the host restatement mgb_geo_flow_lines_host (csrc/flowline.hpp: the per-seed routine the gfx950 kernel also
runs) against the longdouble yardstick tests/flowline_reference.py: whole lines (status, count, elements), the closed forms,
the one-step replay under its bars, the degenerate seeds and fields, and the argument errors.

Bars (tests/flowline_reference.py): a replayed step 2 ds (E_1 + E_m) + 16 eps (max|x| + ds); an exit point
|q - x_k| 2^-40 + 2 bar; closed-form exits, lengths and times ds 2^-40 + 2e-12 (times the secant where a ray meets the boundary
at an angle).  Largest ratios measured on the host: points 0.014, length and time 0.007; no undecided step in any case."""
import ctypes as C

import numpy as np
import pytest

import flowline_reference as FR
import flowline_util as FU
import mesh_cases as MC

LD = FR.LD


def smooth2(x):
    return np.sin(3.0 * x[:, 0] + 0.5) * np.cos(2.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 1] + 0.9 * x[:, 0]


def smooth3(x):
    return np.sin(1.3 * x[:, 0] + 0.5) * np.cos(1.1 * x[:, 1]) + 0.4 * x[:, 2] * x[:, 0] + 0.8 * x[:, 2]


def tol(ds, end=None):
    sec = 1.0 if end is None else float(np.sqrt((end ** 2).sum()) / np.abs(end).max())
    return ds * 2.0 ** -40 + 2e-12 * sec


@pytest.mark.parametrize("L", [2, 3])
def test_u_equals_x(lib, L):
    """horizontal lines: EXIT at (1, y0), length = time = 1 - x0 for every p; the field is column 1 of 2"""
    g = FU.host_mesh("fem2d", L)
    z = np.stack([np.zeros(g.n), g.x[:, 0]], axis=1)
    seeds = FU.seeds_2d(9)
    for p in (1.0, 1.5, 2.0, 3.0):
        got = FU.host_flow_lines(lib, g, [z], seeds, p=p, u=1)
        assert got.ds == 2.0 ** -L and (got.status == FR.EXIT).all()
        t = tol(got.ds)
        assert np.abs(got.end[0, :, 0] - 1).max() <= t and np.abs(got.end[0, :, 1] - seeds[:, 1]).max() <= t
        assert np.abs(got.rows[0, :, 0] - (1 - seeds[:, 0])).max() <= t and np.abs(got.rows[0, :, 1] - (1 - seeds[:, 0])).max() <= t
        assert np.abs(got.rows[0, :, 2] - seeds[:, 0]).max() <= 1e-15 and np.abs(got.rows[0, :, 3] - 1).max() <= t
    FU.against_lines("u = x L=%d" % L, got, g, [z], seeds, 3.0, 1, 256, 1e-12, u=1)
    FU.replay("u = x L=%d" % L, got, g, [z], 3.0, 1, 256, 1e-12, u=1)


@pytest.mark.parametrize("L", [2, 3])
def test_paraboloid_rays(lib, L):
    g = FU.host_mesh("fem2d", L)
    z = (g.x ** 2).sum(axis=1)
    seeds = FU.seeds_2d(9)
    r0 = np.sqrt((seeds ** 2).sum(axis=1))
    end = seeds / np.abs(seeds).max(axis=1)[:, None]
    rend = np.sqrt((end ** 2).sum(axis=1))
    for p in (1.0, 2.0):
        got = FU.host_flow_lines(lib, g, [z], seeds, p=p)
        assert (got.status == FR.EXIT).all()
        for i in range(len(seeds)):
            t = tol(got.ds, end[i])
            assert np.abs(got.end[0, i] - end[i]).max() <= t and abs(got.rows[0, i, 0] - (rend[i] - r0[i])) <= t
            if p == 1.0:
                assert abs(got.rows[0, i, 1] - got.rows[0, i, 0]) <= t
            else:
                assert abs(got.rows[0, i, 1] - np.log(rend[i] / r0[i]) / 2) <= got.ds ** 2 / r0[i] ** 2
    FU.against_lines("paraboloid L=%d" % L, got, g, [z], seeds, 2.0, 1, 256, 1e-12)
    FU.replay("paraboloid L=%d" % L, got, g, [z], 2.0, 1, 256, 1e-12)
    ds = got.ds
    back = FU.host_flow_lines(lib, g, [z], seeds, p=2.0, direction=-1, gmin=2 * ds)
    # 2 r <= gmin = 2 ds where the stall is seen: at x_k or, by step 5 of the rule, at the midpoint ds / 2 ahead of it
    assert (back.status == FR.STALLED).all() and (np.sqrt((back.end[0] ** 2).sum(axis=1)) <= 1.5 * ds + 1e-15).all()
    assert (back.rows[0, :, 3] <= back.rows[0, :, 2]).all()
    FU.against_lines("paraboloid down L=%d" % L, back, g, [z], seeds, 2.0, -1, 256, 2 * ds)
    FU.replay("paraboloid down L=%d" % L, back, g, [z], 2.0, -1, 256, 2 * ds)


def test_hyperbolas(lib):
    """u = x y: x^2 - y^2 is constant along a line up to the second-order error of the rule, which the yardstick's own lines
    (test_flowline_reference.py measures their order) show: the library's drift is the yardstick's to 1e-12"""
    g = FU.host_mesh("fem2d", 3)
    z = g.x[:, 0] * g.x[:, 1]
    seeds = np.array([[0.31 + 0.0417 * i, 0.23 - 0.0331 * i] for i in range(4)])
    M = FU.mesh_of(g)
    for ds, n in ((0.125, 4), (0.0625, 8)):
        got = FU.host_flow_lines(lib, g, [z], seeds, p=2.0, ds=ds, max_steps=n)
        assert (got.status == FR.MAXSTEPS).all() and (got.count == n + 1).all() and np.abs(got.rows[0, :, 0] - 0.5).max() <= 1e-15
        for i, s in enumerate(seeds):
            R = FR.trace(M, z, s, 2.0, 1, ds, n, 1e-12)
            drift = got.end[0, i, 0] ** 2 - got.end[0, i, 1] ** 2 - (s[0] ** 2 - s[1] ** 2)
            ref = float(R.end[0] ** 2 - R.end[1] ** 2 - (LD(s[0]) ** 2 - LD(s[1]) ** 2))
            assert abs(drift - ref) <= 1e-12 and abs(drift) <= ds * ds
        FU.against_lines("hyperbolas", got, g, [z], seeds, 2.0, 1, n, 1e-12)
        FU.replay("hyperbolas ds=%g" % ds, got, g, [z], 2.0, 1, n, 1e-12)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_fem3d_closed_forms(lib, k):
    g = FU.host_mesh("fem3d", 1, k)
    seeds = FU.seeds_3d(6)
    z = g.x[:, 0].copy()
    got = FU.host_flow_lines(lib, g, [z], seeds, p=1.5)
    t = tol(got.ds)
    assert got.ds == 0.5 and (got.status == FR.EXIT).all()
    assert np.abs(got.end[0, :, 0] - 1).max() <= t and np.abs(got.end[0, :, 1:] - seeds[:, 1:]).max() <= t
    assert np.abs(got.rows[0, :, 0] - (1 - seeds[:, 0])).max() <= t and np.abs(got.rows[0, :, 1] - got.rows[0, :, 0]).max() <= t
    FU.against_lines("fem3d k=%d u = x" % k, got, g, [z], seeds, 1.5, 1, 256, 1e-12)
    FU.replay("fem3d k=%d u = x" % k, got, g, [z], 1.5, 1, 256, 1e-12)
    z = (g.x ** 2).sum(axis=1)
    got = FU.host_flow_lines(lib, g, [z], seeds, p=1.0, ds=0.125)
    if k == 1:      # the trilinear interpolant of |x|^2 is the constant 3
        assert (got.status == FR.STALLED).all() and (got.count == 1).all() and (got.rows[0, :, 0] == 0).all()
        return
    end = seeds / np.abs(seeds).max(axis=1)[:, None]
    for i in range(len(seeds)):
        t = tol(0.125, end[i])
        assert got.status[0, i] == FR.EXIT and np.abs(got.end[0, i] - end[i]).max() <= t
        want = np.sqrt((end[i] ** 2).sum()) - np.sqrt((seeds[i] ** 2).sum())
        assert abs(got.rows[0, i, 0] - want) <= t and abs(got.rows[0, i, 1] - got.rows[0, i, 0]) <= t
    FU.against_lines("fem3d k=%d |x|^2" % k, got, g, [z], seeds, 1.0, 1, 256, 1e-12)
    FU.replay("fem3d k=%d |x|^2" % k, got, g, [z], 1.0, 1, 256, 1e-12)


def test_replay_on_smooth_fields(lib):
    """sin / cos products sampled at the nodes: broken gradients across the elements, p = 1.5 (pow), both directions"""
    g = FU.host_mesh("fem2d", 3)
    z, seeds = smooth2(g.x), FU.seeds_2d(10)
    for direction in (1, -1):
        got = FU.host_flow_lines(lib, g, [z], seeds, p=1.5, direction=direction, max_steps=48)
        FU.against_lines("smooth fem2d L=3 dir %d" % direction, got, g, [z], seeds, 1.5, direction, 48, 1e-12)
        FU.replay("smooth fem2d L=3 dir %d" % direction, got, g, [z], 1.5, direction, 48, 1e-12)
    g = FU.host_mesh("fem3d", 1, 2)
    z, seeds = smooth3(g.x), FU.seeds_3d(6)
    got = FU.host_flow_lines(lib, g, [z], seeds, p=1.5, ds=0.0625, max_steps=48)
    FU.against_lines("smooth fem3d L=1 k=2", got, g, [z], seeds, 1.5, 1, 48, 1e-12)
    FU.replay("smooth fem3d L=1 k=2", got, g, [z], 1.5, 1, 48, 1e-12)


def test_seeds_outside_and_not_finite(lib):
    g = FU.host_mesh("fem2d", 2)
    z = g.x[:, 0].copy()
    seeds = np.array([[0.3, 0.2], [1.5, 0.0], [np.nan, 0.1], [0.1, np.inf], [-0.4, 0.7]])
    got = FU.host_flow_lines(lib, g, [z], seeds)
    assert np.array_equal(got.status[0], [FR.EXIT, FR.OUTSIDE, FR.OUTSIDE, FR.OUTSIDE, FR.EXIT])
    for i in (1, 2, 3):
        assert np.isnan(got.rows[0, i]).all() and np.isnan(got.end[0, i]).all()
        assert got.count[0, i] == 0 and got.end_element[0, i] == -1 and len(got.path(0, i)[0]) == 0
    alone = FU.host_flow_lines(lib, g, [z], seeds[[0, 4]])
    assert alone.rows.tobytes() == got.rows[:, [0, 4]].tobytes() and alone.path(0, 1)[0].tobytes() == got.path(0, 4)[0].tobytes()
    FU.against_lines("outside", got, g, [z], seeds, 2.0, 1, 256, 1e-12)


def test_nan_node_reached_by_one_line(lib):
    g = FU.host_mesh("fem2d", 3)
    z = g.x[:, 0] + 0.25 * g.x[:, 1]
    seeds = np.array([[-0.83, -0.7131], [-0.7717, 0.1369], [-0.6134, 0.6838], [0.4351, -0.3307]])
    clean = FU.host_flow_lines(lib, g, [z], seeds, max_steps=64)
    # an element that exactly one line reaches, not at its start: the lines are straight (u is linear), so a line reaches an
    # element when a dense sampling of its segment seed -> end does (stage points and bisection points lie on that segment)
    xe = g.x.reshape(-1, 7, 2)
    t = np.linspace(0.0, 1.0, 2049)[:, None]
    reach = []
    for i in range(len(seeds)):
        q = seeds[i] + t * (clean.end[0, i] - seeds[i])
        a, b, d = xe[:, 1] - xe[:, 0], xe[:, 2] - xe[:, 0], q[:, None, :] - xe[None, :, 0]
        det = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        r0, r1 = (d[..., 0] * b[:, 1] - d[..., 1] * b[:, 0]) / det, (a[:, 0] * d[..., 1] - a[:, 1] * d[..., 0]) / det
        reach.append(set(np.flatnonzero(((r0 >= -1e-3) & (r1 >= -1e-3) & (1 - r0 - r1 >= -1e-3)).any(axis=0)).tolist()))
    assert (clean.status == FR.EXIT).all()
    only = [(e, i) for i in range(len(seeds)) for e in sorted(reach[i])
            if sum(e in q for q in reach) == 1 and e != clean.path(0, i)[1][0] and e in clean.path(0, i)[1]]
    e, line = only[0]
    zb = z.copy()
    zb[7 * e: 7 * e + 7] = np.nan
    got = FU.host_flow_lines(lib, g, [zb], seeds, max_steps=64)
    assert got.status[0, line] == FR.NONFINITE and got.end_element[0, line] == e and np.isnan(got.rows[0, line, 3])
    assert np.isfinite(got.rows[0, line, :3]).all() and 1 < got.count[0, line] < clean.count[0, line]
    n = got.count[0, line]
    assert got.path(0, line)[0].tobytes() == clean.path(0, line)[0][:n].tobytes()
    for i in range(len(seeds)):
        if i != line:
            assert got.rows[0, i].tobytes() == clean.rows[0, i].tobytes() and got.end[0, i].tobytes() == clean.end[0, i].tobytes()
            assert got.status[0, i] == clean.status[0, i] and got.path(0, i)[0].tobytes() == clean.path(0, i)[0].tobytes()
    FU.against_lines("NaN node", got, g, [zb], seeds, 2.0, 1, 64, 1e-12)


def test_constant_field_and_one_step(lib):
    g = FU.host_mesh("fem2d", 2)
    seeds = FU.seeds_2d(5)
    got = FU.host_flow_lines(lib, g, [np.full(g.n, 0.3)], seeds)
    assert (got.status == FR.STALLED).all() and (got.count == 1).all() and (got.rows[0, :, :2] == 0).all()
    assert (got.rows[0, :, 2:] == 0.3).all() or np.abs(got.rows[0, :, 2:] - 0.3).max() <= 1e-15
    assert got.end.tobytes() == seeds[None].tobytes() and got.pts.tobytes() == seeds.tobytes()
    z = g.x[:, 0].copy()
    one = FU.host_flow_lines(lib, g, [z], seeds, max_steps=1)
    inner = seeds[:, 0] + one.ds < 1
    assert inner.any() and (one.status[0, inner] == FR.MAXSTEPS).all() and (one.count[0, inner] == 2).all()
    assert (one.rows[0, inner, 0] == one.ds).all()
    FU.against_lines("max_steps = 1", one, g, [z], seeds, 2.0, 1, 1, 1e-12)
    FU.replay("max_steps = 1", one, g, [z], 2.0, 1, 1, 1e-12)


def test_elements_of_negative_determinant(lib):
    g = FU.host_mesh("fem2d", 3, mixed=True)
    xe = g.x.reshape(-1, 7, 2)
    det = (xe[:, 1, 0] - xe[:, 0, 0]) * (xe[:, 2, 1] - xe[:, 0, 1]) - (xe[:, 1, 1] - xe[:, 0, 1]) * (xe[:, 2, 0] - xe[:, 0, 0])
    assert (det < 0).any() and (det > 0).any()
    z, seeds = (g.x ** 2).sum(axis=1), np.vstack([FU.seeds_2d(5), -FU.seeds_2d(5)])      # both triangles
    got = FU.host_flow_lines(lib, g, [z], seeds, p=1.0)
    end = seeds / np.abs(seeds).max(axis=1)[:, None]
    used = np.unique(got.elem)
    assert (det[used] < 0).any() and (det[used] > 0).any() and (got.status == FR.EXIT).all()
    for i in range(len(seeds)):
        assert np.abs(got.end[0, i] - end[i]).max() <= tol(got.ds, end[i])
    FU.against_lines("mixed determinants", got, g, [z], seeds, 1.0, 1, 256, 1e-12)
    FU.replay("mixed determinants", got, g, [z], 1.0, 1, 256, 1e-12)


def test_non_convex_mesh(lib):
    """The L shape [-1, 1]^2 without (0, 1]^2: lines of u = x + y from the lower left run at 45 degrees into the walls of the
    re-entrant corner, x = 0 (y > 0) or y = 0 (x > 0), or leave through x = 1 or y = 1: every end point is on the boundary."""
    g = FU.host_mesh("fem2d", 3, K=("lshape", MC.LSHAPE))
    z = g.x[:, 0] + g.x[:, 1]
    s0 = np.array([[-0.83 + 0.0917 * i, -0.91 + 0.0531 * i] for i in range(8)])
    s0 = np.vstack([s0, s0[:, ::-1], [[-0.93, 0.0417], [0.0531, -0.97]]])      # both walls, and the outer side x = 1
    got = FU.host_flow_lines(lib, g, [z], s0, p=2.0)
    assert (got.status == FR.EXIT).all()
    ex, ey = got.end[0, :, 0], got.end[0, :, 1]
    t = tol(got.ds) * np.sqrt(2.0)      # the walls are met at 45 degrees
    wall_x0 = (np.abs(ex) <= t) & (ey >= -t)
    wall_y0 = (np.abs(ey) <= t) & (ex >= -t)
    outer = (np.abs(ex - 1) <= t) | (np.abs(ey - 1) <= t)
    assert (wall_x0 | wall_y0 | outer).all() and wall_x0.any() and wall_y0.any() and outer.any()
    assert np.abs((ex - ey) - (s0[:, 0] - s0[:, 1])).max() <= t      # each line kept its diagonal
    FU.against_lines("L shape", got, g, [z], s0, 2.0, 1, 256, 1e-12)
    FU.replay("L shape", got, g, [z], 2.0, 1, 256, 1e-12)


def test_argument_errors(lib):
    g = FU.host_mesh("fem2d", 2)
    z, seeds = np.zeros((g.n, 2)), FU.seeds_2d(3)
    ok = dict(rc_only=True)
    assert FU.host_flow_lines(lib, g, [z], seeds, **ok) == 0
    bad = (dict(ds=0.0), dict(ds=-0.1), dict(ds=np.nan), dict(ds=np.inf), dict(max_steps=0), dict(max_steps=-3), dict(gmin=-1e-3),
           dict(gmin=np.nan), dict(gmin=np.inf), dict(direction=0), dict(direction=2), dict(p=0.5), dict(p=np.nan), dict(p=np.inf),
           dict(u=2), dict(u=-1), dict(B=0), dict(B=65536), dict(m=-1), dict(S=0))
    for kw in bad:
        assert FU.host_flow_lines(lib, g, [z], seeds, **{**ok, **kw}) == FU.MGB_E_ARG, kw
        assert b"flow_lines" in lib.mgb_last_error()
    assert FU.host_flow_lines(lib, g, [z], np.empty((0, 2)), **ok) == 0      # m = 0: at once
    from mgb_amd import _lib
    g1 = FU.LU.host_mesh("fem1d", 3)
    rows, end = np.empty((3, 4)), np.empty((3, 2))
    ints = [np.empty(3, dtype=np.int32) for _ in range(3)]
    t1 = (_lib.c_dbl_p * 1)(_lib.dptr(np.zeros(g1.n)))
    call = lambda h, table, sd, r, off=None, pts=None, el=None, cap=0, steps=16: lib.mgb_geo_flow_lines_host(
        h, 1, table, 2, 0, 3, sd, 2.0, 1, None, steps, 1e-12, r, _lib.dptr(end), *map(_lib.iptr, ints), None, off, pts, el, cap)
    table = (_lib.c_dbl_p * 1)(_lib.dptr(z))
    assert call(g.handle, table, _lib.dptr(seeds), _lib.dptr(rows)) == 0
    assert lib.mgb_geo_flow_lines_host(g1.handle, 1, t1, 1, 0, 3, _lib.dptr(seeds), 2.0, 1, None, 16, 1e-12, _lib.dptr(rows),
                                       _lib.dptr(end), *map(_lib.iptr, ints), None, None, None, None, 0) == FU.MGB_E_ARG      # 1-D
    for args in ((None, table, _lib.dptr(seeds), _lib.dptr(rows)), (g.handle, None, _lib.dptr(seeds), _lib.dptr(rows)),
                 (g.handle, table, None, _lib.dptr(rows)), (g.handle, table, _lib.dptr(seeds), None),
                 (g.handle, (_lib.c_dbl_p * 1)(None), _lib.dptr(seeds), _lib.dptr(rows))):
        assert call(*args) == FU.MGB_E_ARG
    # paths: the three arrays come together, hold what is recorded, and stay inside 2^31 - 1 entries of the fixed-stride buffer
    off, pts, el = np.empty(4, dtype=np.int64), np.empty((3, 2)), np.empty(3, dtype=np.int32)
    offp = off.ctypes.data_as(_lib.c_ll_p)
    zx = np.stack([g.x[:, 0], g.x[:, 1]], axis=1).copy()
    tx = (_lib.c_dbl_p * 1)(_lib.dptr(zx))
    assert call(g.handle, tx, _lib.dptr(seeds), _lib.dptr(rows), offp, _lib.dptr(pts), None, 3) == FU.MGB_E_ARG
    assert call(g.handle, tx, _lib.dptr(seeds), _lib.dptr(rows), offp, _lib.dptr(pts), _lib.iptr(el), 3) == FU.MGB_E_ARG      # too small
    assert call(g.handle, tx, _lib.dptr(seeds), _lib.dptr(rows), offp, _lib.dptr(pts), _lib.iptr(el), -1) == FU.MGB_E_ARG
    assert call(g.handle, tx, _lib.dptr(seeds), _lib.dptr(rows), offp, _lib.dptr(pts), _lib.iptr(el), 3, steps=2 ** 29) == FU.MGB_E_ARG
    assert b"2^31" in lib.mgb_last_error()
    assert call(g.handle, tx, _lib.dptr(seeds), _lib.dptr(rows), steps=2 ** 29) == 0      # without paths no such limit applies


def test_python_names_and_header():
    import mgb_amd as M
    assert {"flow_lines", "FlowLines"} <= set(M.__all__)
    F = M.FlowLines
    assert (F.EXIT, F.STALLED, F.MAXSTEPS, F.OUTSIDE, F.NONFINITE) == (0, 1, 2, 3, 4)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgb_hip.h")).read()
    for name, v in (("EXIT", 0), ("STALLED", 1), ("MAXSTEPS", 2), ("OUTSIDE", 3), ("NONFINITE", 4)):
        assert "#define MGB_FLOW_%s %d\n" % (name, v) in hdr


def test_object_file_shares_no_arithmetic_with_other_objects():
    """flowline.hip is compiled with contraction off, most other files with it on.  An out-of-line copy of a function of
    interp.hpp in flowline.o would be a weak symbol that the linker merges with theirs, so that the link order would decide whose
    bits both sides compute.  Where the object file of the build is at hand it must define no weak
    function of the shared namespaces; exception classes are all it may share."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "multigridbarriermpi.jl_amd", "csrc", "_obj", "flowline.o")
    if not os.path.exists(obj) or shutil.which("nm") is None:
        return      # a tree that was not built here (the objects do not travel): the GPU tests hold device and host to the same bits
    out = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    weak = [l for l in out.splitlines() if len(l.split()) > 2 and l.split()[1] in "WwVv"]
    shared = [l for l in weak if "mgb::interp::" in l or "mgb::flowline::" in l]
    assert not shared, shared
