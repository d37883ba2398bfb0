"""CPU tests of the host restatement mgb_geo_path_lines_host (csrc/pathline.hpp: the per-seed routine the gfx950 kernel also
runs) against the longdouble yardstick tests/pathline_reference.py: whole trajectories (status, count, rested, elements), the
one-step replay under its bars, the stationary case against mgb_geo_flow_lines_host bit for bit, independence of the batch,
every release index, degenerate seeds and fields, and the argument errors.

Bars (tests/pathline_reference.py): a replayed step dt (W_1 + W_m) + 16 eps (max|x| + dt |w|); an exit point
|q - x_k| 2^-40 + 2 bar; an exit time span 2^-40 + 2 bar / |w|.  Largest ratios measured on the host: points 0.014, length
0.003, exit time 0.001; no undecided step in any case."""
import numpy as np
import pytest

import flowline_reference as FR
import flowline_util as FU
import mesh_cases as MC
import pathline_reference as PR
import pathline_util as PU

TS3 = np.array([0.0, 0.125, 0.375])
TS4 = np.array([0.0, 0.125, 0.25, 0.5])


@pytest.mark.parametrize("L", [1, 3])
def test_fem2d_against_the_yardstick(lib, L):
    g = FU.host_mesh("fem2d", L)
    seeds = FU.seeds_2d(8)
    for p, speed, n in ((2.0, 0.25, 3), (1.0, 0.5, 2), (1.5, 0.3, 4), (1.75, 0.25, 2)):
        fields = PU.fields_2d(g.x, 4)
        rel = np.arange(8) % 3
        got = PU.host_path_lines(lib, g, fields, TS4, seeds, release=rel, substeps=n, p=p, speed=speed)
        name = "fem2d L=%d p=%g" % (L, p)
        assert set(got.status) <= {PR.DONE, PR.EXIT} and (got.status == PR.DONE).any()
        PU.against_lines(name, got, g, fields, TS4, seeds, rel, 3, n, p, -1, speed, 1e-12)
        PU.replay(name, got, g, fields, TS4, rel, 3, n, p, -1, speed, 1e-12)
    fast = PU.host_path_lines(lib, g, fields, TS4, seeds, substeps=2, p=2.0, speed=1.0)
    assert (fast.status == PR.EXIT).any()
    PU.against_lines("fem2d L=%d fast" % L, fast, g, fields, TS4, seeds, 0, 3, 2, 2.0, -1, 1.0, 1e-12)
    PU.replay("fem2d L=%d fast" % L, fast, g, fields, TS4, 0, 3, 2, 2.0, -1, 1.0, 1e-12)


@pytest.mark.parametrize("L,k", [(1, 1), (2, 3), (2, 2)])
def test_fem3d_against_the_yardstick(lib, L, k):
    g = FU.host_mesh("fem3d", L, k)
    seeds = FU.seeds_3d(4)
    fields = PU.fields_3d(g.x, 3)
    rel = np.array([0, 1, 0, 1])
    for p, speed, direction in ((2.0, 1.0, -1), (1.5, 4.0, 1)):
        got = PU.host_path_lines(lib, g, fields, TS3, seeds, release=rel, substeps=2, p=p, speed=speed, direction=direction)
        name = "fem3d L=%d k=%d p=%g" % (L, k, p)
        PU.against_lines(name, got, g, fields, TS3, seeds, rel, 2, 2, p, direction, speed, 1e-12)
        PU.replay(name, got, g, fields, TS3, rel, 2, 2, p, direction, speed, 1e-12)


def stationary_pair(lib, g, z, seeds, B):
    ts = 2.0 ** -3 * np.arange(B)
    path = PU.host_path_lines(lib, g, [z] * B, ts, seeds, substeps=4, p=1.0, speed=1.0, direction=-1)
    flow = FU.host_flow_lines(lib, g, [z], seeds, p=1.0, direction=-1, ds=2.0 ** -5, max_steps=4 * (B - 1))
    return path, flow


def same_as_flow_lines(name, path, flow):
    """the stationary cross-check: points and elements bit for bit, DONE <-> MAXSTEPS, EXIT <-> EXIT with the same end point,
    lengths within 2 count eps length (a path adds dt |w|, |w| = 1 to rounding, where a flow line adds ds)"""
    m = len(path.status)
    assert not (flow.status == FR.STALLED).any() and not (path.rested > 0).any(), name
    for i in range(m):
        want = {FR.MAXSTEPS: PR.DONE, FR.EXIT: PR.EXIT}[int(flow.status[0, i])]
        assert path.status[i] == want and path.count[i] == flow.count[0, i], (name, i)
        pp, pe = path.path(i)
        fp, fe = flow.path(0, i)
        assert pp.tobytes() == fp.tobytes() and np.array_equal(pe, fe), (name, i)
        assert path.end[i].tobytes() == flow.end[0, i].tobytes() and path.end_element[i] == flow.end_element[0, i], (name, i)
        assert path.rows[i, 2] == flow.rows[0, i, 2], (name, i)      # u_start; u_end too: both from one snapshot or its own blend
        assert path.rows[i, 3] == flow.rows[0, i, 3], (name, i)
        assert abs(path.rows[i, 0] - flow.rows[0, i, 0]) <= 2 * path.count[i] * FR.EPS * flow.rows[0, i, 0], (name, i)
    assert (path.status == PR.DONE).any() and (path.status == PR.EXIT).any(), name


def test_stationary_field_gives_the_flow_lines(lib):
    g = FU.host_mesh("fem2d", 3)
    path, flow = stationary_pair(lib, g, PU.fields_2d(g.x, 1)[0], FU.seeds_2d(12), 5)
    same_as_flow_lines("fem2d L=3", path, flow)
    g = FU.host_mesh("fem3d", 1, 2)
    path, flow = stationary_pair(lib, g, PU.fields_3d(g.x, 1)[0], FU.seeds_3d(8), 5)
    same_as_flow_lines("fem3d L=1 k=2", path, flow)


def test_rows_do_not_depend_on_the_batch(lib):
    g = FU.host_mesh("fem2d", 3)
    fields, seeds = PU.fields_2d(g.x, 4), FU.seeds_2d(9)
    rel = np.arange(9) % 3
    got = PU.host_path_lines(lib, g, fields, TS4, seeds, release=rel, substeps=3)
    perm = np.array([4, 0, 8, 2, 6, 1, 7, 3, 5])
    mixed = PU.host_path_lines(lib, g, fields, TS4, seeds[perm], release=rel[perm], substeps=3)
    assert mixed.rows.tobytes() == got.rows[perm].tobytes() and mixed.end.tobytes() == got.end[perm].tobytes()
    for a in ("status", "count", "end_element", "rested"):
        assert np.array_equal(getattr(mixed, a), getattr(got, a)[perm])
    for i in (0, 5, 8):
        one = PU.host_path_lines(lib, g, fields, TS4, seeds[i: i + 1], release=rel[i: i + 1], substeps=3)
        assert one.rows.tobytes() == got.rows[i].tobytes() and one.path(0)[0].tobytes() == got.path(i)[0].tobytes()
        assert np.array_equal(one.path(0)[1], got.path(i)[1]) and one.count[0] == got.count[i]


def test_every_release_index(lib):
    """a particle released at ts[r] with stop = s is the particle of the run cut to the snapshots r..s"""
    g = FU.host_mesh("fem2d", 2)
    fields, seeds = PU.fields_2d(g.x, 4), FU.seeds_2d(4)
    for stop in (1, 2, 3):
        for r in range(stop):
            got = PU.host_path_lines(lib, g, fields, TS4, seeds, release=r, stop=stop, substeps=2)
            cut = PU.host_path_lines(lib, g, fields[r: stop + 1], TS4[r: stop + 1], seeds, release=0, substeps=2)
            assert got.rows.tobytes() == cut.rows.tobytes() and got.pts.tobytes() == cut.pts.tobytes()
            assert np.array_equal(got.count, cut.count) and np.array_equal(got.status, cut.status)
            done = got.status == PR.DONE
            assert (got.count[done] == (stop - r) * 2 + 1).all() and (got.rows[done, 1] == TS4[stop]).all()
            PU.against_lines("release %d stop %d" % (r, stop), got, g, fields, TS4, seeds, r, stop, 2, 2.0, -1, 1.0, 1e-12)


def test_rest_and_resume(lib):
    g = FU.host_mesh("fem2d", 2)
    zero = np.zeros(g.n)
    fields, ts, n = [zero, zero, g.x[:, 0].copy()], np.array([0.0, 0.5, 1.0]), 4
    seeds = FU.seeds_2d(5, 0.5)
    got = PU.host_path_lines(lib, g, fields, ts, seeds, substeps=n)
    assert (got.status == PR.DONE).all() and (got.rested == n).all() and (got.count == 2 * n + 1).all()
    for i in range(5):
        pts = got.path(i)[0]
        assert (pts[: n + 1] == seeds[i]).all() and (np.diff(pts[n:, 0]) < 0).all()
    assert np.abs(got.end[:, 0] - (seeds[:, 0] - 0.25)).max() <= 1e-13 and np.abs(got.rows[:, 0] - 0.25).max() <= 1e-13
    PU.against_lines("rest", got, g, fields, ts, seeds, 0, 2, n, 2.0, -1, 1.0, 1e-12)
    PU.replay("rest", got, g, fields, ts, 0, 2, n, 2.0, -1, 1.0, 1e-12)


def test_outside_seeds(lib):
    g = FU.host_mesh("fem2d", 2)
    fields = PU.fields_2d(g.x, 3)
    seeds = np.array([[0.3, 0.2], [1.5, 0.0], [np.nan, 0.1], [0.1, np.inf], [-0.4, 0.7]])
    got = PU.host_path_lines(lib, g, fields, TS3, seeds, release=[0, 1, 0, 1, 1])
    assert np.array_equal(got.status != PR.OUTSIDE, [True, False, False, False, True])
    for i in (1, 2, 3):
        assert np.isnan(got.rows[i]).all() and np.isnan(got.end[i]).all() and got.rested[i] == 0
        assert got.count[i] == 0 and got.end_element[i] == -1 and len(got.path(i)[0]) == 0
    alone = PU.host_path_lines(lib, g, fields, TS3, seeds[[0, 4]], release=[0, 1])
    assert alone.rows.tobytes() == got.rows[[0, 4]].tobytes() and alone.path(1)[0].tobytes() == got.path(4)[0].tobytes()
    PU.against_lines("outside", got, g, fields, TS3, seeds, [0, 1, 0, 1, 1], 2, 4, 2.0, -1, 1.0, 1e-12)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_nodes_reached_and_not_reached(lib, bad):
    g = FU.host_mesh("fem2d", 3)
    fields, seeds = PU.fields_2d(g.x, 3), FU.seeds_2d(6)
    clean = PU.host_path_lines(lib, g, fields, TS3, seeds, substeps=4, speed=2.0)
    # an element that some trajectory enters after its start, and the element farthest from every recorded point
    e, line = next((int(el[k]), i) for i in range(6) for el in [clean.path(i)[1]] for k in range(2, len(el)) if el[k] != el[0])
    cent = g.x.reshape(-1, 7, 2)[:, 6]
    far = int(np.argmax(np.min(((cent[:, None, :] - clean.pts[None, :, :]) ** 2).sum(axis=2), axis=1)))
    for snap in (0, 1, 2):
        poisoned = [z.copy() for z in fields]
        poisoned[snap][7 * far: 7 * far + 7] = bad
        got = PU.host_path_lines(lib, g, poisoned, TS3, seeds, substeps=4, speed=2.0)
        assert got.rows.tobytes() == clean.rows.tobytes() and got.pts.tobytes() == clean.pts.tobytes()      # not reached
        assert np.array_equal(got.status, clean.status)
    first = int(np.flatnonzero(clean.path(line)[1] == e)[0])      # the first recorded point in e: after `first` steps
    for snap in (first // 4, first // 4 + 1):      # snapshot j and j + 1 of the slab in which e is entered
        poisoned = [z.copy() for z in fields]
        poisoned[snap][7 * e: 7 * e + 7] = bad
        got = PU.host_path_lines(lib, g, poisoned, TS3, seeds, substeps=4, speed=2.0)
        assert got.status[line] == PR.NONFINITE and not np.isfinite(got.rows[line, 3])
        assert 1 <= got.count[line] <= first + 1 and np.isfinite(got.rows[line, [0, 1, 2, 4]]).all()
        n = got.count[line]
        assert got.path(line)[0].tobytes() == clean.path(line)[0][:n].tobytes()
        k = n - 1      # stopped at the start of step k: time = t_k
        j, i = k // 4, k % 4
        assert got.rows[line, 1] == TS3[j] + i * ((TS3[j + 1] - TS3[j]) / 4)
        PU.against_lines("non-finite node", got, g, poisoned, TS3, seeds, 0, 2, 4, 2.0, -1, 2.0, 1e-12)


def test_elements_of_negative_determinant(lib):
    g = FU.host_mesh("fem2d", 3, mixed=True)
    xe = g.x.reshape(-1, 7, 2)
    det = (xe[:, 1, 0] - xe[:, 0, 0]) * (xe[:, 2, 1] - xe[:, 0, 1]) - (xe[:, 1, 1] - xe[:, 0, 1]) * (xe[:, 2, 0] - xe[:, 0, 0])
    assert (det < 0).any() and (det > 0).any()
    fields, seeds = PU.fields_2d(g.x, 3), np.vstack([FU.seeds_2d(4), -FU.seeds_2d(4)])      # both triangles
    got = PU.host_path_lines(lib, g, fields, TS3, seeds, substeps=3, speed=2.0)
    used = np.unique(got.elem)
    assert (det[used] < 0).any() and (det[used] > 0).any()
    PU.against_lines("mixed determinants", got, g, fields, TS3, seeds, 0, 2, 3, 2.0, -1, 2.0, 1e-12)
    PU.replay("mixed determinants", got, g, fields, TS3, 0, 2, 3, 2.0, -1, 2.0, 1e-12)


def test_non_convex_mesh(lib):
    """The L shape [-1, 1]^2 without (0, 1]^2 and u = (1 + j) (x + y): particles from the lower left run at 45 degrees into the
    walls of the re-entrant corner or stay inside; every EXIT end point is on the boundary and kept its diagonal"""
    g = FU.host_mesh("fem2d", 3, K=("lshape", MC.LSHAPE))
    fields = [(1.0 + j) * (g.x[:, 0] + g.x[:, 1]) for j in range(3)]
    s0 = np.array([[-0.83 + 0.0917 * i, -0.91 + 0.0531 * i] for i in range(8)])
    s0 = np.vstack([s0, s0[:, ::-1], [[-0.1, 0.3], [0.3, -0.1]]])      # the last two meet the walls x = 0 and y = 0
    got = PU.host_path_lines(lib, g, fields, TS3, s0, substeps=4, direction=1, speed=0.5)
    ex, ey = got.end[:, 0], got.end[:, 1]
    out = got.status == PR.EXIT
    t = (2.0 ** -40 + 2e-12) * np.sqrt(2.0)
    wall = ((np.abs(ex) <= t) & (ey >= -t)) | ((np.abs(ey) <= t) & (ex >= -t)) | (np.abs(ex - 1) <= t) | (np.abs(ey - 1) <= t)
    assert out.any() and (~out).any() and wall[out].all() and (got.status[~out] == PR.DONE).all()
    assert np.abs((ex - ey) - (s0[:, 0] - s0[:, 1])).max() <= 1e-12
    PU.against_lines("L shape", got, g, fields, TS3, s0, 0, 2, 4, 2.0, 1, 0.5, 1e-12)
    PU.replay("L shape", got, g, fields, TS3, 0, 2, 4, 2.0, 1, 0.5, 1e-12)


def test_argument_errors(lib):
    """every MGB_E_ARG line of the header; the outputs keep their prefill: nothing was written"""
    g = FU.host_mesh("fem2d", 2)
    z, seeds = np.zeros((g.n, 2)), FU.seeds_2d(3)
    fields = [z, z, z]
    ok = dict(rc_only=True)
    assert PU.host_path_lines(lib, g, fields, TS3, seeds, **ok)[0] == 0
    bad = (dict(B=1), dict(B=65536), dict(stop=0), dict(stop=3), dict(stop=-1), dict(release=2), dict(release=-1), dict(release=[0, 1, 2]),
           dict(substeps=0), dict(substeps=-2), dict(p=0.5), dict(p=np.nan), dict(p=np.inf), dict(speed=0.0), dict(speed=-1.0),
           dict(speed=np.nan), dict(speed=np.inf), dict(gmin=-1e-3), dict(gmin=np.nan), dict(gmin=np.inf), dict(direction=0),
           dict(direction=2), dict(S=0), dict(u=2), dict(u=-1), dict(m=-1))
    for kw in bad:
        assert PU.host_path_lines(lib, g, fields, TS3, seeds, **{**ok, **kw}) == (PU.MGB_E_ARG, True), kw
        assert b"path_lines" in lib.mgb_last_error()
    for ts in ([0.0, 0.125, 0.125], [0.0, 0.25, 0.125], [0.0, np.nan, 0.375], [0.0, 0.125, np.inf]):
        assert PU.host_path_lines(lib, g, fields, ts, seeds, **ok) == (PU.MGB_E_ARG, True), ts
    assert PU.host_path_lines(lib, g, fields, TS3, np.empty((0, 2)), **ok)[0] == 0      # m = 0: at once
    from mgb_amd import _lib
    rows, end = np.full((3, 5), 7.0), np.full((3, 2), 7.0)
    ints = [np.full(3, -7, dtype=np.int32) for _ in range(4)]
    rel, ts = np.zeros(3, dtype=np.int32), TS3.copy()
    table = (_lib.c_dbl_p * 3)(*[_lib.dptr(z)] * 3)

    def call(h=g.handle, tab=table, t=_lib.dptr(ts), sd=_lib.dptr(seeds), rl=_lib.iptr(rel), r=_lib.dptr(rows), e=_lib.dptr(end),
             i0=_lib.iptr(ints[0]), i3=_lib.iptr(ints[3]), off=None, pts=None, el=None, cap=0, n=4, S=2):
        return lib.mgb_geo_path_lines_host(h, 3, tab, t, S, 0, 3, sd, rl, 2, n, 2.0, -1, 1.0, 1e-12, r, e, i0, _lib.iptr(ints[1]),
                                           _lib.iptr(ints[2]), i3, off, pts, el, cap)
    assert call() == 0
    rows[:], end[:] = 7.0, 7.0
    for a in ints:
        a[:] = -7
    g1 = FU.LU.host_mesh("fem1d", 3)
    t1 = (_lib.c_dbl_p * 3)(*[_lib.dptr(np.zeros(g1.n))] * 3)
    assert call(h=g1.handle, tab=t1, S=1) == PU.MGB_E_ARG      # 1-D
    nulls = (dict(h=None), dict(tab=None), dict(t=None), dict(sd=None), dict(rl=None), dict(r=None), dict(e=None), dict(i0=None),
             dict(i3=None), dict(tab=(_lib.c_dbl_p * 3)(_lib.dptr(z), None, _lib.dptr(z))))
    for kw in nulls:
        assert call(**kw) == PU.MGB_E_ARG, kw
    # paths: the three arrays come together, hold what is recorded, and stay inside 2^31 - 1 entries of the fixed-stride buffer
    off, pts, el = np.empty(4, dtype=np.int64), np.empty((3, 2)), np.empty(3, dtype=np.int32)
    offp = off.ctypes.data_as(_lib.c_ll_p)
    assert call(off=offp, pts=_lib.dptr(pts), cap=3) == PU.MGB_E_ARG
    assert call(off=offp, pts=_lib.dptr(pts), el=_lib.iptr(el), cap=-1) == PU.MGB_E_ARG
    assert call(off=offp, pts=_lib.dptr(pts), el=_lib.iptr(el), cap=3, n=2 ** 28) == PU.MGB_E_ARG
    assert b"2^31" in lib.mgb_last_error()
    assert (rows == 7.0).all() and (end == 7.0).all() and all((a == -7).all() for a in ints)
    assert call(off=offp, pts=_lib.dptr(pts), el=_lib.iptr(el), cap=3) == PU.MGB_E_ARG      # too small: 3 x 9 points are recorded


def test_python_names_and_header():
    import os
    import mgb_amd as M
    assert {"path_lines", "PathLines"} <= set(M.__all__)
    P = M.PathLines
    assert (P.DONE, P.EXIT, P.OUTSIDE, P.NONFINITE) == (0, 1, 2, 3)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgb_hip.h")).read()
    for name, v in (("COLS", 5), ("DONE", 0), ("EXIT", 1), ("OUTSIDE", 2), ("NONFINITE", 3)):
        assert "#define MGB_PATH_%s %d\n" % (name, v) in hdr
    with pytest.raises(TypeError, match="flow_lines"):
        M.path_lines(object(), np.zeros((1, 2)))


def test_object_file_shares_no_arithmetic_with_other_objects():
    """pathline.hip is compiled with contraction off and linked last; like flowline.o (test_flowline_host.py) its object must
    define no weak function of the shared namespaces, or the link order would decide whose bits both sides compute."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "multigridbarriermpi.jl_amd", "csrc", "_obj", "pathline.o")
    if not os.path.exists(obj) or shutil.which("nm") is None:
        return      # a tree that was not built here (the objects do not travel): the GPU tests hold device and host to the same bits
    out = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    weak = [l for l in out.splitlines() if len(l.split()) > 2 and l.split()[1] in "WwVv"]
    shared = [l for l in weak if "mgb::interp::" in l or "mgb::flowline::" in l or "mgb::pathline::" in l]
    assert not shared, shared
