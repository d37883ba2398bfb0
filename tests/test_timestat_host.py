"""CPU tests of the host restatement mgb_geo_time_stats_host (csrc/timestat.hpp: the per-node routines the gfx950 kernel also
runs) against the exact yardstick tests/timestat_reference.py under the bars of tests/timestat_util.py.

Shapes: fem1d L=3 with B=2, the smallest run there is; fem2d L=2 with S=2, u=1 and non-uniform times, some negative; B=9 with 9
levels, one above and one below every value, some equal to snapshot values.

Largest ratios to the bars seen (printed by every run): change 0.50, integral 0.13, variation 0.15, rate 0.17, arrival 0.08,
left 0.06, exposure 0.07, excess 0.06, totals 0.03."""
import ctypes as C

import numpy as np
import pytest

import timestat_reference as TR
import timestat_util as TU

NAN = float("nan")


def fields_of(Z, S=1, u=0, seed=0):
    """the (B, n) values as B fields of S columns with the values in column u and noise elsewhere"""
    rng = np.random.default_rng(seed)
    out = []
    for row in Z:
        z = rng.standard_normal((len(row), S))
        z[:, u] = row
        out.append(z)
    return out


def test_the_smallest_run(lib):
    g = TU.host_mesh("fem1d", 3)
    assert g.n == 16
    ts = np.array([0.25, 0.75])
    Z = TU.front(g.x, ts)
    got = TU.host_time_stats(lib, g, fields_of(Z), ts, [0.1])
    TU.against_reference("fem1d L=3 B=2", got, TR.Reference(Z, ts, [0.1], g.w), NAN)
    assert (got.level[0, :, 4] >= 0).all() and got.level[0, :, 4].max() == 1.0


def test_a_column_stride_and_non_uniform_times(lib):
    g = TU.host_mesh("fem2d", 2)
    assert g.n == 56
    ts = np.array([-1.5, -0.75, -0.125, 0.5, 2.0])
    rng = np.random.default_rng(3)
    Z = np.where(rng.random((5, g.n)) < 0.5, TU.front(g.x, ts + 1.5), rng.standard_normal((5, g.n)))
    levels = [-0.5, 0.0, 0.6]
    got = TU.host_time_stats(lib, g, fields_of(Z, S=2, u=1), ts, levels, never=7.5, u=1)
    TU.against_reference("fem2d L=2 S=2 u=1", got, TR.Reference(Z, ts, levels, g.w), 7.5)
    again = TU.host_time_stats(lib, g, fields_of(Z, S=2, u=1, seed=9), ts, levels, never=7.5, u=1)      # the other column does not matter
    assert again.node.tobytes() == got.node.tobytes() and again.level.tobytes() == got.level.tobytes()
    assert again.rows.tobytes() == got.rows.tobytes()
    none = TU.host_time_stats(lib, g, fields_of(Z, S=2, u=1), ts, None, u=1)
    assert none.node.tobytes() == got.node.tobytes() and none.rows.shape == (1, 5) and none.rows[0, 3:].tobytes() == got.rows[0, 3:].tobytes()


def test_nine_snapshots_and_nine_levels(lib):
    g = TU.host_mesh("fem2d", 2)
    rng = np.random.default_rng(5)
    ts = np.cumsum(rng.uniform(0.05, 0.4, 9)) - 0.6
    Z = np.round(0.7 * TU.front(g.x, ts + 0.6) + 0.3 * rng.standard_normal((9, g.n)), 2)      # values rounded onto levels
    levels = np.array([Z.max() + 1.0, Z.min() - 1.0, 0.25, -0.25, 0.0, 0.5, Z[3, 11], Z[0, 0], Z[8, 55]])
    got = TU.host_time_stats(lib, g, fields_of(Z), ts, levels, never=np.inf)
    R = TR.Reference(Z, ts, levels, g.w)
    TU.against_reference("fem2d L=2 B=9 nl=9", got, R, np.inf)
    assert (got.level[0, :, 0] == np.inf).all() and (got.level[0, :, 1] == np.inf).all() and (got.level[0, :, 2:] == 0.0).all()
    assert got.rows[1].tolist() == [0.0, 0.0, 0.0, -np.inf, 0.0]
    span = ts[-1] - ts[0]
    assert (got.level[1, :, 0] == ts[0]).all() and (got.level[1, :, 4] == 1.0).all() and abs(got.rows[2, 4] - span) <= 16 * TR.EPS * span
    for l in range(9):      # a level's table and row do not depend on the other levels
        one = TU.host_time_stats(lib, g, fields_of(Z), ts, [levels[l]], never=np.inf)
        assert one.level[0].tobytes() == got.level[l].tobytes() and one.rows[1].tobytes() == got.rows[1 + l].tobytes()


def series_on(g, series, B, fill=0.0):
    """(B, n) values: node i carries series[i], the others `fill`"""
    Z = np.full((B, g.n), fill)
    for i, s in enumerate(series):
        Z[:, i] = s
    return Z


@pytest.mark.parametrize("never", [NAN, 7.5, np.inf])
def test_exact_cases(lib, never):
    g = TU.host_mesh("fem1d", 3)
    ts = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
    c = 0.5
    series = [[0.0, 0.5, 1.0, 0.5, 0.0],      # 0: a value equal to the level at a snapshot is not above
              [0.0, 0.5, 0.5, 0.5, 0.0],      # 1: a plateau on the level gives no entry
              [1.0, 1.0, 0.0, 0.0, 0.0],      # 2: v_0 > c
              [0.0, 1.0, 0.0, 1.0, 0.0],      # 3: up, down, up, down
              [0.0, 1.0, 0.0, 1.0, 1.0]]      # 4: up, down, up
    Z = series_on(g, series, 5)
    got = TU.host_time_stats(lib, g, fields_of(Z), ts, [c, 2.0], never=never)
    TU.against_reference("exact cases", got, TR.Reference(Z, ts, [c, 2.0], g.w), never)
    L = got.level[0]
    same = lambda v: TU._same_never(v, never)
    assert L[0].tolist() == [1.0, 3.0, 2.0, 0.5, 1.0]                     # above on (1, 3) only: the triangle of height 1/2
    assert same(L[1, 0]) and same(L[1, 1]) and L[1, 2:].tolist() == [0.0, 0.0, 0.0]
    assert L[2, 0] == ts[0] and L[2, 4] == 1.0 and L[2, 1] == 1.5 and L[2, 2] == 1.5
    assert L[3].tolist() == [0.5, 3.5, 2.0, 0.5, 2.0]                   # the first arrival and the last left are kept
    assert L[4, 0] == 0.5 and L[4, 1] == 1.5 and L[4, 4] == 2.0 and L[4, 2] == 2.5
    assert same(L[5:, 0]).all() and same(L[5:, 1]).all() and (L[5:, 2:] == 0.0).all()
    top = got.level[1]                                                     # a level above everything
    assert same(top[:, 0]).all() and same(top[:, 1]).all() and (top[:, 2:] == 0.0).all()
    assert got.rows[2].tolist() == [0.0, 0.0, 0.0, -np.inf, 0.0]
    assert got.rows[1, 3] == 1.0 and got.rows[1, 4] == 2.5                # node 0 arrives last, node 4 stays longest
    N = got.node
    assert N[3].tolist() == [2.0, 1.0, 1.0, 0.0, 0.0, 4.0, 1.0, 0.0]      # the FIRST maximum and the first minimum
    assert N[2].tolist() == [1.5, 1.0, 0.0, 0.0, 2.0, 1.0, 1.0, -1.0]


@pytest.mark.parametrize("what", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_poisons_its_node_alone(lib, what):
    g = TU.host_mesh("fem1d", 3)
    ts = np.array([0.0, 0.5, 1.5, 2.0])
    rng = np.random.default_rng(11)
    Z = rng.standard_normal((4, g.n))
    clean = TU.host_time_stats(lib, g, fields_of(Z), ts, [0.1, -0.3], never=7.5)
    Zb = Z.copy()
    Zb[2, 5] = what
    got = TU.host_time_stats(lib, g, fields_of(Zb), ts, [0.1, -0.3], never=7.5)
    TU.against_reference("non-finite %r" % what, got, TR.Reference(Zb, ts, [0.1, -0.3], g.w), 7.5)
    assert np.isnan(got.node[5]).all() and np.isnan(got.level[:, 5]).all() and np.isnan(got.rows).all()
    keep = np.arange(g.n) != 5
    assert got.node[keep].tobytes() == clean.node[keep].tobytes() and got.level[:, keep].tobytes() == clean.level[:, keep].tobytes()
    assert np.isfinite(clean.rows).all()


def test_argument_errors(lib):
    from mgb_amd import _lib
    g = TU.host_mesh("fem1d", 3)
    ts = np.array([0.0, 1.0, 2.0])
    Z = np.random.default_rng(1).standard_normal((3, g.n))
    f = fields_of(Z)
    rc = lambda ts_=ts, levels=[0.1], fields=f, **over: TU.host_time_stats(lib, g, fields, ts_, levels, rc_only=True, **over)
    assert rc() == 0
    assert rc(levels=None) == 0 and rc(levels=None, level=None) == 0
    for over in (dict(geo=None), dict(table=None), dict(times=None), dict(node=None), dict(out=None), dict(levels=None, nl=1), dict(level=None),
                 dict(B=1), dict(B=0), dict(nl=-1), dict(S=0), dict(u=1), dict(u=-1)):
        assert rc(**over) == TU.MGB_E_ARG, over
    null_field = (_lib.c_dbl_p * 3)(_lib.dptr(f[0]), None, _lib.dptr(f[2]))
    assert rc(table=null_field) == TU.MGB_E_ARG and b"null field" in lib.mgb_last_error()
    for bad_ts in ([0.0, np.nan, 2.0], [0.0, np.inf, 2.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0]):
        assert rc(ts_=np.array(bad_ts)) == TU.MGB_E_ARG, bad_ts
    assert rc(levels=[0.1, np.nan]) == TU.MGB_E_ARG and rc(levels=[np.inf]) == TU.MGB_E_ARG
    assert rc(levels=np.zeros(4097)) == TU.MGB_E_ARG and b"4096" in lib.mgb_last_error()
    # an output that is also an input or the other output
    node, level, out = np.full((g.n, 8), 7.0), np.full((1, g.n, 5), 7.0), np.full((2, 5), 7.0)
    assert rc(level=_lib.dptr(node), node=_lib.dptr(node)) == TU.MGB_E_ARG
    assert rc(out=_lib.dptr(node), node=_lib.dptr(node)) == TU.MGB_E_ARG
    assert rc(out=_lib.dptr(level), level=_lib.dptr(level)) == TU.MGB_E_ARG
    big = np.zeros((g.n, 8))
    tab = (_lib.c_dbl_p * 3)(_lib.dptr(f[0]), _lib.dptr(big), _lib.dptr(f[2]))
    assert rc(table=tab, node=_lib.dptr(big)) == TU.MGB_E_ARG and b"also an input" in lib.mgb_last_error()
    assert rc(table=tab, level=_lib.dptr(big)) == TU.MGB_E_ARG
    assert rc(table=tab, out=_lib.dptr(big)) == TU.MGB_E_ARG
    assert (big == 0.0).all()
    assert lib.mgb_geo_time_stats(None, 3, None, None, 1, 0, 0, None, 0.0, None, None, None) == TU.MGB_E_ARG      # the device entry point: null before any context


def test_python_names_and_header():
    import os
    import mgb_amd as M
    assert {"time_stats", "TimeStats"} <= set(M.__all__)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgb_hip.h")).read()
    assert "#define MGB_TIMESTAT_NODE_COLS 8\n" in hdr and "#define MGB_TIMESTAT_LEVEL_COLS 5\n" in hdr
    with pytest.raises(TypeError):
        M.time_stats(np.zeros(3))


def test_object_file_shares_no_arithmetic_with_other_objects():
    """timestat.hip is compiled with contraction off, most other files with it on: where the object file of the build is at
    hand it must define no weak function of the shared namespaces (the check of test_flowline_host.py)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    obj = os.path.join(root, "multigridbarriermpi.jl_amd", "csrc", "_obj", "timestat.o")
    if not os.path.exists(obj) or shutil.which("nm") is None:
        # a tree that was not built in place: the GPU tests hold device and host to the same bits
        pytest.skip("timestat.o of an in-place build and nm are needed to list the object's weak symbols")
    out = subprocess.run(["nm", "-C", "--defined-only", obj], check=True, capture_output=True, text=True).stdout
    weak = [l for l in out.splitlines() if len(l.split()) > 2 and l.split()[1] in "WwVv"]
    shared = [l for l in weak if "mgb::interp::" in l or "mgb::timestat::" in l or "mgb::levelset::" in l or "mgb::reduce::" in l]
    assert not shared, shared
