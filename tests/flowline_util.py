"""What test_flowline_host.py and test_gpu_flow_lines.py share: host geometries, the call of mgb_geo_flow_lines_host, the
comparison of a library result with the yardstick tests/flowline_reference.py (whole lines and the one-step replay) and of a
device result with the host restatement.  Not a test."""
import ctypes as C

import numpy as np

import flowline_reference as FR
import isosurface_util as IU
import levelset_util as LU

MGB_E_ARG = -1
_HOST = {}


def host_mesh(kind, L, k=None, K=None, mixed=False):
    """fem2d level L (K: a named array of coarse triangles, mixed: levelset_util's two triangles of opposite orientation) or
    fem3d level L of degree k; built once."""
    if kind == "fem3d":
        return IU.host_mesh(L, k)
    if K is None:
        return LU.host_mesh("fem2d", L, mixed)
    key = (L, K[0])
    if key not in _HOST:
        _HOST[key] = LU.HostMesh("fem2d", L, K[1])
    return _HOST[key]


def mesh_of(g):
    """the yardstick's Mesh of a host geometry, built once"""
    if getattr(g, "_flow_mesh", None) is None:
        g._flow_mesh = FR.Mesh(g.x, g.block)
    return g._flow_mesh


class Result:
    """rows (B, m, 4), end (B, m, dim), status, count, end_element (B, m), ds, offsets (B m + 1), pts (total, dim), elem (total,)"""

    def __init__(self, rows, end, status, count, end_element, ds, offsets, pts, elem):
        self.rows, self.end, self.status, self.count, self.end_element = rows, end, status, count, end_element
        self.ds, self.offsets, self.pts, self.elem = ds, offsets, pts, elem

    def path(self, b, i):
        r = b * self.count.shape[1] + i
        a, e = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.pts[a:e], self.elem[a:e]


def host_flow_lines(lib, g, fields, seeds, p=2.0, direction=1, ds=None, max_steps=256, gmin=1e-12, u=0, paths=True, rc_only=False,
                    S=None, B=None, m=None):
    """mgb_geo_flow_lines_host on a host mesh: `fields` a list of (n,) or (n, S) arrays.  Two calls: the counts, then the points
    in arrays of exactly that size.  Outputs are prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    dim = g.x.shape[1]
    fields = [_lib.f64(z).reshape(g.x.shape[0], -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    seeds = _lib.f64(np.asarray(seeds).reshape(-1, dim))
    m = seeds.shape[0] if m is None else m
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    Bm, mm = max(B, 1), max(m, 1)
    rows, end = np.full((Bm, mm, 4), 7.0), np.full((Bm, mm, dim), 7.0)
    status, count, eel = (np.full((Bm, mm), -7, dtype=np.int32) for _ in range(3))
    dsv = C.c_double(0.0 if ds is None else ds)      # kept alive for both calls
    dsp = None if ds is None else C.cast(C.byref(dsv), _lib.c_dbl_p)
    used = C.c_double(-7.0)
    up = C.cast(C.byref(used), _lib.c_dbl_p)
    ll = lambda a: None if a is None else a.ctypes.data_as(_lib.c_ll_p)
    rc = lib.mgb_geo_flow_lines_host(g.handle, B, table, S, u, m, _lib.dptr(seeds), p, direction, dsp, max_steps, gmin, _lib.dptr(rows),
                                     _lib.dptr(end), _lib.iptr(status), _lib.iptr(count), _lib.iptr(eel), up, None, None, None, 0)
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    rows, end, status, count, eel = rows[:B, :m], end[:B, :m], status[:B, :m], count[:B, :m], eel[:B, :m]
    if not paths:
        return Result(rows, end, status, count, eel, used.value, None, None, None)
    total = int(count.sum())
    offsets = np.full(B * m + 1, -7, dtype=np.int64)
    pts, elem = np.full((total, dim), 7.0), np.full(total, -7, dtype=np.int32)
    rows2, end2 = np.full((B, m, 4), 7.0), np.full((B, m, dim), 7.0)
    status2, count2, eel2 = (np.full((B, m), -7, dtype=np.int32) for _ in range(3))
    rc = lib.mgb_geo_flow_lines_host(g.handle, B, table, S, u, m, _lib.dptr(seeds), p, direction, dsp, max_steps, gmin, _lib.dptr(rows2),
                                     _lib.dptr(end2), _lib.iptr(status2), _lib.iptr(count2), _lib.iptr(eel2), up, ll(offsets),
                                     _lib.dptr(pts), _lib.iptr(elem), total)
    assert rc == 0, lib.mgb_last_error()
    assert rows2.tobytes() == np.ascontiguousarray(rows).tobytes() and end2.tobytes() == np.ascontiguousarray(end).tobytes()
    assert np.array_equal(status2, status) and np.array_equal(count2, count) and np.array_equal(eel2, eel)
    return Result(rows2, end2, status2, count2, eel2, used.value, offsets, pts, elem)


def device_result(fl):
    """The same Result from a FlowLines of the Python interface."""
    B, m = fl._shape
    r = lambda a: np.asarray(a).reshape(B, m)
    return Result(fl.rows, np.asarray(fl.end).reshape(B, m, -1), r(fl.status), r(fl.count), r(fl.end_element), fl.ds, fl._offsets,
                  fl._pts, fl._elem)


def seeds_2d(m, scale=1.0):
    """fixed irrational-looking offsets: no seed on a mesh line of L <= 5"""
    i = np.arange(m)
    x = -0.83 + 0.0917 * i
    y = 0.41 - 0.0531 * i
    wrap = lambda t: ((t + 0.97) % 1.94) - 0.97
    return np.stack([wrap(x), wrap(y)], axis=1) * scale


def seeds_3d(m):
    """inside the cube [-1, 1]^3 of fem3d, away from the planes of L <= 3"""
    i = np.arange(m)
    wrap = lambda t: ((t + 0.97) % 1.94) - 0.97
    return np.stack([wrap(-0.83 + 0.0917 * i), wrap(0.41 - 0.0531 * i), wrap(0.29 + 0.0713 * i)], axis=1)


def against_lines(name, got, g, fields, seeds, p, direction, max_steps, gmin, u=0, ds=None):
    """Whole lines: status, count, the element of every point and the end element equal to the yardstick's own trace from the
    seed; an OUTSIDE row is NaN.  (Points, lengths and times are held to the yardstick step by step: replay().)"""
    M = mesh_of(g)
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, M.dim)
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(g.x.shape[0], -1)[:, u]
        F = FR.Field(M, z)
        for i, s in enumerate(seeds):
            R = FR.trace(M, F, s, p, direction, got.ds if ds is None else ds, max_steps, gmin)
            who = "%s field %d seed %d" % (name, b, i)
            assert got.status[b, i] == R.status, (who, got.status[b, i], R.status)
            assert got.count[b, i] == R.count, (who, got.count[b, i], R.count)
            assert got.end_element[b, i] == R.end_element, who
            if got.offsets is not None:
                pts, el = got.path(b, i)
                assert np.array_equal(el, R.elems), who
            if R.status == FR.OUTSIDE:
                assert np.isnan(got.rows[b, i]).all() and np.isnan(got.end[b, i]).all(), who


def replay(name, got, g, fields, p, direction, max_steps, gmin, u=0, cap=0.01):
    """The one-step replay of every recorded point of every line of `got` against the yardstick: the next recorded point inside
    its bar and in the yardstick's element; undecided steps are left out and counted.  The length and the time of a line none of
    whose steps is undecided are held to the sums of the replayed steps' own terms (taken from the library's points: nothing
    accumulates against the yardstick) within the sum of their bars plus count eps of the sum for the serial additions; u_start
    and u_end to the yardstick's values at the library's points.  Prints the largest ratios and the undecided share; asserts the
    bars, the 1 % cap and that no line is left out as a whole."""
    M = mesh_of(g)
    worst, wsum, steps, undecided = 0.0, 0.0, 0, 0
    B, m = got.count.shape
    for b in range(B):
        z = np.asarray(fields[b], dtype=np.float64).reshape(g.x.shape[0], -1)[:, u]
        F = FR.Field(M, z)
        for i in range(m):
            pts, el = got.path(b, i)
            n = len(pts)
            if n < 2:
                continue
            checked = 0
            tot, tbar, whole = np.zeros(2, dtype=FR.LD), np.zeros(2, dtype=FR.LD), True
            for k in range(n - 1):
                s = FR.step(F, pts[k].astype(FR.LD), int(el[k]), k, p, direction, got.ds, max_steps, gmin)
                steps += 1
                if s.undecided and s.kind != "exit":
                    undecided += 1
                    whole = False
                    continue
                who = "%s field %d seed %d step %d" % (name, b, i, k)
                assert s.kind in ("step", "exit") and s.recorded, (who, s.kind)
                bar = s.exit_bar if s.kind == "exit" else s.bar
                if s.kind == "exit":
                    assert k == n - 2 and got.status[b, i] == FR.EXIT, who
                else:
                    assert s.e == el[k + 1], (who, s.e, el[k + 1])
                gap = np.abs(pts[k + 1].astype(FR.LD) - s.x).max()
                worst = max(worst, float(gap / bar))
                assert gap <= bar, (who, float(gap), float(bar))
                checked += 1
                tot += [s.dlength, s.dtime]
                tbar += [s.lbar, s.tbar]
            if whole and got.status[b, i] != FR.EXIT or (whole and s.kind == "exit"):
                # every accepted step and the exit were replayed (an exit with lo = 0 records no point: such a line is left out)
                who = "%s field %d seed %d" % (name, b, i)
                sums = np.abs(got.rows[b, i, :2].astype(FR.LD) - tot)
                sbar = tbar + n * FR.EPS * tot
                wsum = max(wsum, float((sums / sbar).max()))
                assert (sums <= sbar).all(), (who, sums, sbar)
                v0, v1 = F.value(int(el[0]), pts[0].astype(FR.LD)), F.value(int(el[-1]), pts[-1].astype(FR.LD))
                assert abs(got.rows[b, i, 2] - v0) <= F.value_bar(int(el[0]), pts[0].astype(FR.LD)), who
                assert abs(got.rows[b, i, 3] - v1) <= F.value_bar(int(el[-1]), pts[-1].astype(FR.LD)), who
                assert got.end[b, i].tobytes() == pts[-1].tobytes() and got.end_element[b, i] == el[-1], who
            assert checked > 0, "%s field %d seed %d: every step undecided" % (name, b, i)
    share = undecided / max(steps, 1)
    print("%s: %d steps replayed, largest ratio to the bar: points %.3f, length and time %.3f; undecided %d (%.3f %%)"
          % (name, steps, worst, wsum, undecided, 100 * share))
    assert steps > 0 and share <= cap, (name, share)
    return worst, share


def same_as_host(name, dev, host, p, exact_time=None):
    """Device Result against the host Result: everything discrete equal; points, end, length, u_start, u_end bit for bit; time bit
    for bit for p = 1 and p = 2, else within 4 eps times the sum of the absolute terms (all terms are positive: the time itself)."""
    assert np.array_equal(dev.status, host.status), name
    assert np.array_equal(dev.count, host.count) and np.array_equal(dev.end_element, host.end_element), name
    assert dev.ds == host.ds, name
    for k in (0, 2, 3):
        assert np.ascontiguousarray(dev.rows[..., k]).tobytes() == np.ascontiguousarray(host.rows[..., k]).tobytes(), (name, k)
    assert np.ascontiguousarray(dev.end).tobytes() == np.ascontiguousarray(host.end).tobytes(), name
    td, th = np.ascontiguousarray(dev.rows[..., 1]), np.ascontiguousarray(host.rows[..., 1])
    if p in (1.0, 2.0):
        assert td.tobytes() == th.tobytes(), name
    else:
        ok = np.isfinite(th)
        assert np.array_equal(np.isnan(td), np.isnan(th)) and np.array_equal(np.isinf(td), np.isinf(th)), name
        gap = np.abs(td[ok] - th[ok])
        bar = 4 * FR.EPS * np.abs(th[ok])
        print("%s: time, largest ratio to 4 eps sum |terms|: %.3f" % (name, float((gap / np.where(bar > 0, bar, 1)).max()) if ok.any() else 0.0))
        assert (gap <= bar).all(), name
    if host.offsets is not None and dev.offsets is not None:
        assert np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.elem, host.elem), name
        assert dev.pts.tobytes() == host.pts.tobytes(), name
