"""What test_pathline_host.py and test_gpu_path_lines.py share: the call of mgb_geo_path_lines_host, the comparison of a library
result with the yardstick tests/pathline_reference.py (whole trajectories and the one-step replay) and of a device result with
the host restatement.  Not a test."""
import numpy as np

import flowline_reference as FR
import flowline_util as FU
import pathline_reference as PR

MGB_E_ARG = FU.MGB_E_ARG


class Result:
    """rows (m, 5), end (m, dim), status, count, end_element, rested (m,), offsets (m + 1), pts (total, dim), elem (total,)"""

    def __init__(self, rows, end, status, count, end_element, rested, offsets, pts, elem):
        self.rows, self.end, self.status, self.count, self.end_element, self.rested = rows, end, status, count, end_element, rested
        self.offsets, self.pts, self.elem = offsets, pts, elem

    def path(self, i):
        a, e = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.pts[a:e], self.elem[a:e]


def host_path_lines(lib, g, fields, ts, seeds, release=0, stop=None, substeps=4, p=2.0, direction=-1, speed=1.0, gmin=1e-12, u=0,
                    paths=True, rc_only=False, S=None, B=None, m=None):
    """mgb_geo_path_lines_host on a host mesh: `fields` a list of (n,) or (n, S) arrays.  Two calls: the counts, then the points
    in arrays of exactly that size.  Outputs are prefilled so that an unwritten word shows; with rc_only the status code and
    whether every output still holds its prefill are returned."""
    from mgb_amd import _lib
    dim = g.x.shape[1]
    fields = [_lib.f64(z).reshape(g.x.shape[0], -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    stop = len(fields) - 1 if stop is None else stop
    ts = _lib.f64(np.asarray(ts, dtype=np.float64))
    seeds = _lib.f64(np.asarray(seeds).reshape(-1, dim))
    m = seeds.shape[0] if m is None else m
    rel = np.ascontiguousarray(np.broadcast_to(np.asarray(release), (seeds.shape[0],)), dtype=np.int32)
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    mm = max(m, 1)
    rows, end = np.full((mm, 5), 7.0), np.full((mm, dim), 7.0)
    status, count, eel, rested = (np.full(mm, -7, dtype=np.int32) for _ in range(4))
    ll = lambda a: None if a is None else a.ctypes.data_as(_lib.c_ll_p)
    rc = lib.mgb_geo_path_lines_host(g.handle, B, table, _lib.dptr(ts), S, u, m, _lib.dptr(seeds), _lib.iptr(rel), stop, substeps, p,
                                     direction, speed, gmin, _lib.dptr(rows), _lib.dptr(end), _lib.iptr(status), _lib.iptr(count),
                                     _lib.iptr(eel), _lib.iptr(rested), None, None, None, 0)
    if rc_only:
        untouched = (rows == 7.0).all() and (end == 7.0).all() and all((a == -7).all() for a in (status, count, eel, rested))
        return rc, bool(untouched)
    assert rc == 0, lib.mgb_last_error()
    rows, end, status, count, eel, rested = rows[:m], end[:m], status[:m], count[:m], eel[:m], rested[:m]
    if not paths:
        return Result(rows, end, status, count, eel, rested, None, None, None)
    total = int(count.sum())
    offsets = np.full(m + 1, -7, dtype=np.int64)
    pts, elem = np.full((total, dim), 7.0), np.full(total, -7, dtype=np.int32)
    rows2, end2 = np.full((m, 5), 7.0), np.full((m, dim), 7.0)
    status2, count2, eel2, rested2 = (np.full(m, -7, dtype=np.int32) for _ in range(4))
    rc = lib.mgb_geo_path_lines_host(g.handle, B, table, _lib.dptr(ts), S, u, m, _lib.dptr(seeds), _lib.iptr(rel), stop, substeps, p,
                                     direction, speed, gmin, _lib.dptr(rows2), _lib.dptr(end2), _lib.iptr(status2), _lib.iptr(count2),
                                     _lib.iptr(eel2), _lib.iptr(rested2), ll(offsets), _lib.dptr(pts), _lib.iptr(elem), total)
    assert rc == 0, lib.mgb_last_error()
    assert rows2.tobytes() == np.ascontiguousarray(rows).tobytes() and end2.tobytes() == np.ascontiguousarray(end).tobytes()
    assert np.array_equal(status2, status) and np.array_equal(count2, count) and np.array_equal(eel2, eel)
    assert np.array_equal(rested2, rested)
    return Result(rows2, end2, status2, count2, eel2, rested2, offsets, pts, elem)


def device_result(pl):
    """The same Result from a PathLines of the Python interface."""
    return Result(pl.rows, pl.end, pl.status, pl.count, pl.end_element, pl.rested, pl._offsets, pl._pts, pl._elem)


def _columns(g, fields, u):
    M = FU.mesh_of(g)
    return M, [FR.Field(M, np.asarray(z, dtype=np.float64).reshape(g.x.shape[0], -1)[:, u]) for z in fields]


def against_lines(name, got, g, fields, ts, seeds, release, stop, substeps, p, direction, speed, gmin, u=0):
    """Whole trajectories: status, count, rested, the element of every point and the end element equal to the yardstick's own
    trace from the seed; an OUTSIDE row is NaN.  A trajectory one of whose steps the yardstick calls undecided is left out and
    counted; returns (trajectories compared, left out)."""
    M, F = _columns(g, fields, u)
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, M.dim)
    rel = np.broadcast_to(np.asarray(release), (len(seeds),))
    done = skipped = 0
    for i, s in enumerate(seeds):
        R = PR.trace(M, F, ts, s, int(rel[i]), stop, substeps, p, direction, speed, gmin)
        if R.undecided:
            skipped += 1
            continue
        done += 1
        who = "%s seed %d" % (name, i)
        assert got.status[i] == R.status, (who, got.status[i], R.status)
        assert got.count[i] == R.count, (who, got.count[i], R.count)
        assert got.rested[i] == R.rested, (who, got.rested[i], R.rested)
        assert got.end_element[i] == R.end_element, who
        if got.offsets is not None:
            assert np.array_equal(got.path(i)[1], R.elems), who
        if R.status == PR.OUTSIDE:
            assert np.isnan(got.rows[i]).all() and np.isnan(got.end[i]).all(), who
    assert done > 0, name
    return done, skipped


def replay(name, got, g, fields, ts, release, stop, substeps, p, direction, speed, gmin, u=0, cap=0.01):
    """The one-step replay of every recorded point of every trajectory of `got` against the yardstick, each at its own place
    (slab, step) in time: the next recorded point inside its bar and in the yardstick's element, the rest decision equal;
    undecided steps are left out and counted.  The length of a trajectory none of whose steps is undecided is held to the sum of
    the replayed steps' own terms within the sum of their bars plus count eps of the sum; its exit time to the yardstick's within
    its bar; u_start and u_end to the yardstick's values at the library's points.  Prints the largest ratios and the undecided
    share; asserts the bars and the 1 % cap."""
    M, F = _columns(g, fields, u)
    m = len(got.count)
    rel = np.broadcast_to(np.asarray(release), (m,))
    worst, wsum, wtime, steps, undecided = 0.0, 0.0, 0.0, 0, 0
    for r in range(m):
        pts, el = got.path(r)
        n = len(pts)
        if n < 2:
            continue
        tot, tbar, whole, rested, s = FR.LD(0), FR.LD(0), True, 0, None
        for k in range(n - 1):
            j, i = int(rel[r]) + k // substeps, k % substeps
            s = PR.step(F[j], F[j + 1], ts[j], ts[j + 1], substeps, i, pts[k].astype(FR.LD), int(el[k]), p, direction, speed, gmin)
            steps += 1
            if s.undecided and s.kind != "exit":
                undecided += 1
                whole = False
                continue
            who = "%s seed %d step %d" % (name, r, k)
            assert s.kind in ("step", "exit") and s.recorded, (who, s.kind)
            bar = s.exit_bar if s.kind == "exit" else s.bar
            if s.kind == "exit":
                assert k == n - 2 and got.status[r] == PR.EXIT, who
                gapt = abs(FR.LD(got.rows[r, 1]) - s.time)
                wtime = max(wtime, float(gapt / s.time_bar))
                assert gapt <= s.time_bar, (who, float(gapt), float(s.time_bar))
            else:
                assert s.e == el[k + 1], (who, s.e, el[k + 1])
                rested += int(not s.moved)
            gap = np.abs(pts[k + 1].astype(FR.LD) - s.x).max()
            worst = max(worst, float(gap / bar))
            assert gap <= bar, (who, float(gap), float(bar))
            tot, tbar = tot + s.dlength, tbar + s.lbar
        if whole and (got.status[r] != PR.EXIT or s.kind == "exit"):
            who = "%s seed %d" % (name, r)
            gap, sbar = abs(FR.LD(got.rows[r, 0]) - tot), tbar + n * FR.EPS * tot
            if sbar > 0:
                wsum = max(wsum, float(gap / sbar))
            assert gap <= sbar, (who, float(gap), float(sbar))
            assert got.rested[r] == rested, (who, got.rested[r], rested)
            j0 = int(rel[r])
            v0 = PR.blend(F[j0], F[j0 + 1], int(el[0]), pts[0].astype(FR.LD), 0)[0]
            assert abs(got.rows[r, 2] - v0) <= PR.value_bar(F[j0], F[j0 + 1], int(el[0]), pts[0].astype(FR.LD)), who
            if got.status[r] == PR.DONE:
                v1 = F[stop].value(int(el[-1]), pts[-1].astype(FR.LD))
                assert abs(got.rows[r, 3] - v1) <= F[stop].value_bar(int(el[-1]), pts[-1].astype(FR.LD)), who
                assert got.rows[r, 1] == ts[stop], who
            assert got.end[r].tobytes() == pts[-1].tobytes() and got.end_element[r] == el[-1], who
    share = undecided / max(steps, 1)
    print("%s: %d steps replayed, largest ratio to the bar: points %.3f, length %.3f, exit time %.3f; undecided %d (%.3f %%)"
          % (name, steps, worst, wsum, wtime, undecided, 100 * share))
    assert steps > 0 and share <= cap, (name, share)
    return worst, share


def same_as_host(name, dev, host):
    """Device Result against the host Result, bit for bit: everything discrete, the five row columns, the end points, the
    offsets, points and elements."""
    assert np.array_equal(dev.status, host.status), name
    assert np.array_equal(dev.count, host.count) and np.array_equal(dev.end_element, host.end_element), name
    assert np.array_equal(dev.rested, host.rested), name
    assert np.ascontiguousarray(dev.rows).tobytes() == np.ascontiguousarray(host.rows).tobytes(), name
    assert np.ascontiguousarray(dev.end).tobytes() == np.ascontiguousarray(host.end).tobytes(), name
    if host.offsets is not None and dev.offsets is not None:
        assert np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.elem, host.elem), name
        assert dev.pts.tobytes() == host.pts.tobytes(), name


def fields_2d(x, B):
    """B snapshots of a smooth field that turns in time: broken gradients across the elements, no critical point near the seeds"""
    return [(1.0 + 0.25 * j) * (np.sin(1.5 * x[:, 0] + 0.5 + 0.2 * j) * np.cos(1.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 1]) + 0.9 * x[:, 0]
            + 0.15 * j * x[:, 1] for j in range(B)]


def fields_3d(x, B):
    return [(1.0 + 0.25 * j) * (np.sin(1.3 * x[:, 0] + 0.5) * np.cos(1.1 * x[:, 1]) + 0.4 * x[:, 2] * x[:, 0]) + 0.8 * x[:, 2]
            + 0.15 * j * x[:, 1] for j in range(B)]
