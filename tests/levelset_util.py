"""What test_levelset_host.py and test_gpu_level_sets.py share: host geometries, the call of mgb_geo_level_sets_host and the
comparison of a library result with the numpy yardstick tests/levelset_reference.py under its bars.  Not a test."""
import ctypes as C

import numpy as np

import levelset_reference as LR

MGB_E_ARG = -1
KTOL = 1e-12
# one CCW and one CW triangle: the elements of the second have a negative determinant
K_MIXED = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])


class HostMesh:
    """A host mgb_geo handle of fem1d / fem2d level L (K: coarse triangles) with n, dim, block and x."""

    def __init__(self, kind, L, K=None):
        from mgb_amd import _lib
        h = C.c_void_p()
        if kind == "fem1d":
            _lib.call("mgb_fem1d_native", L, C.byref(h))
        else:
            Ka = None if K is None else _lib.f64(K)
            _lib.call("mgb_fem2d_native", L, _lib.dptr(Ka), 0 if K is None else Ka.shape[0], C.byref(h))
        self.handle, self.kind, self.L = h, kind, L
        n, dim, Lv, block = (C.c_int() for _ in range(4))
        _lib.call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(Lv), C.byref(block))
        self.n, self.dim, self.block = n.value, dim.value, block.value
        self.nel = self.n // self.block
        self.x, self.w = np.empty((self.n, self.dim)), np.empty(self.n)
        _lib.call("mgb_geo_get_xw", h, _lib.dptr(self.x), _lib.dptr(self.w))

    def close(self):
        from mgb_amd import _lib
        if self.handle is not None:
            _lib.call("mgb_geo_destroy", self.handle)
            self.handle = None


_HOST = {}


def host_mesh(kind, L, mixed=False):
    key = (kind, L, mixed)
    if key not in _HOST:
        _HOST[key] = HostMesh(kind, L, K_MIXED if mixed else None)
    return _HOST[key]


class Result:
    """rows (B, nl, 5), counts (B, nl), offsets (B nl + 1), seg (total, 4 or 2), item (total,) of a library call."""

    def __init__(self, rows, counts, offsets, seg, item):
        self.rows, self.counts, self.offsets, self.seg, self.item = rows, counts, offsets, seg, item

    def row(self, b, l):
        r = b * self.counts.shape[1] + l
        a, e = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.seg[a:e], self.item[a:e]


def host_level_sets(lib, g, fields, levels, refine=0, u=0, rc_only=False, S=None, B=None, nl=None, segments=True):
    """mgb_geo_level_sets_host on a HostMesh: `fields` a list of (n,) or (n, S) arrays.  Two calls: the counts, then the
    segments in arrays of exactly that size.  Outputs are prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    fields = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    lv = _lib.f64(np.atleast_1d(levels))
    nl = lv.size if nl is None else nl
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    rows = np.full((max(B, 1), max(nl, 1), 5), 7.0)
    counts = np.full((max(B, 1), max(nl, 1)), -7, dtype=np.int64)
    ll = lambda a: None if a is None else a.ctypes.data_as(_lib.c_ll_p)
    rc = lib.mgb_geo_level_sets_host(g.handle, B, table, S, u, nl, _lib.dptr(lv), refine, _lib.dptr(rows), ll(counts), None, None,
                                     None, 0)
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    if not segments:
        return Result(rows, counts, None, None, None)
    total = int(counts.sum())
    offsets = np.full(B * nl + 1, -7, dtype=np.int64)
    seg, item = np.full((total, 4 if g.dim == 2 else 2), 7.0), np.full(total, -7, dtype=np.int32)
    rows2, counts2 = np.full_like(rows, 7.0), np.full_like(counts, -7)
    rc = lib.mgb_geo_level_sets_host(g.handle, B, table, S, u, nl, _lib.dptr(lv), refine, _lib.dptr(rows2), ll(counts2), ll(offsets),
                                     _lib.dptr(seg), _lib.iptr(item), total)
    assert rc == 0, lib.mgb_last_error()
    assert rows2.tobytes() == rows.tobytes() and np.array_equal(counts2, counts)
    return Result(rows, counts, offsets, seg, item)


def device_result(ls, B, nl):
    """The same Result from a LevelSets of the Python interface."""
    return Result(ls.rows, ls._counts, ls._offsets, ls._seg, ls._item)


def against_reference(name, got, x, fields, levels, refine, u=0, need_margin=True):
    """A library Result against the yardstick, row by row: counts, items and offsets equal, every endpoint inside its bar, the
    three sums within KTOL of the sum of the absolute terms, the maxima within 8 eps (max|v| + |c|).  Prints the largest ratio
    to each bar, then asserts.  For refine > 0 the classification margin of the yardstick must be 1e3 value bars."""
    levels = np.atleast_1d(levels)
    worst = {"endpoint": 0.0, "sum": 0.0, "max": 0.0}
    at = 0
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(x.shape[0], -1)
        ref = LR.level_sets(x, z[:, u], levels, refine)
        for l, R in enumerate(ref):
            who = "%s field %d level %g" % (name, b, levels[l])
            if refine > 0 and need_margin:
                print("%s: classification margin %.3e, value bar %.3e" % (who, R.margin, R.value_bar))
                assert R.margin >= 1e3 * R.value_bar, who
            assert got.counts[b, l] == R.count, (who, got.counts[b, l], R.count)
            assert got.offsets[b * len(levels) + l] == at, who
            at += R.count
            seg, item = got.row(b, l)
            assert np.array_equal(item, R.items), who
            if R.count:
                gap = np.abs(seg.astype(LR.LD) - R.seg)
                if x.shape[1] == 2:
                    ratio = gap / np.repeat(R.bar, 2, axis=1)
                else:      # the direction is exact
                    assert np.array_equal(seg[:, 1], R.seg[:, 1].astype(np.float64)), who
                    ratio = gap[:, 0] / R.bar
                worst["endpoint"] = max(worst["endpoint"], float(ratio.max()))
                assert (ratio <= 1.0).all(), (who, float(ratio.max()))
            rows = got.rows[b, l]
            if np.isnan(R.rows).any():
                assert np.isnan(R.rows).all() and np.isnan(rows).all(), who
                continue
            assert np.isfinite(rows).all(), who
            sbar = KTOL * R.abs_terms
            sgap = np.abs(rows[:3].astype(LR.LD) - R.rows[:3])
            mbar = 8 * LR.EPS * (R.vmax + abs(LR.LD(levels[l])))
            mgap = np.abs(rows[3:].astype(LR.LD) - R.rows[3:])
            for k in range(3):
                if sbar[k] > 0:
                    worst["sum"] = max(worst["sum"], float(sgap[k] / sbar[k]))
            worst["max"] = max(worst["max"], float((mgap / mbar).max()))
            assert (sgap <= sbar).all(), (who, sgap, sbar)
            assert (mgap <= mbar).all(), (who, mgap, mbar)
    assert got.offsets[-1] == at
    print("%s: largest ratio to the bar: endpoints %.3f, sums %.3e, maxima %.3f" % (name, worst["endpoint"], worst["sum"], worst["max"]))
    return worst


def paraboloid(x):
    """The nodal values of u = x^2 + y^2: the P2 + bubble interpolant reproduces u."""
    return (x * x).sum(axis=1)


def green(seg):
    """1/2 sum (x0 y1 - x1 y0) over the segments: the signed area their loops enclose."""
    return 0.5 * float(np.sum(seg[:, 0] * seg[:, 3] - seg[:, 2] * seg[:, 1]))
