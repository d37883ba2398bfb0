"""What test_isosurface_host.py and test_gpu_isosurfaces.py share: host fem3d geometries, the call of mgb_geo_isosurfaces_host
and the comparison of a library result with the numpy yardstick tests/isosurface_reference.py under its bars.  Not a test.
The sum bar KTOL and the maxima bar 8 eps (max|v| + |c|) are those of levelset_util.py."""
import ctypes as C

import numpy as np

import isosurface_reference as IR
from levelset_util import KTOL, MGB_E_ARG      # noqa: F401  (MGB_E_ARG: for the tests)


class HostMesh:
    """A host mgb_geo handle of fem3d level L, degree k, with n, nel, block and x."""

    def __init__(self, L, k):
        from mgb_amd import _lib
        h = C.c_void_p()
        _lib.call("mgb_fem3d_native", L, k, C.byref(h))
        self.handle, self.L, self.k = h, L, k
        n, dim, Lv, block = (C.c_int() for _ in range(4))
        _lib.call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(Lv), C.byref(block))
        self.n, self.dim, self.block = n.value, dim.value, block.value
        assert self.dim == 3 and self.block == (k + 1) ** 3
        self.nel = self.n // self.block
        self.x, self.w = np.empty((self.n, 3)), np.empty(self.n)
        _lib.call("mgb_geo_get_xw", h, _lib.dptr(self.x), _lib.dptr(self.w))

    def items(self, refine=0):
        return 6 * (self.k * 2 ** refine) ** 3 * self.nel


_HOST = {}


def host_mesh(L, k):
    if (L, k) not in _HOST:
        _HOST[(L, k)] = HostMesh(L, k)
    return _HOST[(L, k)]


class Result:
    """rows (B, nl, 5), counts (B, nl), offsets (B nl + 1), tri (total, 9), item (total,) of a library call."""

    def __init__(self, rows, counts, offsets, tri, item):
        self.rows, self.counts, self.offsets, self.tri, self.item = rows, counts, offsets, tri, item

    def row(self, b, l):
        r = b * self.counts.shape[1] + l
        a, e = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.tri[a:e], self.item[a:e]


def host_isosurfaces(lib, g, fields, levels, refine=0, u=0, rc_only=False, S=None, B=None, nl=None, triangles=True):
    """mgb_geo_isosurfaces_host on a HostMesh: `fields` a list of (n,) or (n, S) arrays.  Two calls: the counts, then the
    triangles in arrays of exactly that size.  Outputs are prefilled so that an unwritten word shows."""
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
    rc = lib.mgb_geo_isosurfaces_host(g.handle, B, table, S, u, nl, _lib.dptr(lv), refine, _lib.dptr(rows), ll(counts), None, None,
                                      None, 0)
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    if not triangles:
        return Result(rows, counts, None, None, None)
    total = int(counts.sum())
    offsets = np.full(B * nl + 1, -7, dtype=np.int64)
    tri, item = np.full((total, 9), 7.0), np.full(total, -7, dtype=np.int32)
    rows2, counts2 = np.full_like(rows, 7.0), np.full_like(counts, -7)
    rc = lib.mgb_geo_isosurfaces_host(g.handle, B, table, S, u, nl, _lib.dptr(lv), refine, _lib.dptr(rows2), ll(counts2), ll(offsets),
                                      _lib.dptr(tri), _lib.iptr(item), total)
    assert rc == 0, lib.mgb_last_error()
    assert rows2.tobytes() == rows.tobytes() and np.array_equal(counts2, counts)
    return Result(rows, counts, offsets, tri, item)


def device_result(iso):
    """The same Result from an Isosurfaces of the Python interface."""
    return Result(iso.rows, iso._counts, iso._offsets, iso._tri, iso._item)


_REF = {}


def reference(key, x, z, k, levels, refine):
    """The yardstick of one field, computed once per `key` (None: not kept) and shared among the tests; never changed."""
    if key is None:
        return IR.isosurfaces(x, z, k, levels, refine)
    key = (key, k, tuple(float(c) for c in levels), refine)
    if key not in _REF:
        _REF[key] = IR.isosurfaces(x, z, k, levels, refine)
    return _REF[key]


def against_reference(name, got, g, fields, levels, refine, u=0, keys=None):
    """A library Result against the yardstick, row by row: counts, items and offsets equal, every vertex inside its bar, the
    three sums within KTOL of the sum of the absolute terms, the maxima within 8 eps (max|v| + |c|).  Prints the largest ratio
    to each bar, then asserts.  For refine > 0 the classification margin of the yardstick must be 1e3 value bars."""
    levels = np.atleast_1d(levels)
    worst = {"vertex": 0.0, "sum": 0.0, "max": 0.0}
    at = 0
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(g.n, -1)
        ref = reference(None if keys is None else keys[b], g.x, z[:, u], g.k, levels, refine)
        for l, R in enumerate(ref):
            who = "%s field %d level %g" % (name, b, levels[l])
            if refine > 0:
                print("%s: classification margin %.3e, value bar %.3e" % (who, R.margin, R.value_bar))
                assert R.margin >= 1e3 * R.value_bar, who
            assert got.counts[b, l] == R.count, (who, got.counts[b, l], R.count)
            assert got.offsets[b * len(levels) + l] == at, who
            at += R.count
            tri, item = got.row(b, l)
            assert np.array_equal(item, R.items), who
            if R.count:
                gap = np.abs(tri.astype(IR.LD) - R.tri)
                ratio = gap / np.repeat(R.bar, 3, axis=1)
                worst["vertex"] = max(worst["vertex"], float(ratio.max()))
                assert (ratio <= 1.0).all(), (who, float(ratio.max()))
            rows = got.rows[b, l]
            if np.isnan(R.rows).any():
                assert np.isnan(R.rows).all() and np.isnan(rows).all(), who
                continue
            assert np.isfinite(rows).all(), who
            sbar = KTOL * R.abs_terms
            sgap = np.abs(rows[:3].astype(IR.LD) - R.rows[:3])
            mbar = 8 * IR.EPS * (R.vmax + abs(IR.LD(levels[l])))
            mgap = np.abs(rows[3:].astype(IR.LD) - R.rows[3:])
            for j in range(3):
                if sbar[j] > 0:
                    worst["sum"] = max(worst["sum"], float(sgap[j] / sbar[j]))
            worst["max"] = max(worst["max"], float((mgap / mbar).max()))
            assert (sgap <= sbar).all(), (who, sgap, sbar)
            assert (mgap <= mbar).all(), (who, mgap, mbar)
    assert got.offsets[-1] == at
    print("%s: largest ratio to the bar: vertices %.3f, sums %.3e, maxima %.3f" % (name, worst["vertex"], worst["sum"], worst["max"]))
    return worst


def same_as_host(name, dev, host, g, fields, levels, refine, u=0, keys=None):
    """Device Result against the host Result: everything discrete equal, vertices and maxima bit for bit, sums at KTOL."""
    assert np.array_equal(dev.counts, host.counts), name
    assert np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.item, host.item), name
    differ = int((dev.tri != host.tri).sum())
    print("%s: %d triangles, %d vertex coordinates differ from the host restatement" % (name, len(host.tri), differ))
    assert dev.tri.tobytes() == host.tri.tobytes(), name
    assert dev.rows[:, :, 3:].tobytes() == host.rows[:, :, 3:].tobytes(), name
    worst = 0.0
    levels = np.atleast_1d(levels)
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(g.n, -1)
        for l, R in enumerate(reference(None if keys is None else keys[b], g.x, z[:, u], g.k, levels, refine)):
            if np.isnan(R.rows).any():
                assert np.isnan(dev.rows[b, l]).all() and np.isnan(host.rows[b, l]).all()
                continue
            gap, bar = np.abs(dev.rows[b, l, :3] - host.rows[b, l, :3]), KTOL * R.abs_terms.astype(np.float64)
            worst = max([worst] + [q / s for q, s in zip(gap, bar) if s > 0])
            assert (gap <= bar).all(), (name, b, l, gap, bar)
    print("%s: sums against the host restatement, largest ratio to the bar %.3e" % (name, worst))
    return worst


def paraboloid(x):
    """The nodal values of u = x^2 + y^2 + z^2: the tensor interpolant of degree k >= 2 reproduces u."""
    return (x * x).sum(axis=1)


def gauss(tri):
    """1/6 sum det [P0, P1, P2] over the triangles (m, 9): the signed volume their closed surfaces enclose."""
    t = np.asarray(tri, dtype=IR.LD).reshape(-1, 3, 3)
    return float((np.cross(t[:, 0], t[:, 1]) * t[:, 2]).sum() / 6)


def edge_pairs(tri):
    """How often every directed edge of the triangles (m, 9) occurs, bit for bit (-0.0 taken as 0.0), and how often its
    reverse: two dicts keyed by the 48 bytes of the edge."""
    t = (np.asarray(tri, dtype=np.float64).reshape(-1, 3, 3) + 0.0)
    fwd, rev = {}, {}
    for a, b in ((0, 1), (1, 2), (2, 0)):
        for p, q in zip(t[:, a], t[:, b]):
            kf, kr = p.tobytes() + q.tobytes(), q.tobytes() + p.tobytes()
            fwd[kf] = fwd.get(kf, 0) + 1
            rev[kr] = rev.get(kr, 0) + 1
    return fwd, rev
