"""What test_section_reference.py, test_section_host.py and test_gpu_sections.py share: host geometries, the call of
mgb_geo_sections_host and the comparison of a library result with the numpy yardstick tests/section_reference.py under its
bars.  Not a test.  The sum bar KTOL is that of levelset_util.py; the vertex, value and maxima bars are section_reference.py's."""
import numpy as np

import isosurface_util as IU
import levelset_util as LU
import section_reference as SR
from levelset_util import KTOL, MGB_E_ARG      # noqa: F401  (MGB_E_ARG: for the tests)

# axis-aligned, tilted, on element faces, on the faces of the Kuhn tetrahedra, x = -1 with nothing above, x = 1, outside
PLANES3 = [[0.0, 0.0, 1.0, 0.3], [1.0, 0.5, 0.25, 0.05], [1.0, 0.0, 0.0, 0.0], [1.0, -1.0, 0.0, 0.0], [-2.0, 0.0, 0.0, 2.0],
           [1.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0]]      # axis, tilted, faces, Kuhn faces, x = -1 (above: x < -1), x = 1, outside
PLANES2 = [[1.0, 0.0, 0.3], [1.0, 0.5, 0.05], [1.0, 0.0, 0.0], [1.0, -1.0, 0.0], [-2.0, 0.0, 2.0], [1.0, 0.0, 1.0], [0.0, 1.0, 3.0]]


def smooth(x):
    """A field without symmetry, continuous across the elements."""
    if x.shape[1] == 2:
        return np.sin(3.0 * x[:, 0] + 0.5) * np.cos(2.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 1] + 0.2 * x[:, 1]
    return np.sin(3.0 * x[:, 0] + 0.5) * np.cos(2.0 * x[:, 1]) + 0.3 * x[:, 0] * x[:, 2] + 0.2 * x[:, 2]


def host_mesh(dim, L, k=0):
    """fem2d level L, or fem3d level L of degree k, with n, nel, dim, block, x and k (0 in 2-D)."""
    g = LU.host_mesh("fem2d", L) if dim == 2 else IU.host_mesh(L, k)
    g.k = k if dim == 3 else 0
    return g


def items_per_row(g):
    return g.nel * (6 if g.dim == 3 else 1)


class Result:
    """rows (B, nc, 5), counts (B, nc), offsets (B nc + 1), piece (total, 6 or 12), item (total,) of a library call."""

    def __init__(self, rows, counts, offsets, piece, item):
        self.rows, self.counts, self.offsets, self.piece, self.item = rows, counts, offsets, piece, item

    def row(self, b, l):
        r = b * self.counts.shape[1] + l
        a, e = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.piece[a:e], self.item[a:e]


def host_sections(lib, g, fields, planes, p=2.0, u=0, rc_only=False, S=None, B=None, nc=None, pieces=True):
    """mgb_geo_sections_host on a host mesh: `fields` a list of (n,) or (n, S) arrays.  Two calls: the counts, then the pieces
    in arrays of exactly that size.  Outputs are prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    fields = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    pl = _lib.f64(np.asarray(planes, dtype=np.float64).reshape(-1, g.dim + 1))
    nc = pl.shape[0] if nc is None else nc
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    shape = (max(B, 1), max(nc, 1)) if B * nc <= 1 << 20 else (1, 1)      # a refused call writes nothing
    rows = np.full(shape + (5,), 7.0)
    counts = np.full(shape, -7, dtype=np.int64)
    ll = lambda a: None if a is None else a.ctypes.data_as(_lib.c_ll_p)
    rc = lib.mgb_geo_sections_host(g.handle, B, table, S, u, nc, _lib.dptr(pl), p, _lib.dptr(rows), ll(counts), None, None, None, 0)
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    if not pieces:
        return Result(rows, counts, None, None, None)
    total = int(counts.sum())
    offsets = np.full(B * nc + 1, -7, dtype=np.int64)
    piece, item = np.full((total, 6 if g.dim == 2 else 12), 7.0), np.full(total, -7, dtype=np.int32)
    rows2, counts2 = np.full_like(rows, 7.0), np.full_like(counts, -7)
    rc = lib.mgb_geo_sections_host(g.handle, B, table, S, u, nc, _lib.dptr(pl), p, _lib.dptr(rows2), ll(counts2), ll(offsets),
                                   _lib.dptr(piece), _lib.iptr(item), total)
    assert rc == 0, lib.mgb_last_error()
    assert rows2.tobytes() == rows.tobytes() and np.array_equal(counts2, counts)
    return Result(rows, counts, offsets, piece, item)


def device_result(sec):
    """The same Result from a Sections of the Python interface."""
    return Result(sec.rows, sec._counts, sec._offsets, sec._piece, sec._item)


_REF = {}


def reference(key, g, z, planes, p):
    """The yardstick of one field, computed once per `key` (None: not kept) and shared among the tests; never changed."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, g.dim + 1)
    if key is None:
        return SR.sections(g.x, z, g.dim, g.k, planes, p)
    key = (key, g.dim, g.L, g.k, planes.tobytes(), float(p))
    if key not in _REF:
        _REF[key] = SR.sections(g.x, z, g.dim, g.k, planes, p)
    return _REF[key]


def against_reference(name, got, g, fields, planes, p=2.0, u=0, keys=None):
    """A library Result against the yardstick, row by row: counts, items and offsets equal, every vertex and vertex value
    inside its bar, the three sums within KTOL of the sum of the absolute terms, both maxima inside the value bar.  Prints the
    largest ratio to each bar, then asserts."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, g.dim + 1)
    nv = g.dim
    worst = {"vertex": 0.0, "value": 0.0, "sum": 0.0, "max": 0.0}
    at = 0
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(g.n, -1)
        ref = reference(None if keys is None else keys[b], g, z[:, u], planes, p)
        for l, R in enumerate(ref):
            who = "%s field %d plane %d" % (name, b, l)
            assert got.counts[b, l] == R.count, (who, got.counts[b, l], R.count)
            assert got.offsets[b * len(planes) + l] == at, who
            at += R.count
            piece, item = got.row(b, l)
            assert np.array_equal(item, R.items), who
            if R.count:
                gap = np.abs(piece.astype(SR.LD) - R.piece)
                ratio = gap[:, :nv * nv] / np.repeat(R.bar, nv, axis=1)
                worst["vertex"] = max(worst["vertex"], float(ratio.max()))
                assert (ratio <= 1.0).all(), (who, float(ratio.max()))
                vratio = gap[:, nv * nv:] / R.vbar
                worst["value"] = max(worst["value"], float(vratio.max()))
                assert (vratio <= 1.0).all(), (who, float(vratio.max()))
            rows = got.rows[b, l]
            if np.isnan(R.rows).any():
                assert np.isnan(R.rows).all() and np.isnan(rows).all(), who
                continue
            if R.count == 0:
                assert np.array_equal(rows, [0.0, 0.0, 0.0, -np.inf, -np.inf]), (who, rows)
                continue
            assert np.isfinite(rows).all(), who
            sbar = KTOL * R.abs_terms
            sgap = np.abs(rows[:3].astype(SR.LD) - R.rows[:3])
            mgap = np.abs(rows[3:].astype(SR.LD) - R.rows[3:])
            for j in range(3):
                if sbar[j] > 0:
                    worst["sum"] = max(worst["sum"], float(sgap[j] / sbar[j]))
            worst["max"] = max(worst["max"], float((mgap / R.mbar).max()))
            assert (sgap <= sbar).all(), (who, sgap, sbar)
            assert (mgap <= R.mbar).all(), (who, mgap, R.mbar)
    assert got.offsets[-1] == at
    print("%s: largest ratio to the bar: vertices %.3f, vertex values %.3f, sums %.3e, maxima %.3f"
          % (name, worst["vertex"], worst["value"], worst["sum"], worst["max"]))
    return worst


def same_as_host(name, dev, host, g, fields, planes, p=2.0, u=0, keys=None):
    """Device Result against the host Result: everything discrete equal, vertices, vertex values and maxima bit for bit, the
    three sums at KTOL of their absolute terms (the flow rate with pow for p other than 1 and 2 has no other bar)."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, g.dim + 1)
    assert np.array_equal(dev.counts, host.counts), name
    assert np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.item, host.item), name
    differ = int((dev.piece != host.piece).sum())
    print("%s: %d pieces, %d doubles of them differ from the host restatement" % (name, len(host.piece), differ))
    assert dev.piece.tobytes() == host.piece.tobytes(), name
    assert dev.rows[:, :, 3:].tobytes() == host.rows[:, :, 3:].tobytes(), name
    worst = 0.0
    for b, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(g.n, -1)
        for l, R in enumerate(reference(None if keys is None else keys[b], g, z[:, u], planes, p)):
            if np.isnan(R.rows).any():
                assert np.isnan(dev.rows[b, l]).all() and np.isnan(host.rows[b, l]).all()
                continue
            gap, bar = np.abs(dev.rows[b, l, :3] - host.rows[b, l, :3]), KTOL * R.abs_terms.astype(np.float64)
            worst = max([worst] + [q / s for q, s in zip(gap, bar) if s > 0])
            assert (gap <= bar).all(), (name, b, l, gap, bar)
    print("%s: sums against the host restatement, largest ratio to the bar %.3e" % (name, worst))
    return worst


def piece_measure(piece, dim):
    """The lengths or areas of the pieces (m, 6 or 12)."""
    V = np.asarray(piece, dtype=SR.LD)[:, :dim * dim].reshape(-1, dim, dim)
    if dim == 2:
        return np.sqrt(((V[:, 1] - V[:, 0]) ** 2).sum(axis=1))
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    return np.sqrt((n * n).sum(axis=1)) / 2
