"""What test_ray_reference.py, test_ray_host.py and test_gpu_line_integrals.py share: host geometries, the ray sets, the call
of mgb_geo_line_integrals_host and the comparison of a library result with the numpy yardstick tests/ray_reference.py under
its bars.  Not a test."""
import numpy as np

import levelset_util as LU
import mesh_cases as MC
import ray_reference as RR
import section_util as SU
from levelset_util import MGB_E_ARG      # noqa: F401  (for the tests)

smooth = SU.smooth
COLS = ("length", "integral", "along", "across", "max", "min", "enter", "leave")
_LSHAPE = {}


def host_mesh(kind, L, k=0):
    """kind "fem2d", "lshape" or "fem3d": a host mesh with handle, n, nel, dim, block, x, k (0 in 2-D), L and name."""
    if kind == "lshape":
        if L not in _LSHAPE:
            _LSHAPE[L] = LU.HostMesh("fem2d", L, MC.LSHAPE)
        g = _LSHAPE[L]
        g.k = 0
    else:
        g = SU.host_mesh(2 if kind == "fem2d" else 3, L, k)
    g.name = "%s L=%d k=%d" % (kind, L, g.k)
    return g


MESHES = [("fem2d", 1, 0), ("fem2d", 4, 0), ("lshape", 2, 0), ("fem3d", 1, 1), ("fem3d", 2, 3), ("fem3d", 3, 2)]


def degenerate(dim):
    """The named degenerate segments (a, b) on meshes of [-1, 1]^dim whose lines include the coordinate planes: in a face, in a
    boundary face, along an edge, along a boundary edge, 1e-13 either side of a face, at slope 1e-11 against a face, the
    vertex-to-vertex diagonals, inside one element of the finest meshes used, and outside."""
    if dim == 2:
        segs = [((-1.2, 0.0), (1.2, 0.0)), ((-0.9, 1.0), (0.8, 1.0)), ((0.0, -1.0), (0.0, 1.0)), ((-1.0, -0.7), (-1.0, 0.9)),
                ((-0.8, 1e-13), (0.9, 1e-13)), ((-0.8, -1e-13), (0.9, -1e-13)), ((-0.9, 0.0), (0.9, 1.8e-11)),
                ((-1.0, -1.0), (1.0, 1.0)), ((-1.0, 1.0), (1.0, -1.0)), ((0.10, 0.02), (0.20, 0.04)), ((1.5, 1.5), (2.0, 3.0)),
                ((-2.0, 1.5), (2.0, 1.5))]
    else:
        segs = [((-1.2, 0.3, 0.0), (1.2, 0.4, 0.0)), ((-0.9, 0.2, 1.0), (0.8, -0.3, 1.0)), ((-1.1, 0.0, 0.0), (1.1, 0.0, 0.0)),
                ((-1.0, -1.0, -0.7), (-1.0, -1.0, 0.9)), ((-0.8, 0.1, 1e-13), (0.9, 0.2, 1e-13)), ((-0.8, 0.1, -1e-13), (0.9, 0.2, -1e-13)),
                ((-0.9, 0.1, 0.0), (0.9, 0.3, 1.8e-11)), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), ((-1.0, 1.0, -1.0), (1.0, -1.0, 1.0)),
                ((0.10, 0.02, 0.07), (0.20, 0.04, 0.21)), ((1.5, 1.5, 0.0), (2.0, 3.0, 0.5)), ((-2.0, 1.5, 0.2), (2.0, 1.5, 0.3))]
    s = np.array(segs, dtype=np.float64)
    return s[:, 0].copy(), s[:, 1].copy()


N_DEGENERATE = 12


def rays(dim, m, seed=7):
    """m segments: the degenerate ones first (as many as fit), then seeded random ones -- chords across [-1.3, 1.3]^dim, one
    in eight wholly outside."""
    a, b = degenerate(dim)
    rng = np.random.default_rng(seed + dim)
    ra, rb = rng.uniform(-1.3, 1.3, (max(m, 1), dim)), rng.uniform(-1.3, 1.3, (max(m, 1), dim))
    out = np.arange(max(m, 1)) % 8 == 5
    ra[out, 0] += 3.0
    rb[out, 0] += 3.0
    a, b = np.concatenate([a, ra])[:m], np.concatenate([b, rb])[:m]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


class Result:
    """rows (B, m, 8), count (B, m), offsets (B m + 1), piece (total, 3), elem (total,) of a library call."""

    def __init__(self, rows, count, offsets, piece, elem):
        self.rows, self.count, self.offsets, self.piece, self.elem = rows, count, offsets, piece, elem

    def row(self, b, i):
        r = b * self.count.shape[1] + i
        s, e = int(self.offsets[r]), int(self.offsets[r + 1])
        return self.elem[s:e], self.piece[s:e]


def host_line_integrals(lib, g, fields, a, b, p=2.0, u=0, rc_only=False, S=None, B=None, m=None, pieces=True):
    """mgb_geo_line_integrals_host on a host mesh: `fields` a list of (n,) or (n, S) arrays.  Two calls: the counts, then the
    pieces in arrays of exactly that size.  Outputs are prefilled so that an unwritten word shows."""
    from mgb_amd import _lib
    fields = [_lib.f64(z).reshape(g.n, -1) for z in fields]
    S = fields[0].shape[1] if S is None else S
    B = len(fields) if B is None else B
    a, b = (_lib.f64(np.asarray(v, dtype=np.float64).reshape(-1, g.dim)) for v in (a, b))
    m = a.shape[0] if m is None else m
    table = (_lib.c_dbl_p * max(len(fields), 1))(*[_lib.dptr(z) for z in fields])
    shape = (max(B, 1), max(m, 1)) if 0 <= B * m <= 1 << 20 else (1, 1)      # a refused call writes nothing
    rows, count = np.full(shape + (8,), 7.0), np.full(shape, -7, dtype=np.int32)
    rc = lib.mgb_geo_line_integrals_host(g.handle, B, table, S, u, m, _lib.dptr(a), _lib.dptr(b), p, _lib.dptr(rows), _lib.iptr(count),
                                         None, None, None, 0)
    if rc_only:
        return rc
    assert rc == 0, lib.mgb_last_error()
    if not pieces:
        return Result(rows, count, None, None, None)
    total = int(count.sum()) if m else 0
    offsets = np.full(B * m + 1, -7, dtype=np.int64)
    piece, elem = np.full((total, 3), 7.0), np.full(total, -7, dtype=np.int32)
    rows2, count2 = np.full_like(rows, 7.0), np.full_like(count, -7)
    rc = lib.mgb_geo_line_integrals_host(g.handle, B, table, S, u, m, _lib.dptr(a), _lib.dptr(b), p, _lib.dptr(rows2), _lib.iptr(count2),
                                         offsets.ctypes.data_as(_lib.c_ll_p), _lib.dptr(piece), _lib.iptr(elem), total)
    assert rc == 0, lib.mgb_last_error()
    assert rows2.tobytes() == rows.tobytes() and np.array_equal(count2, count)
    return Result(rows, count, offsets, piece, elem)


def device_result(res):
    """The same Result from a LineIntegrals of the Python interface."""
    return Result(res.rows, res._count, res._offsets, res._piece, res._elem)


def reference(g, z, a, b, p=2.0):
    """The yardstick of one field; its geometric part is computed once per mesh and ray set and shared among the tests."""
    return RR.line_integrals(g.x, z, g.dim, g.k, a, b, p, key=g.name)


def against_reference(name, got, g, fields, a, b, p=2.0, u=0, named=N_DEGENERATE):
    """A library Result against the yardstick, row by row: counts and the sets of piece elements equal, every piece end and
    piece integral and all eight columns inside their bars.  A ray with an undecided decision is left out: at most 1 % of the
    rays, and none of the first `named`.  Prints the largest ratio to each bar and the number left out, then asserts."""
    worst = {c: 0.0 for c in COLS + ("t0", "t1", "piece")}
    m = len(a)
    left_out = 0
    for bi, z in enumerate(fields):
        z = np.asarray(z, dtype=np.float64).reshape(g.n, -1)
        ref = reference(g, z[:, u], a, b, p)
        for i, R in enumerate(ref):
            who = "%s field %d ray %d" % (name, bi, i)
            if R.undecided:
                assert i >= named, who + ": a named degenerate ray is undecided"
                left_out += bi == 0
                continue
            assert got.count[bi, i] == R.count, (who, got.count[bi, i], R.count)
            rows = got.rows[bi, i]
            if got.offsets is not None:
                elem, piece = got.row(bi, i)
                order = np.argsort(elem, kind="stable")
                want = np.argsort(R.elements, kind="stable")
                assert np.array_equal(elem[order], R.elements[want]), (who, elem, R.elements)
                if R.count and not R.poisoned:
                    for c, (ref_v, bar) in enumerate(((R.t0, R.dt0), (R.t1, R.dt1), (R.integral, R.ibar))):
                        gap = np.abs(piece[order, c].astype(RR.LD) - ref_v[want])
                        tiny = np.maximum(bar[want], np.finfo(np.float64).tiny)
                        worst[("t0", "t1", "piece")[c]] = max(worst[("t0", "t1", "piece")[c]], float((gap / tiny).max()))
                        assert (gap <= bar[want]).all(), (who, c, gap, bar[want])
            if R.count == 0:
                assert np.array_equal(rows[:6], [0.0, 0.0, 0.0, 0.0, -np.inf, np.inf]) and np.isnan(rows[6:]).all(), (who, rows)
                continue
            cols = range(8)
            if R.poisoned:
                assert np.isnan(rows[1:6]).all(), (who, rows)
                cols = (0, 6, 7)
            for c in cols:
                gap = abs(RR.LD(rows[c]) - R.rows[c])
                assert gap <= R.bars[c], (who, COLS[c], rows[c], R.rows[c], gap, R.bars[c])
                if R.bars[c] > 0:
                    worst[COLS[c]] = max(worst[COLS[c]], float(gap / R.bars[c]))
    assert left_out <= 0.01 * m, (name, left_out, m)
    print("%s: %d of %d rays undecided; largest ratio to the bar: %s"
          % (name, left_out, m, ", ".join("%s %.3f" % (c, v) for c, v in worst.items())))
    assert max(worst.values()) <= 0.5, (name, worst)
    return worst, left_out


def same_as_host(name, dev, host, g, fields, a, b, p=2.0, u=0):
    """Device Result against the host Result: counts, offsets and piece elements equal; t0, t1, the piece integrals and all
    eight columns bit for bit, except along / across at an exponent other than 1 and 2: there within 4 eps sum |terms|, the
    terms those of the yardstick."""
    assert np.array_equal(dev.count, host.count), name
    if host.offsets is not None:
        assert np.array_equal(dev.offsets, host.offsets) and np.array_equal(dev.elem, host.elem), name
        assert dev.piece.tobytes() == host.piece.tobytes(), name
    exact = [0, 1, 4, 5, 6, 7] if p not in (1.0, 2.0) else list(range(8))
    assert dev.rows[:, :, exact].tobytes() == host.rows[:, :, exact].tobytes(), name
    worst = 0.0
    if p not in (1.0, 2.0):
        eps = np.finfo(np.float64).eps
        for bi, z in enumerate(fields):
            z = np.asarray(z, dtype=np.float64).reshape(g.n, -1)
            for i, R in enumerate(reference(g, z[:, u], a, b, p)):
                for c in (2, 3):
                    d, h = dev.rows[bi, i, c], host.rows[bi, i, c]
                    if np.isnan(h) or R.undecided:
                        assert np.isnan(d) == np.isnan(h), (name, bi, i)
                        continue
                    bar = 4 * eps * float(R.abs_terms[c])
                    assert abs(d - h) <= bar, (name, bi, i, COLS[c], d, h, bar)
                    if bar > 0:
                        worst = max(worst, abs(d - h) / bar)
        print("%s: along / across against the host restatement, largest ratio to the pow bar %.3f" % (name, worst))
    return worst
