#!/usr/bin/env python3
"""Time isosurfaces() (csrc/isosurface.hip) on fem3d solutions, next to energy() on the same fields.  GPU only.
usage: python3 tools/isosurface_bench.py [L=4] [k=3] [refine=0] [nl=4] [reps=50] [--out FILE]

Solves fem3d at L, k (p = 1), takes nl levels evenly inside the range of u, then times, in this order and in the same run,
  isosurfaces, measure only     mgb_geo_isosurfaces without triangles: two launches, one copy, one wait
  isosurfaces, with triangles   ... plus the emit launch, its wait, and the copy of the triangles to the host
  energy                        mgb_geo_field_energy on the same fields: two launches, one copy, one wait
on the solution (B = 1) and on a batch of 16 distinct fields (the solution and 15 perturbed copies, separate allocations, as
the snapshots of a parabolic run are).  The host clock around `reps` calls measures what a user pays per call.
Compulsory bytes: isosurfaces read the u column of z (8 per node and field; its S columns lie in the same cache lines, so
8 S per node is what moves) and, at refine = 0, x (24 per node; at refine > 0 the two box corners of an element only, counted
the same) and write 48 bytes per workgroup and row plus 76 per triangle; energy reads x, w, f and z.  Item arithmetic is
redone for every level and, with triangles, once more in the emit launch."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import mgb_amd as M         # noqa: E402
from mgb_amd import _lib    # noqa: E402

P = 1.0
BATCH = 16


def timed(fn, reps, backend):
    for _ in range(5):
        fn()
    backend.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    backend.synchronize()
    return (time.perf_counter() - t0) / reps


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 4
    k = int(argv[1]) if len(argv) > 1 else 3
    refine = int(argv[2]) if len(argv) > 2 else 0
    nl = max(1, int(argv[3])) if len(argv) > 3 else 4
    reps = max(10, int(argv[4])) if len(argv) > 4 else 50
    if M.device_count() <= 0:
        raise SystemExit("isosurface_bench: no HIP device visible")
    sol = M.fem3d_mpi_solve(L=L, k=k, p=P)
    loc, backend = M._locator_of(sol.geometry)
    n, S = sol.z.shape
    rng = np.random.default_rng(0)
    z0 = sol.z.to_numpy()
    u0 = z0[:, 0]
    levels = np.ascontiguousarray(u0.min() + (u0.max() - u0.min()) * (np.arange(nl) + 1.0) / (nl + 1.0))
    fields = [sol.z] + [M.HPCMatrix(z0 * (1.0 + 1e-3 * rng.standard_normal(z0.shape)), backend) for _ in range(BATCH - 1)]
    f = M.HPCVector(np.full(n, 0.5), backend)
    items = 6 * (k * 2 ** refine) ** 3 * (n // (k + 1) ** 3)
    nwg = (items + 255) // 256
    lines = ["isosurface_bench: fem3d L=%d k=%d  n=%d  S=%d  nl=%d  refine=%d  items per row=%d  workgroups per row=%d  reps=%d"
             % (L, k, n, S, nl, refine, items, nwg, reps)]
    lp = _lib.dptr(levels)
    for B in (1, BATCH):
        table = (C.c_void_p * B)(*[zk._v.handle.value for zk in fields[:B]])
        rows, counts, eout = np.empty((B, nl, 5)), np.empty((B, nl), dtype=np.int64), np.empty((B, 5))
        cp = counts.ctypes.data_as(_lib.c_ll_p)

        def measure():
            _lib.call("mgb_geo_isosurfaces", loc, B, table, S, 0, nl, lp, refine, _lib.dptr(rows), cp, None)

        measure()
        total = int(counts.sum())
        offsets, tri, item = np.empty(B * nl + 1, dtype=np.int64), np.empty((total, 9)), np.empty(total, dtype=np.int32)

        def with_triangles():
            h = C.c_void_p()
            _lib.call("mgb_geo_isosurfaces", loc, B, table, S, 0, nl, lp, refine, _lib.dptr(rows), cp, C.byref(h))
            _lib.call("mgb_levelset_get", h, offsets.ctypes.data_as(_lib.c_ll_p), _lib.dptr(tri), _lib.iptr(item))
            _lib.call("mgb_levelset_destroy", h)

        def energy():
            _lib.call("mgb_geo_field_energy", loc, B, table, S, 0, S - 1, P, None, f.handle, 1, _lib.dptr(eout))

        read = n * 24 + B * n * 8 * S
        wrote = B * nl * nwg * 48
        cases = (("isosurfaces, measure only", measure, read + wrote),
                 ("isosurfaces, with triangles", with_triangles, 2 * read + wrote + total * 76),
                 ("energy", energy, n * (24 + 8 + 8) + B * n * 8 * S))
        times = {}
        for name, fn, nbytes in cases:
            dt = times[name] = timed(fn, reps, backend)
            lines.append("B=%-3d %-28s %9.2f us per call   %8.3f MB compulsory   %6.3f TB/s"
                         % (B, name, 1e6 * dt, nbytes / 1e6, nbytes / dt / 1e12))
        tm, tt, te = (times[c[0]] for c in cases)
        lines.append("B=%-3d %d rows, %d triangles: measure only %.2f x energy, with triangles %.2f x energy; %.3f ns per item and row"
                     % (B, B * nl, total, tm / te, tt / te, 1e9 * tm / (B * nl * items)))
    iso = M.isosurfaces(sol, levels, refine=refine)
    lines.append("solution: levels %s" % np.array2string(levels, precision=6))
    lines.append("          above %s  area %s  count %s" % (np.array2string(np.atleast_1d(iso.above), precision=9),
                                                            np.array2string(np.atleast_1d(iso.area), precision=9), iso.count))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
