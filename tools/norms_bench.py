#!/usr/bin/env python3
"""Time norms() and a two-mesh error() (csrc/norms.hip) on fem2d solutions.  GPU only.
usage: python3 tools/norms_bench.py [L=7] [reps=50] [--out FILE]

Solves fem2d at L and L - 1 (p = 1), then times mgb_field_norms on the level-L solution (no reference) and on the level-L
solution against the level-(L-1) one (the quadrature on the finer mesh, the coarser field evaluated by its own polynomials).
Every call is two launches, a copy of S x 5 doubles to the host and a wait, so the host clock around `reps` calls measures what
a user of norms() pays per call.  Bytes/s from the compulsory traffic per node: x (8 dim), w (8) and z (8 S); across meshes the
coarse field and the bins are shared by neighbouring nodes and stay in cache.  Share of HBM peak (8.0 TB/s spec): bandwidth
is the bound by construction (about 100 flop per 40 compulsory bytes in 2-D)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import mgb_amd as M         # noqa: E402
from mgb_amd import _lib    # noqa: E402

HBM_PEAK = 8.0e12


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 7
    reps = max(10, int(argv[1])) if len(argv) > 1 else 50
    if M.device_count() <= 0:
        raise SystemExit("norms_bench: no HIP device visible")
    fine, coarse = M.fem2d_mpi_solve(L=L, p=1.0), M.fem2d_mpi_solve(L=L - 1, p=1.0)
    loc, backend = M._locator_of(fine.geometry)
    loc_c, _ = M._locator_of(coarse.geometry)
    n, S = fine.z.shape
    dim = 2
    nbytes = n * (8 * dim + 8 + 8 * S)
    sums = np.empty((S, 5))
    outside = C.c_longlong(0)
    lines = ["norms_bench: fem2d L=%d  n=%d  S=%d  against L=%d (n=%d)  reps=%d" % (L, n, S, L - 1, coarse.z.shape[0], reps)]
    for name, other, zo in (("norms", None, None), ("error, two meshes", loc_c, coarse.z._v.handle)):
        args = (loc, S, fine.z._v.handle, 2.0, None, None, other, zo, _lib.dptr(sums), C.byref(outside))
        for _ in range(5):
            _lib.call("mgb_field_norms", *args)
        backend.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            _lib.call("mgb_field_norms", *args)
        dt = (time.perf_counter() - t0) / reps
        lines.append("%-18s %9.2f us per call   %7.2f MB compulsory   %6.3f TB/s   %5.1f %% of HBM peak (bound: bandwidth)   outside %d"
                     % (name, 1e6 * dt, nbytes / 1e6, nbytes / dt / 1e12, 100.0 * nbytes / dt / HBM_PEAK, outside.value))
    err = M.error(fine, coarse)
    lines.append("L2 distance of the two solutions %.6e, H1 seminorm %.6e" % (err.lq[0], err.w1q[0]))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
