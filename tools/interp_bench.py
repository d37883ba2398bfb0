#!/usr/bin/env python3
"""Time mgb_interpolate (csrc/interp.hip) for m points on the fem2d level-L solution: the image a user would render.
GPU only.  usage: python3 tools/interp_bench.py [L=7] [m=1048576] [reps=100] [--out FILE]

m a perfect square: the regular sqrt(m) x sqrt(m) grid over the bounding box (sample_grid's points); otherwise uniform random
points.  Warm-up launches, then `reps` (>= 50) back-to-back launches on the context stream between two device
synchronisations, host clock around them: the context stream is not visible outside the library, so device events cannot be
recorded on it from here; the launches are asynchronous, so the window is kernel time plus one enqueue.  Bytes/s from the
compulsory traffic m * (8 dim + 8 S) (points in, values out; + 8 S dim with gradients); the nodal values and the bins are
shared by neighbouring points and stay in cache.  Share of HBM peak (8.0 TB/s spec): the kernel is bandwidth-bound by
construction (about 60 flop per 32 compulsory bytes in 2-D), so bandwidth is the bound that is named."""
import ctypes as C
import math
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
    m = int(argv[1]) if len(argv) > 1 else 1 << 20
    reps = max(50, int(argv[2])) if len(argv) > 2 else 100
    if M.device_count() <= 0:
        raise SystemExit("interp_bench: no HIP device visible")
    sol = M.fem2d_mpi_solve(L=L, p=1.0)
    geo = sol.geometry
    loc, backend = M._locator_of(geo)
    x = geo.x.to_numpy()
    n, dim = x.shape
    S = sol.z.shape[1]
    side = math.isqrt(m)
    if side * side == m:
        lo, hi = x.min(axis=0), x.max(axis=0)
        Y, X = np.meshgrid(np.linspace(lo[1], hi[1], side), np.linspace(lo[0], hi[0], side), indexing="ij")
        pts = np.stack([X, Y], axis=-1).reshape(-1, dim)
        kind = "%d x %d grid" % (side, side)
    else:
        rng = np.random.default_rng(0)
        pts = x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.random((m, dim))
        kind = "uniform random"
    pv = M.HPCVector(pts, backend)
    vals = M.HPCVector(m * S, backend)
    grads = M.HPCVector(m * S * dim, backend)
    lines = ["interp_bench: fem2d L=%d  n=%d  elements=%d  S=%d  m=%d (%s)  reps=%d" % (L, n, n // 7, S, m, kind, reps)]
    for name, gv, nbytes in (("values", None, m * (8 * dim + 8 * S)), ("values+gradients", grads, m * (8 * dim + 8 * S + 8 * S * dim))):
        args = (loc, m, pv.handle, S, sol.z._v.handle, vals.handle, gv.handle if gv is not None else None, None)
        for _ in range(5):
            _lib.call("mgb_interpolate", *args)
        backend.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            _lib.call("mgb_interpolate", *args)
        backend.synchronize()
        dt = (time.perf_counter() - t0) / reps
        lines.append("%-17s %9.2f us per launch   %7.1f MB compulsory   %6.3f TB/s   %5.1f %% of HBM peak (bound: bandwidth)"
                     % (name, 1e6 * dt, nbytes / 1e6, nbytes / dt / 1e12, 100.0 * nbytes / dt / HBM_PEAK))
    elem = np.empty(m, dtype=np.int32)
    _lib.call("mgb_interpolate", loc, m, pv.handle, S, sol.z._v.handle, vals.handle, None, _lib.iptr(elem))
    lines.append("points outside the mesh: %d" % int((elem < 0).sum()))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
