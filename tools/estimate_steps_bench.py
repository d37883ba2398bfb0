#!/usr/bin/env python3
"""Time estimate_steps() (csrc/estimate.hip) on a solved parabolic run, next to what the library offered
before for the same snapshots.  GPU only.
usage: python3 tools/estimate_steps_bench.py [L=7] [B=16] [--out FILE]

On fem2d at level L, B equal steps on [0, 1], p = 2, default data, microseconds per call of
  estimate_steps(par)        one call: flux of all B + 1 snapshots, facet terms, element indicators and the finish, each ONE launch
  B x estimate(snapshot)     the stationary indicator of snapshots 1 .. B, one call each: the yardstick for "does the batch pay"
  energy(par)                the two launches that reduce every snapshot of the run
  mgb_estimate_steps         the C call under estimate_steps() on vectors made once (no argument handling, no allocation) ...
  B x mgb_estimate           ... and the C call under estimate(), B times
Each is the host clock around 50 calls after 5 warm-up calls; every call ends in its own wait.  Also the compulsory bytes of one
estimate_steps call from the shapes alone (every array once: the snapshots read, the fluxes written and read, f, x and w read,
the per-facet values written and read, the facet tables read, the parts written) and the bytes per second that makes of the C
call.
Nothing here is a bar."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import ctypes as C          # noqa: E402
import mgb_amd as M         # noqa: E402
from mgb_amd import _lib    # noqa: E402

P, CALLS, WARM = 2.0, 50, 5


def timed(fn):
    for _ in range(WARM):
        fn()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    return (time.perf_counter() - t0) / CALLS * 1e6


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path, argv = argv[i + 1], argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 7
    B = int(argv[1]) if len(argv) > 1 else 16
    if M.device_count() <= 0:
        raise SystemExit("estimate_steps_bench: no HIP device visible")
    geo = M.fem2d_mpi(L)
    par = M.parabolic_solve(geo, p=P, ts=np.linspace(0.0, 1.0, B + 1))
    n, dim, S = len(geo.w), 2, par.u[0].shape[1]
    nel, nif = n // 7, len(M.interior(geo))
    nf, q = M.boundary(geo).nodes.shape
    ind = M.estimate_steps(par, P)
    t_steps = timed(lambda: M.estimate_steps(par, P))
    t_single = timed(lambda: [M.estimate(geo, P, f=0.5, z=par.u[k], scale=1.0) for k in range(1, B + 1)])
    t_energy = timed(lambda: M.energy(par, P, f=0.5))
    bd, backend = geo._boundary_dev, geo.x.backend
    ts = np.ascontiguousarray(par.ts, dtype=np.float64)
    fv = M.HPCVector(np.full(n, 0.5), backend)
    sigma, parts, eta = M.HPCVector((B + 1) * n * dim, backend), M.HPCVector(B * nel * 4, backend), M.HPCVector(3 * nel, backend)
    table = (C.c_void_p * (B + 1))(*[z._v.handle.value for z in par.u])
    out, out5 = np.empty((B, 2, 5)), np.empty(5)

    def c_steps():
        _lib.call("mgb_estimate_steps", bd, B, table, _lib.dptr(ts), S, 0, P, None, fv.handle, 1, 2.0, 1.0, None, 1, None, sigma.handle,
                  parts.handle, _lib.dptr(out))

    def c_single():
        for k in range(1, B + 1):
            _lib.call("mgb_estimate", bd, par.u[k]._v.handle, S, 0, P, None, fv.handle, 2.0, 1, 1.0, None, None, eta.handle, _lib.dptr(out5))

    t_csteps, t_csingle = timed(c_steps), timed(c_single)
    if parts.to_numpy().tobytes() != ind.parts.tobytes():
        raise SystemExit("estimate_steps_bench: the C call and estimate_steps() disagree")
    doubles = ((B + 1) * n * S + 2 * (B + 1) * n * dim + n + n * dim + n + 2 * B * nif + B * nel * 4 + nif * q + nif * dim)
    ints = nif * 2 * q + nel * 3
    nbytes = 8 * doubles + 4 * ints
    lines = ["estimate_steps_bench: fem2d L=%d  n=%d  elements=%d  interior facets=%d  boundary facets=%d  steps B=%d  S=%d  calls=%d after %d"
             % (L, n, nel, nif, nf, B, S, CALLS, WARM),
             "estimate_steps(par)        %10.2f us per call" % t_steps,
             "%2d x estimate(snapshot)    %10.2f us per %d calls  (%.2f us each)" % (B, t_single, B, t_single / B),
             "energy(par)                %10.2f us per call" % t_energy,
             "mgb_estimate_steps         %10.2f us per call" % t_csteps,
             "%2d x mgb_estimate          %10.2f us per %d calls  (%.2f us each)" % (B, t_csingle, B, t_csingle / B),
             "single calls / one batched call: %.2f (public functions)  %.2f (C calls)" % (t_single / t_steps, t_csingle / t_csteps),
             "compulsory bytes of one estimate_steps call: %d (%.2f MB)  ->  %.2f GB/s" % (nbytes, nbytes / 1e6, nbytes / t_csteps / 1e3),
             "total %.6e  total_space %.6e  total_time %.6e" % (ind.total, ind.total_space, ind.total_time)]
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
