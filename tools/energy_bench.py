#!/usr/bin/env python3
"""Time energy() (csrc/energy.hip) on fem2d solutions, next to norms() on the same mesh.  GPU only.
usage: python3 tools/energy_bench.py [L=7] [B=16] [reps=50] [--out FILE]

Solves fem2d at L (p = 1.5), then times, in this order and in the same run,
  energy, one field      mgb_geo_field_energy on the solution, B = 1
  energy, B fields       ONE call on B distinct fields (the solution and B - 1 perturbed copies, separate allocations, as the
                         snapshots of a parabolic run are)
  energy, B single calls the same B fields one call each (what the batch replaces), reported per B calls
  norms                  mgb_field_norms on the solution (both columns, q = 2)
Every call is two launches, a copy of the results to the host and a wait, so the host clock around `reps` calls measures what
a user pays per call.  Bytes/s from the compulsory traffic: per node x (8 dim), w (8), f (8) once per call and z (8 S) per
field; norms reads x, w and z.  Share of HBM peak (8.0 TB/s spec): bandwidth is the bound by construction for both."""
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
P = 1.5


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
    L = int(argv[0]) if len(argv) > 0 else 7
    B = max(1, int(argv[1])) if len(argv) > 1 else 16
    reps = max(10, int(argv[2])) if len(argv) > 2 else 50
    if M.device_count() <= 0:
        raise SystemExit("energy_bench: no HIP device visible")
    sol = M.fem2d_mpi_solve(L=L, p=P)
    loc, backend = M._locator_of(sol.geometry)
    n, S = sol.z.shape
    dim = 2
    rng = np.random.default_rng(0)
    z0 = sol.z.to_numpy()
    fields = [sol.z] + [M.HPCMatrix(z0 * (1.0 + 1e-3 * rng.standard_normal(z0.shape)), backend) for _ in range(B - 1)]
    f = M.HPCVector(np.full(n, 0.5), backend)
    tables = [(C.c_void_p * 1)(zk._v.handle.value) for zk in fields]
    table = (C.c_void_p * B)(*[zk._v.handle.value for zk in fields])
    out1, outB, sums, outside = np.empty((1, 5)), np.empty((B, 5)), np.empty((S, 5)), C.c_longlong(0)

    def energy(tab, nb, out):
        _lib.call("mgb_geo_field_energy", loc, nb, tab, S, 0, S - 1, P, None, f.handle, 1, _lib.dptr(out))

    def singles():
        for tab in tables:
            energy(tab, 1, out1)

    shared = n * (8 * dim + 8 + 8)
    cases = (("energy, one field", lambda: energy(tables[0], 1, out1), shared + n * 8 * S),
             ("energy, %d fields" % B, lambda: energy(table, B, outB), shared + B * n * 8 * S),
             ("energy, %d single calls" % B, singles, B * (shared + n * 8 * S)),
             ("norms", lambda: _lib.call("mgb_field_norms", loc, S, sol.z._v.handle, 2.0, None, None, None, None, _lib.dptr(sums),
                                         C.byref(outside)), n * (8 * dim + 8 + 8 * S)))
    lines = ["energy_bench: fem2d L=%d  n=%d  S=%d  p=%g  B=%d  reps=%d" % (L, n, S, P, B, reps)]
    times = {}
    for name, fn, nbytes in cases:
        dt = times[name] = timed(fn, reps, backend)
        lines.append("%-26s %9.2f us per call   %7.2f MB compulsory   %6.3f TB/s   %5.1f %% of HBM peak (bound: bandwidth)"
                     % (name, 1e6 * dt, nbytes / 1e6, nbytes / dt / 1e12, 100.0 * nbytes / dt / HBM_PEAK))
    t1, tB, tS, tN = (times[c[0]] for c in cases)
    lines.append("one call on %d fields takes %.2f x the time of %d single calls; per field %.2f us batched, %.2f us alone"
                 % (B, tB / tS, B, 1e6 * tB / B, 1e6 * t1))
    lines.append("per node: energy %.3f ns (one field), %.3f ns (per field of the batch), norms %.3f ns (%d columns)"
                 % (1e9 * t1 / n, 1e9 * tB / (B * n), 1e9 * tN / n, S))
    singles()
    energy(table, B, outB)
    e = M.energy(sol, P, f=0.5)
    if outB[B - 1].tobytes() != out1[0].tobytes():            # out1 holds the last single call: field B - 1
        raise SystemExit("energy_bench: the batch and the single call disagree on field %d" % (B - 1))
    lines.append("solution: gradient %.12g  load %.12g  total %.12g  slack gap %.6e  margin %.6e  flux_max %.6g"
                 % (e.gradient, e.load, e.total, e.slack_gap, e.margin, e.flux_max))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
