#!/usr/bin/env python3
"""Time boundary_flux() (csrc/boundary.hip) on fem2d solutions, next to energy() on the same fields.  GPU only.
usage: python3 tools/boundary_bench.py [L=7] [B=16] [reps=200] [rounds=7] [--out FILE]

Solves fem2d at L (p = 1.5), then times, alternating the four cases round after round in the same run,
  boundary_flux, one field   mgb_boundary_flux on the solution, B = 1, every facet, no per-facet output
  energy, one field          mgb_geo_field_energy on the same field
  boundary_flux, B fields    ONE call on B distinct fields (the solution and B - 1 perturbed copies, separate allocations)
  energy, B fields           the same B fields
and once more boundary_flux with a facet mask and the per-facet output (one more copy each way).  Every call is two launches, a
copy of the results to the host and a wait, so the host clock around `reps` calls measures what a user pays per call: at
O(surface nodes) of work that is the price of two launches, a wait and a copy, which energy() pays too -- the yardstick.  Reported:
the median of the rounds and their range."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import mgb_amd as M         # noqa: E402
from mgb_amd import _lib    # noqa: E402

P = 1.5


def timed(fn, reps, backend):
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
    reps = max(10, int(argv[2])) if len(argv) > 2 else 200
    rounds = max(3, int(argv[3])) if len(argv) > 3 else 7
    if M.device_count() <= 0:
        raise SystemExit("boundary_bench: no HIP device visible")
    sol = M.fem2d_mpi_solve(L=L, p=P)
    loc, backend = M._locator_of(sol.geometry)
    n, S = sol.z.shape
    rng = np.random.default_rng(0)
    z0 = sol.z.to_numpy()
    fields = [sol.z] + [M.HPCMatrix(z0 * (1.0 + 1e-3 * rng.standard_normal(z0.shape)), backend) for _ in range(B - 1)]
    first = M.boundary_flux(sol, P, per_facet=True)       # makes the device facet list
    bd, b = sol.geometry._boundary_dev, M.boundary(sol.geometry)
    nf, q = b.nodes.shape
    table1 = (C.c_void_p * 1)(fields[0]._v.handle.value)
    tableB = (C.c_void_p * B)(*[zk._v.handle.value for zk in fields])
    out1, outB, fac = np.empty((1, 5)), np.empty((B, 5)), np.empty((1, nf))
    mask = np.ascontiguousarray(b.centre[:, 0] > 0.0, dtype=np.uint8)

    def flux(tab, nb, out, m=None, f=None):
        _lib.call("mgb_boundary_flux", bd, nb, tab, S, 0, P, None, _lib.u8ptr(m), _lib.dptr(f), _lib.dptr(out))

    def energy(tab, nb, out):
        _lib.call("mgb_geo_field_energy", loc, nb, tab, S, 0, S - 1, P, None, None, 1, _lib.dptr(out))

    cases = (("boundary_flux, one field", lambda: flux(table1, 1, out1)),
             ("energy, one field", lambda: energy(table1, 1, out1)),
             ("boundary_flux, %d fields" % B, lambda: flux(tableB, B, outB)),
             ("energy, %d fields" % B, lambda: energy(tableB, B, outB)),
             ("boundary_flux, mask + facets", lambda: flux(table1, 1, out1, mask, fac)))
    for _, fn in cases:
        for _ in range(20):
            fn()
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            times[name].append(timed(fn, reps, backend))
    lines = ["boundary_bench: fem2d L=%d  n=%d  S=%d  p=%g  facets=%d  facet nodes=%d  B=%d  reps=%d  rounds=%d"
             % (L, n, S, P, nf, nf * q, B, reps, rounds)]
    med = {}
    for name, _ in cases:
        t = np.array(times[name]) * 1e6
        med[name] = float(np.median(t))
        lines.append("%-30s %8.2f us per call (median of %d rounds; range %.2f .. %.2f)" % (name, med[name], rounds, t.min(), t.max()))
    names = [c[0] for c in cases]
    lines.append("boundary_flux / energy: %.2f (one field), %.2f (%d fields)" % (med[names[0]] / med[names[1]], med[names[2]] / med[names[3]], B))
    flux(tableB, B, outB)
    flux(table1, 1, out1)
    if outB[0].tobytes() != out1[0].tobytes():
        raise SystemExit("boundary_bench: the batch and the single call disagree on field 0")
    f = np.array([M.DEFAULT_F[2](xi)[0] for xi in sol.geometry.x.to_numpy()])
    lines.append("solution: flux %.12g  trace %.12g  measure %.12g  normal_max %.6g  tangential_max %.6g"
                 % (first.flux, first.trace, first.measure, first.normal_max, first.tangential_max))
    lines.append("balance: p * flux = %.6g against int f = %.6g" % (P * first.flux, float(sol.geometry.w.to_numpy() @ f)))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
