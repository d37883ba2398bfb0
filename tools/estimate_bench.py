#!/usr/bin/env python3
"""Time estimate() (csrc/estimate.hip) on the fem2d solution, next to energy() and boundary_flux() on the same field, and measure
the indicators of the default problem and of adapt() on the L shape.  GPU only.
usage: python3 tools/estimate_bench.py [L=7] [reps=200] [rounds=7] [--totals LMAX] [--adapt STEPS] [--out FILE]

Times, alternating the cases round after round in the same run (the method of tools/neumann_bench.py),
  mgb_estimate                  the C call on a device field: flux launch, facet terms, element indicators, finish, one wait
  mgb_estimate, Neumann + mask  the same with h on every second boundary facet (two more copies on the stream)
  estimate()                    the public function: the same plus its Python argument handling and the result vector
  mgb_geo_field_energy          the yardsticks on the same field: two launches over the nodes and one wait ...
  mgb_boundary_flux             ... and two launches over the boundary facets and one wait
Reported: the median of the rounds and their range, and the ratios to the two yardsticks.

--totals LMAX: the default fem2d problem (p = 1.5 and 2) solved at L = 2 .. LMAX: `total` and its three parts.
--adapt STEPS: adapt() on the L shape, L = 2, p = 2, theta = 0.5: `total`, triangles and rows per step.
These are measurements of the discretisation, not bars."""
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
L_SHAPE = np.array([[-1, -1], [0, -1], [0, 0], [-1, -1], [0, 0], [-1, 0], [0, -1], [1, -1], [1, 0],
                    [0, -1], [1, 0], [0, 0], [-1, 0], [0, 0], [0, 1], [-1, 0], [0, 1], [-1, 1]], dtype=float)


def timed(fn, reps, backend):
    backend.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    backend.synchronize()
    return (time.perf_counter() - t0) / reps


def totals(lmax):
    lines = ["totals: fem2d, default f and g, estimate(sol, p, f=0.5)"]
    for p in (2.0, 1.5):
        for L in range(2, lmax + 1):
            sol = M.fem2d_mpi_solve(L=L, p=p)
            ind = M.estimate(sol, p, f=0.5)
            lines.append("p=%g L=%d  rows %7d  total %.6f  volume %.6e  jump %.6e  eta_max %.4e  jump_max %.4e"
                         % (p, L, len(sol.geometry.w), ind.total, ind.volume, ind.jump, ind.eta_max, ind.jump_max))
    return lines


def adapt(steps):
    lines = ["adapt: L shape, L = 2, p = 2, theta = 0.5"]
    for k, (K, sol, ind) in enumerate(M.adapt(L_SHAPE, 2, 2.0, steps, theta=0.5)):
        lines.append("step %d  triangles %4d  rows %6d  total %.6f  newton steps %d"
                     % (k, len(K) // 3, len(sol.geometry.w), ind.total, int(sol.SOL_main["its"].sum())))
    for L in (2, 3, 4):
        sol = M.fem2d_mpi_solve(L=L, K=L_SHAPE, p=2.0)
        lines.append("uniform L=%d  rows %6d  total %.6f" % (L, len(sol.geometry.w), M.estimate(sol, 2.0, f=0.5).total))
    return lines


def main(argv):
    out_path, lmax, steps = None, 0, -1
    for flag in ("--out", "--totals", "--adapt"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--out":
                out_path = argv[i + 1]
            elif flag == "--totals":
                lmax = int(argv[i + 1])
            else:
                steps = int(argv[i + 1])
            argv = argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 7
    reps = max(10, int(argv[1])) if len(argv) > 1 else 200
    rounds = max(3, int(argv[2])) if len(argv) > 2 else 7
    if M.device_count() <= 0:
        raise SystemExit("estimate_bench: no HIP device visible")
    sol = M.fem2d_mpi_solve(L=L, p=P)
    g, z = sol.geometry, sol.z
    n = len(g.w)
    first = M.estimate(sol, P, f=0.5)                             # makes the device facet lists
    loc, backend = M._locator_of(g)
    bd, b = g._boundary_dev, M.boundary(g)
    nf, q = b.nodes.shape
    nel = n // 7
    fv = M.HPCVector(np.full(n, 0.5), backend)
    eta = M.HPCVector(3 * nel, backend)
    h = np.random.default_rng(0).standard_normal((nf, q))
    mask = np.ascontiguousarray(np.arange(nf) % 2, dtype=np.uint8)
    table = (C.c_void_p * 1)(z._v.handle.value)
    res, res5 = np.empty(5), np.empty((1, 5))

    def est(hv=None, m=None):
        _lib.call("mgb_estimate", bd, z._v.handle, 2, 0, P, None, fv.handle, 2.0, 0, 1.0, _lib.dptr(hv), _lib.u8ptr(m), eta.handle, _lib.dptr(res))

    cases = (("mgb_estimate", lambda: est()),
             ("mgb_estimate, Neumann + mask", lambda: est(h, mask)),
             ("estimate()", lambda: M.estimate(sol, P, f=0.5)),
             ("mgb_geo_field_energy", lambda: _lib.call("mgb_geo_field_energy", loc, 1, table, 2, 0, 1, P, None, fv.handle, 1, _lib.dptr(res5))),
             ("mgb_boundary_flux", lambda: _lib.call("mgb_boundary_flux", bd, 1, table, 2, 0, P, None, None, None, _lib.dptr(res5))))
    for _, fn in cases:
        for _ in range(20):
            fn()
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            times[name].append(timed(fn, reps, backend))
    lines = ["estimate_bench: fem2d L=%d  n=%d  elements=%d  interior facets=%d  boundary facets=%d  reps=%d  rounds=%d"
             % (L, n, nel, len(M.interior(g)), nf, reps, rounds)]
    med = {}
    for name, _ in cases:
        t = np.array(times[name]) * 1e6
        med[name] = float(np.median(t))
        lines.append("%-30s %8.2f us per call (median of %d rounds; range %.2f .. %.2f)" % (name, med[name], rounds, t.min(), t.max()))
    lines.append("mgb_estimate / mgb_geo_field_energy: %.2f   mgb_estimate / mgb_boundary_flux: %.2f"
                 % (med["mgb_estimate"] / med["mgb_geo_field_energy"], med["mgb_estimate"] / med["mgb_boundary_flux"]))
    est()
    if eta.to_numpy().tobytes() != first.parts.tobytes():
        raise SystemExit("estimate_bench: the C call and estimate() disagree")
    lines.append("total %.6f at L=%d, p=%g" % (first.total, L, P))
    if lmax >= 2:
        lines += totals(lmax)
    if steps >= 0:
        lines += adapt(steps)
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
