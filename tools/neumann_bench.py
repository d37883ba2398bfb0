#!/usr/bin/env python3
"""Time neumann_load() (csrc/boundary.hip: boundary_load_kernel) on fem2d, next to boundary_flux() on the same geometry, and
measure the flux balance of mixed solves.  GPU only.
usage: python3 tools/neumann_bench.py [L=7] [B=16] [reps=200] [rounds=7] [--balance LMAX] [--out FILE]

Times, alternating the cases round after round in the same run (the method of tools/boundary_bench.py),
  boundary_load, one level     mgb_boundary_load for one field of h, every facet: copy of h, ONE launch, no wait
  boundary_load, B levels      ONE call for B time levels of h
  boundary_load, mask          one level with a facet mask (one more copy)
  load_add                     mgb_boundary_load_add of one level into a vector of n values
  neumann_load(), one level    the public function: the same plus the allocation of its result
  boundary_flux, one field     mgb_boundary_flux on a field of the same geometry: the yardstick (copies, launches, no node loop)
boundary_flux waits for its results, boundary_load does not; the host clock around `reps` calls with one wait at the end
measures what a caller pays per call.  Reported: the median of the rounds and their range.

--balance LMAX: mixed solves fem2d L = 2 .. LMAX, p = 1.5, default f and g, Dirichlet on x = -1, h = 0.3 + 0.2 y on the other
sides; with boundary_flux(where=...):  p flux(Gamma_D) - int h  (-> int f = 2)  and  p flux(Gamma_N) + int h  (-> 0)."""
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


def balance(lmax):
    lines = ["balance: fem2d, p = %g, Dirichlet on x = -1, h = 0.3 + 0.2 y elsewhere (int f = 2)" % P]
    left = lambda c: c[0] < -0.999
    for L in range(2, lmax + 1):
        sol = M.fem2d_mpi_solve(L=L, p=P, dirichlet=left, neumann=lambda x: 0.3 + 0.2 * x[1])
        g = sol.geometry
        b = M.boundary(g)
        on_d = np.array([left(c) for c in b.centre])
        load = M.neumann_load(g, lambda x: 0.3 + 0.2 * x[1], where=~on_d)
        int_h = float(g.w.to_numpy()[load.rows] @ load.values.to_numpy()[0])
        fd, fn = M.boundary_flux(sol, P, where=on_d), M.boundary_flux(sol, P, where=~on_d)
        lines.append("L=%d  newton steps %3d  int h = %.6f  p flux(Gamma_D) - int h = %.4f  p flux(Gamma_N) + int h = %.4f  "
                     "max |sigma . n| on Gamma_N = %.4f" % (L, int(sol.SOL_main["its"].sum()), int_h, P * fd.flux - int_h,
                                                            P * fn.flux + int_h, fn.normal_max))
    return lines


def main(argv):
    out_path, lmax = None, 0
    for flag in ("--out", "--balance"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--out":
                out_path = argv[i + 1]
            else:
                lmax = int(argv[i + 1])
            argv = argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 7
    B = max(1, int(argv[1])) if len(argv) > 1 else 16
    reps = max(10, int(argv[2])) if len(argv) > 2 else 200
    rounds = max(3, int(argv[3])) if len(argv) > 3 else 7
    if M.device_count() <= 0:
        raise SystemExit("neumann_bench: no HIP device visible")
    g = M.fem2d_mpi(L)
    x = g.x.to_numpy()
    n = x.shape[0]
    z = M.HPCMatrix(M._rows(M.DEFAULT_G[2], x), g.x.backend)
    M.boundary_flux(g, P, z=z)                                  # makes the device facet list
    loc, backend = M._locator_of(g)
    bd, b = g._boundary_dev, M.boundary(g)
    nf, q = b.nodes.shape
    rng = np.random.default_rng(0)
    h1, hB = rng.standard_normal((1, nf, q)), rng.standard_normal((B, nf, q))
    first = M.neumann_load(g, h1)
    nb = len(first.rows)
    out1, outB, y = M.HPCVector(nb, backend), M.HPCVector(B * nb, backend), M.HPCVector(n, backend)
    mask = np.ascontiguousarray(b.centre[:, 0] > 0.0, dtype=np.uint8)
    table1 = (C.c_void_p * 1)(z._v.handle.value)
    res = np.empty((1, 5))

    def load(hv, nlev, out, m=None):
        _lib.call("mgb_boundary_load", bd, nlev, _lib.dptr(hv), _lib.u8ptr(m), out.handle)

    cases = (("boundary_load, one level", lambda: load(h1, 1, out1)),
             ("boundary_load, %d levels" % B, lambda: load(hB, B, outB)),
             ("boundary_load, mask", lambda: load(h1, 1, out1, mask)),
             ("load_add", lambda: _lib.call("mgb_boundary_load_add", bd, out1.handle, 0, 1.0, y.handle, 1, 0)),
             ("neumann_load(), one level", lambda: M.neumann_load(g, h1)),
             ("boundary_flux, one field", lambda: _lib.call("mgb_boundary_flux", bd, 1, table1, 2, 0, P, None, None, None, _lib.dptr(res))))
    for _, fn in cases:
        for _ in range(20):
            fn()
    times = {name: [] for name, _ in cases}
    for _ in range(rounds):
        for name, fn in cases:
            times[name].append(timed(fn, reps, backend))
    lines = ["neumann_bench: fem2d L=%d  n=%d  facets=%d  facet nodes=%d  boundary rows=%d  B=%d  reps=%d  rounds=%d"
             % (L, n, nf, nf * q, nb, B, reps, rounds)]
    med = {}
    for name, _ in cases:
        t = np.array(times[name]) * 1e6
        med[name] = float(np.median(t))
        lines.append("%-28s %8.2f us per call (median of %d rounds; range %.2f .. %.2f)" % (name, med[name], rounds, t.min(), t.max()))
    names = [c[0] for c in cases]
    lines.append("boundary_load / boundary_flux: %.2f (one level), %.2f (%d levels)" % (med[names[0]] / med[names[5]],
                                                                                     med[names[1]] / med[names[5]], B))
    h0 = hB[:1].copy()
    load(hB, B, outB)
    load(h0, 1, out1)
    if outB.to_numpy()[:nb].tobytes() != out1.to_numpy().tobytes():
        raise SystemExit("neumann_bench: the batch and the single call disagree on level 0")
    if lmax >= 2:
        lines += balance(lmax)
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
