#!/usr/bin/env python3
"""Time sections() (csrc/section.hip) on fem2d / fem3d solutions, next to level_sets() / isosurfaces() and energy() on the same
fields, and measure the conservation gap of actual solves.  GPU only.
usage: python3 tools/section_bench.py [L=7] [nplanes=64] [--fem3d k] [--reps 50] [--gap L1,L2,...] [--out FILE]

Solves fem2d at L (or fem3d at L, k) with p = 1.5, takes planes x = x_0 spread over the domain and tilted a little, then times,
in this order and in the same run, for 1 and `nplanes` planes on the solution (B = 1) and on a batch of 16 distinct fields,
  sections, measure only      mgb_geo_sections without pieces: two launches, one copy, one wait
  sections, with pieces       ... plus the emit launch, its wait, and the copy of the pieces to the host
  level sets / isosurfaces    measure only, refine = 0, as many levels as planes: the same launch scheme, no quadrature
  energy                      mgb_geo_field_energy on the same fields: two launches, one copy, one wait
The host clock around `reps` calls measures what a user pays per call.  Lane utilisation of the quadrature: the items that
are cut, over the threads that are launched -- the uncut ones leave after the classification.

--gap L1,L2,...: the conservation gap of stationary solves with the default constant load f and p = 1.5.  With
Omega+ = {x > x_0}, Q = the flow rate through x = x_0 (sections) and F+ = boundary_flux over the part of the boundary with
x > x_0, the divergence theorem gives p (F+ - Q) = int_{Omega+} f; the total int f is p times the flux through the whole
boundary, and f is constant, so the gap printed is p (F+ - Q) - |Omega+| / |Omega| p F(boundary)."""
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


def solve(L, k):
    return M.fem3d_mpi_solve(L=L, k=k, p=P) if k else M.fem2d_mpi_solve(L=L, p=P)


def gap(levels, k):
    dim = 3 if k else 2
    lines = ["conservation gap: fem%dd%s, p = %g, default load; Q = sections().flux through x = x_0, F+ = boundary_flux on x > x_0"
             % (dim, " k=%d" % k if k else "", P)]
    for L in levels:
        sol = solve(L, k)
        whole = M.boundary_flux(sol, P).flux
        for x0 in (-0.5, 0.0, 0.5):
            plane = [1.0] + [0.0] * (dim - 1) + [x0]
            q = M.sections(sol, plane, p=P, pieces=False).flux
            fp = M.boundary_flux(sol, P, where=lambda c: c[0] > x0).flux
            share = (1.0 - x0) / 2.0
            lines.append("L=%d x_0=%5.2f  Q = %+.9f  F+ = %+.9f  p (F+ - Q) = %.9f  share of int f = %.9f  gap %+.3e"
                         % (L, x0, q, fp, P * (fp - q), share * P * whole, P * (fp - q) - share * P * whole))
    return lines


def main(argv):
    opts = {"--out": None, "--fem3d": "0", "--reps": "50", "--gap": ""}
    for flag in list(opts):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = argv[i + 1]
            argv = argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 7
    nplanes = max(1, int(argv[1])) if len(argv) > 1 else 64
    k, reps = int(opts["--fem3d"]), max(10, int(opts["--reps"]))
    if M.device_count() <= 0:
        raise SystemExit("section_bench: no HIP device visible")
    dim = 3 if k else 2
    sol = solve(L, k)
    loc, backend = M._locator_of(sol.geometry)
    n, S = sol.z.shape
    rng = np.random.default_rng(0)
    z0 = sol.z.to_numpy()
    u0 = z0[:, 0]
    fields = [sol.z] + [M.HPCMatrix(z0 * (1.0 + 1e-3 * rng.standard_normal(z0.shape)), backend) for _ in range(BATCH - 1)]
    f = M.HPCVector(np.full(n, 0.5), backend)
    block = sol.geometry.discretization["block"]
    items = (n // block) * (6 if k else 1)
    nwg = (items + 255) // 256
    lines = ["section_bench: fem%dd L=%d%s  n=%d  S=%d  p=%g  items per row=%d  workgroups per row=%d  reps=%d"
             % (dim, L, " k=%d" % k if k else "", n, S, P, items, nwg, reps)]
    for nc in sorted({1, nplanes}):
        c = -0.9 + 1.8 * (np.arange(nc) + 0.5) / nc
        planes = np.zeros((nc, dim + 1))
        planes[:, 0], planes[:, 1], planes[:, -1] = 1.0, 0.05, c
        levels = np.ascontiguousarray(u0.min() + (u0.max() - u0.min()) * (np.arange(nc) + 1.0) / (nc + 1.0))
        pp, lp = _lib.dptr(planes), _lib.dptr(levels)
        for B in (1, BATCH):
            table = (C.c_void_p * B)(*[zk._v.handle.value for zk in fields[:B]])
            rows, counts, eout = np.empty((B, nc, 5)), np.empty((B, nc), dtype=np.int64), np.empty((B, 5))
            cp = counts.ctypes.data_as(_lib.c_ll_p)

            def measure():
                _lib.call("mgb_geo_sections", loc, B, table, S, 0, nc, pp, P, _lib.dptr(rows), cp, None)

            measure()
            total = int(counts.sum())
            offsets, piece, item = np.empty(B * nc + 1, dtype=np.int64), np.empty((total, 6 if dim == 2 else 12)), np.empty(total, dtype=np.int32)

            def with_pieces():
                h = C.c_void_p()
                _lib.call("mgb_geo_sections", loc, B, table, S, 0, nc, pp, P, _lib.dptr(rows), cp, C.byref(h))
                _lib.call("mgb_levelset_get", h, offsets.ctypes.data_as(_lib.c_ll_p), _lib.dptr(piece), _lib.iptr(item))
                _lib.call("mgb_levelset_destroy", h)

            def marching():
                _lib.call("mgb_geo_isosurfaces" if k else "mgb_geo_level_sets", loc, B, table, S, 0, nc, lp, 0, _lib.dptr(rows), cp, None)

            def energy():
                _lib.call("mgb_geo_field_energy", loc, B, table, S, 0, S - 1, P, None, f.handle, 1, _lib.dptr(eout))

            with_pieces()
            cut = sum(len(np.unique(item[offsets[r]:offsets[r + 1]])) for r in range(B * nc))
            cases = (("sections, measure only", measure), ("sections, with pieces", with_pieces),
                     ("isosurfaces, measure only" if k else "level_sets, measure only", marching), ("energy", energy))
            times = {}
            for name, fn in cases:
                dt = times[name] = timed(fn, reps, backend)
                lines.append("planes=%-3d B=%-3d %-28s %9.2f us per call" % (nc, B, name, 1e6 * dt))
            tm, tp, tl, te = (times[c[0]] for c in cases)
            lines.append("planes=%-3d B=%-3d %d rows, %d pieces: measure only %.2f x marching, %.2f x energy; with pieces %.2f x energy; "
                         "cut items / launched threads = %d / %d = %.4f"
                         % (nc, B, B * nc, total, tm / tl, tm / te, tp / te, cut, B * nc * nwg * 256, cut / (B * nc * nwg * 256.0)))
    sec = M.sections(sol, [1.0] + [0.0] * (dim - 1) + [0.25], p=P)
    lines.append("solution, x = 0.25: measure %.12f  mean %.9f  flux %.9f  min %.6f  max %.6f  pieces %d"
                 % (sec.measure, sec.mean, sec.flux, sec.min, sec.max, sec.count))
    if opts["--gap"]:
        lines += gap([int(v) for v in opts["--gap"].split(",")], k)
    text = "\n".join(lines)
    print(text)
    if opts["--out"]:
        with open(opts["--out"], "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
