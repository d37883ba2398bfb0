#!/usr/bin/env python3
"""Time path_lines() (csrc/pathline.hip) through a parabolic run, next to flow_lines() on the same number of steps.  GPU only.
usage: python3 tools/pathline_bench.py [L=7] [m ...=4096 65536] [--fem3d K] [--reps N] [--substeps N] [--out FILE]

Runs parabolic_solve at fem2d L (or fem3d L with degree K), p = 2, h = 0.25 (5 snapshots), puts m seeds on a regular grid
strictly inside the domain, releases all of them at ts[0] and times, in this order and in the same run, for each m and each
workgroup size 64, 128, 256:
  path_lines, summaries only     one launch, four uploads, two copies, one wait
  path_lines, with paths         ... plus the fixed-stride path buffer, the gather launch and the copy of the points to the host
and then flow_lines(paths=False) on the last snapshot with max_steps = 4 x substeps, the same number of steps per seed.
The host clock around `reps` calls measures what a user pays per call.  Reported per case: us per call, accepted steps per
second, and the lane utilisation accepted steps / (waves x 64 x longest row), waves = ceil(m / 64), the longest row in accepted
steps, from `count` on the host: the share of lane-steps that did work if every wave lived as long as the longest row."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import mgb_amd as M         # noqa: E402

P = 2.0


def timed(fn, reps, backend):
    for _ in range(2):
        fn()
    backend.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    backend.synchronize()
    return (time.perf_counter() - t0) / reps


def grid_seeds(m, dim, lo, hi):
    """about m points of a regular grid strictly inside the box [lo, hi]^dim, irrationally offset from the mesh lines"""
    per = max(1, int(round(m ** (1.0 / dim))))
    t = lo + (hi - lo) * (np.arange(per) + 0.5 - 0.0137) / per
    g = np.stack(np.meshgrid(*([t] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    return np.ascontiguousarray(g[:m] if len(g) >= m else g)


def utilisation(steps):
    s = np.asarray(steps, dtype=np.int64).ravel()
    waves = (len(s) + 63) // 64
    return s.sum() / max(1, waves * 64 * int(s.max()))


def option(argv, name, default):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


def main(argv):
    argv = list(argv)
    out_path = option(argv, "--out", None)
    k = option(argv, "--fem3d", None)
    reps = int(option(argv, "--reps", 10))
    substeps = int(option(argv, "--substeps", 64))
    L = int(argv[0]) if argv else 7
    ms = [int(a) for a in argv[1:]] or [4096, 65536]
    if M.device_count() <= 0:
        raise SystemExit("pathline_bench: no HIP device visible")
    if k is None:
        geo, dim, what = M.fem2d_mpi(L), 2, "fem2d L=%d" % L
    else:
        geo, dim, what = M.fem3d_mpi(L, k=int(k)), 3, "fem3d L=%d k=%s" % (L, k)
    t0 = time.perf_counter()
    par = M.parabolic_solve(geo, h=0.25, p=P)
    t_solve = time.perf_counter() - t0
    loc, backend = M._locator_of(geo)
    n, S = par.u[0].shape
    B = len(par.ts)
    x = geo.x.to_numpy().reshape(n, dim)
    lines = ["pathline_bench: %s  p=%g  n=%d  S=%d  B=%d  substeps=%d  steps per seed %d  reps=%d  (parabolic_solve %.1f s)"
             % (what, P, n, S, B, substeps, (B - 1) * substeps, reps, t_solve)]
    for m in ms:
        seeds = grid_seeds(m, dim, x.min(), x.max())
        pl = M.path_lines(par, seeds, p=P, substeps=substeps, paths=False)
        acc = np.maximum(pl._accepted(), 0)
        steps = int(acc.sum())
        lines.append("m=%d seeds  accepted steps %d  status counts %s  rested %d  lane utilisation %.3f  longest row %d steps"
                     % (len(seeds), steps, np.bincount(pl.status, minlength=4).tolist(), int(pl.rested.sum()), utilisation(acc), int(acc.max())))
        for paths in (False, True):
            r = reps if not paths or len(seeds) <= 8192 else max(2, reps // 5)
            for wg in (64, 128, 256):
                dt = timed(lambda: M.path_lines(par, seeds, p=P, substeps=substeps, paths=paths, workgroup=wg), r, backend)
                lines.append("m=%-6d %-14s workgroup %-3d  %11.1f us per call   %8.2f M steps/s" %
                             (len(seeds), "with paths" if paths else "summaries", wg, 1e6 * dt, steps / dt / 1e6))
        fl = M.flow_lines(geo, seeds, p=P, z=par.u[-1], direction=-1, max_steps=(B - 1) * substeps, paths=False)
        fsteps = int(np.maximum(fl.count - 1, 0).sum())
        dt = timed(lambda: M.flow_lines(geo, seeds, p=P, z=par.u[-1], direction=-1, max_steps=(B - 1) * substeps, paths=False), reps, backend)
        lines.append("m=%-6d flow_lines(last snapshot, max_steps=%d, summaries): accepted steps (and exits) %d  status counts %s  "
                     "%.1f us per call  %.2f M steps/s" % (len(seeds), (B - 1) * substeps, fsteps, np.bincount(fl.status, minlength=5).tolist(),
                                                           1e6 * dt, fsteps / dt / 1e6))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
