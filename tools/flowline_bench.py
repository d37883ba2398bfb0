#!/usr/bin/env python3
"""Time flow_lines() (csrc/flowline.hip) on a solution, next to interpolate(grad=True) on as many point evaluations.  GPU only.
usage: python3 tools/flowline_bench.py [L=7] [m ...=4096 65536] [--fem3d K] [--reps N] [--max-steps N] [--out FILE]

Solves fem2d at L (or fem3d at L with degree K), p = 1, puts m seeds on a regular grid strictly inside the domain and times, in
this order and in the same run, for each m and each workgroup size 64, 128, 256:
  flow_lines, summaries only     one launch, two copies, one wait
  flow_lines, with paths         ... plus the fixed-stride path buffer, the gather launch and the copy of the points to the host
and then interpolate(grad=True) on 2 x (accepted steps) points (two gradient evaluations per step), capped at 2^22 points and
scaled, which is what a host loop around interpolate() would launch in total -- without its one wait per step.
The host clock around `reps` calls measures what a user pays per call.  Reported per case: us per call, accepted steps per
second, and the lane utilisation sum(count) / (64 sum over waves of the wave's largest count), from `count` on the host: the
share of lane-steps that did work while their wave was alive."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import mgb_amd as M         # noqa: E402

P = 1.0


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


def utilisation(count):
    c = np.asarray(count, dtype=np.int64).ravel()
    pad = (-len(c)) % 64
    w = np.concatenate([c, np.zeros(pad, dtype=np.int64)]).reshape(-1, 64)
    return c.sum() / max(1, 64 * w.max(axis=1).sum())


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
    max_steps = int(option(argv, "--max-steps", 1024))
    L = int(argv[0]) if argv else 7
    ms = [int(a) for a in argv[1:]] or [4096, 65536]
    if M.device_count() <= 0:
        raise SystemExit("flowline_bench: no HIP device visible")
    if k is None:
        sol, dim, what = M.fem2d_mpi_solve(L=L, p=P), 2, "fem2d L=%d" % L
    else:
        sol, dim, what = M.fem3d_mpi_solve(L=L, k=int(k), p=P), 3, "fem3d L=%d k=%s" % (L, k)
    loc, backend = M._locator_of(sol.geometry)
    n, S = sol.z.shape
    x = sol.geometry.x.to_numpy().reshape(n, dim)
    lines = ["flowline_bench: %s  p=%g  n=%d  S=%d  max_steps=%d  reps=%d" % (what, P, n, S, max_steps, reps)]
    for m in ms:
        seeds = grid_seeds(m, dim, x.min(), x.max())
        fl = M.flow_lines(sol, seeds, p=P, max_steps=max_steps, paths=False)
        steps = int(np.maximum(fl.count - 1, 0).sum())
        lines.append("m=%d seeds  ds=%.6g  accepted steps (and exits) %d  status counts %s  lane utilisation %.3f  longest line %d points"
                     % (len(seeds), fl.ds, steps, np.bincount(fl.status, minlength=5).tolist(), utilisation(fl.count), int(fl.count.max())))
        for paths in (False, True):
            r = reps if not paths or len(seeds) <= 8192 else max(2, reps // 5)
            for wg in (64, 128, 256):
                dt = timed(lambda: M.flow_lines(sol, seeds, p=P, max_steps=max_steps, paths=paths, workgroup=wg), r, backend)
                lines.append("m=%-6d %-14s workgroup %-3d  %11.1f us per call   %8.2f M steps/s" %
                             (len(seeds), "with paths" if paths else "summaries", wg, 1e6 * dt, steps / dt / 1e6))
        npts = min(2 * steps, 1 << 22)
        if npts > 0:
            rng = np.random.default_rng(0)
            pts = np.ascontiguousarray(seeds[rng.integers(0, len(seeds), npts)])
            dt = timed(lambda: M.interpolate(sol, pts, grad=True), reps, backend)
            lines.append("m=%-6d interpolate(grad=True) on %d points: %.1f us per call, %.3f ns per point; on 2 x steps = %d points: %.1f us"
                         % (len(seeds), npts, 1e6 * dt, 1e9 * dt / npts, 2 * steps, 1e6 * dt * 2 * steps / npts))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
