#!/usr/bin/env python3
"""Time line_integrals() and project() (csrc/ray.hip) on a solution, next to interpolate() on as many point evaluations and,
in 2-D, sections() on 64 lines.  GPU only.
usage: python3 tools/line_integrals_bench.py [L=7] [m ...=4096 65536] [--fem3d K] [--reps N] [--out FILE]

Solves fem2d at L (or fem3d at L with degree K), p = 1.  In 3-D the rays are those of project(shape=(s, s)) along z with
s = round(sqrt(m)) (m = 65536 gives the 256 x 256 image); in 2-D they are m seeded random chords across the bounding box.
For each m and each workgroup size 64, 128, 256, in this order and in the same run:
  line_integrals, rows only      one launch, two copies, one wait
  line_integrals, with pieces    ... plus the second walk that writes the pieces, and their copy to the host
and then interpolate() on (Gauss points + 2) x pieces points (what the quadrature evaluates), capped at 2^22 points and scaled,
and in 2-D sections() on 64 lines.  The host clock around `reps` calls measures what a user pays per call.  Reported per case:
us per call, pieces per second, and the lane utilisation sum(count) / (64 sum over waves of the wave's largest count), from
`count` on the host: the share of lane-pieces that did work while their wave was alive."""
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
    L = int(argv[0]) if argv else 7
    ms = [int(a) for a in argv[1:]] or [4096, 65536]
    if M.device_count() <= 0:
        raise SystemExit("line_integrals_bench: no HIP device visible")
    if k is None:
        sol, dim, what = M.fem2d_mpi_solve(L=L, p=P), 2, "fem2d L=%d" % L
    else:
        sol, dim, what = M.fem3d_mpi_solve(L=L, k=int(k), p=P), 3, "fem3d L=%d k=%s" % (L, k)
    loc, backend = M._locator_of(sol.geometry)
    n, S = sol.z.shape
    x = sol.geometry.x.to_numpy().reshape(n, dim)
    lo, hi = x.min(axis=0), x.max(axis=0)
    gauss = 4 if dim == 2 else {1: 3, 2: 4, 3: 6}[int(k)]
    lines = ["line_integrals_bench: %s  p=%g  n=%d  S=%d  reps=%d" % (what, P, n, S, reps)]
    for m in ms:
        if dim == 3:
            s = max(1, int(round(m ** 0.5)))
            X = np.stack(np.meshgrid(*[lo[d] + (np.arange(s) + 0.5) * (hi[d] - lo[d]) / s for d in (1, 0)], indexing="ij")[::-1], axis=-1).reshape(-1, 2)
            a = np.concatenate([X, np.full((len(X), 1), lo[2])], axis=1)
            b = np.concatenate([X, np.full((len(X), 1), hi[2])], axis=1)
            kind = "project %d x %d" % (s, s)
        else:
            rng = np.random.default_rng(0)
            a, b = lo + (hi - lo) * rng.uniform(size=(m, 2)), lo + (hi - lo) * rng.uniform(size=(m, 2))
            kind = "random chords"
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        res = M.line_integrals(sol, a, b, p=P)
        pieces = int(res.count.sum())
        lines.append("m=%d rays (%s)  pieces %d  longest ray %d pieces  lane utilisation %.3f"
                     % (len(a), kind, pieces, int(res.count.max()), utilisation(res.count)))
        for with_pieces in (False, True):
            for wg in (64, 128, 256):
                dt = timed(lambda: M.line_integrals(sol, a, b, p=P, pieces=with_pieces, workgroup=wg), reps, backend)
                lines.append("m=%-6d %-12s workgroup %-3d  %11.1f us per call   %8.2f M pieces/s" %
                             (len(a), "with pieces" if with_pieces else "rows only", wg, 1e6 * dt, pieces / dt / 1e6))
        if dim == 3:
            dt = timed(lambda: M.project(sol, shape=(s, s), p=P), reps, backend)
            lines.append("m=%-6d project(shape=(%d, %d)), rays built on the host included: %.1f us per call" % (len(a), s, s, 1e6 * dt))
        npts = min((gauss + 2) * pieces, 1 << 22)
        if npts > 0:
            rng = np.random.default_rng(1)
            t = rng.uniform(size=(npts, 1))
            j = rng.integers(0, len(a), npts)
            pts = np.ascontiguousarray(a[j] + t * (b[j] - a[j]))
            dt = timed(lambda: M.interpolate(sol, pts), reps, backend)
            lines.append("m=%-6d interpolate on %d points: %.1f us per call, %.3f ns per point; on (%d + 2) x pieces = %d points: %.1f us"
                         % (len(a), npts, 1e6 * dt, 1e9 * dt / npts, gauss, (gauss + 2) * pieces, 1e6 * dt * (gauss + 2) * pieces / npts))
    if dim == 2:
        c = np.linspace(lo[0], hi[0], 66)[1:-1]
        planes = np.stack([np.ones(64), 0.3 * np.ones(64), c], axis=1)
        dt = timed(lambda: M.sections(sol, planes, p=P, pieces=False), reps, backend)
        lines.append("sections on 64 lines, no pieces: %.1f us per call, %.1f us per line" % (1e6 * dt, 1e6 * dt / 64))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
