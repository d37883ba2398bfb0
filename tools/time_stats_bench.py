#!/usr/bin/env python3
"""Time time_stats() (csrc/timestat.hip) on a parabolic_solve run of fem2d, next to energy() on the same run.  GPU only.
usage: python3 tools/time_stats_bench.py [L=7] [steps=20] [nl=8] [reps=50] [--out FILE]

Runs parabolic_solve(fem2d L, h = 1 / steps, p = 2), B = steps + 1 snapshots, takes nl levels evenly inside the range of u,
then times, in this order and in the same process,
  time_stats, no levels       mgb_geo_time_stats with nl = 0: two launches, one upload, one wait, one copy of one row
  time_stats, nl levels       ... with the level table: 1 + ceil(nl / chunk) slabs of workgroups, each of which reads the run once
  energy                      mgb_geo_field_energy on the same B snapshots: two launches, one wait, one copy
  M.time_stats(par, levels)   the public call, which also allocates the two tables
with the host clock around `reps` calls, each of which ends in its own wait: what a user pays per call.
Compulsory bytes of time_stats: B n S 8 read (the column stride fetches whole rows) plus n 8 of weights, n 64 of node table and
nl n 40 of level table written.  What the level slabs read again beyond the first pass is not compulsory and is not counted.
Every case is timed twice: on the same run every call, where the set stays in whatever cache holds it (the line says which:
4 MiB of L2 per XCD, 256 MiB of Infinity Cache), and rotating over copies of the run in separate allocations that together
exceed twice the Infinity Cache, so that every call reads its snapshots from HBM."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np          # noqa: E402
import mgb_amd as M         # noqa: E402
from mgb_amd import _lib    # noqa: E402

P = 2.0
L2_BYTES, L3_BYTES = 4 << 20, 256 << 20


def timed(fn, reps):
    """seconds per call of fn(k), k the call's number; every call waits for its own result"""
    for k in range(5):
        fn(k)
    t0 = time.perf_counter()
    for k in range(reps):
        fn(k)
    return (time.perf_counter() - t0) / reps


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    L = int(argv[0]) if len(argv) > 0 else 7
    steps = max(1, int(argv[1])) if len(argv) > 1 else 20
    nl = max(1, int(argv[2])) if len(argv) > 2 else 8
    reps = max(10, int(argv[3])) if len(argv) > 3 else 50
    if M.device_count() <= 0:
        raise SystemExit("time_stats_bench: no HIP device visible")
    par = M.parabolic_solve(M.fem2d_mpi(L), h=1.0 / steps, p=P)
    loc, backend = M._locator_of(par.geometry)
    B = len(par.u)
    n, S = par.u[0].shape
    ts = np.ascontiguousarray(par.ts, dtype=np.float64)
    snaps = [zk.to_numpy() for zk in par.u]
    lo, hi = min(z[:, 0].min() for z in snaps), max(z[:, 0].max() for z in snaps)
    levels = np.ascontiguousarray(lo + (hi - lo) * (np.arange(nl) + 1.0) / (nl + 1.0))
    set_bytes = B * n * S * 8
    copies = max(2, -(-2 * L3_BYTES // set_bytes))
    runs = [list(par.u)] + [[M.HPCMatrix(z, backend) for z in snaps] for _ in range(copies - 1)]
    tables = [(C.c_void_p * B)(*[zk._v.handle.value for zk in run]) for run in runs]
    where = "L2" if set_bytes <= L2_BYTES else "Infinity Cache" if set_bytes <= L3_BYTES else "HBM"
    lines = ["time_stats_bench: fem2d L=%d  n=%d  S=%d  B=%d snapshots  nl=%d  workgroups=%d  reps=%d" % (L, n, S, B, nl, (n + 255) // 256, reps),
             "one run is %.2f MB: the same run every call is read from %s; rotating over %d copies (%.0f MB) reads from HBM"
             % (set_bytes / 1e6, where, copies, copies * set_bytes / 1e6)]
    node, level = M.HPCVector(n * 8, backend), M.HPCVector(nl * n * 5, backend)
    rows, erows = np.empty((1 + nl, 5)), np.empty((B, 5))
    f = M.HPCVector(np.full(n, 0.5), backend)
    tp, lp = _lib.dptr(ts), _lib.dptr(levels)

    def stats0(k, rot):
        _lib.call("mgb_geo_time_stats", loc, B, tables[k % copies if rot else 0], tp, S, 0, 0, None, float("nan"), node.handle, None, _lib.dptr(rows))

    def stats(k, rot):
        _lib.call("mgb_geo_time_stats", loc, B, tables[k % copies if rot else 0], tp, S, 0, nl, lp, float("nan"), node.handle, level.handle,
                  _lib.dptr(rows))

    def energy(k, rot):
        _lib.call("mgb_geo_field_energy", loc, B, tables[k % copies if rot else 0], S, 0, S - 1, P, None, f.handle, 1, _lib.dptr(erows))

    pars = [M.ParabolicSOL(par.geometry, par.ts, run) for run in runs]

    def public(k, rot):
        M.time_stats(pars[k % copies if rot else 0], levels)

    read = set_bytes + n * 8
    cases = (("time_stats, no levels", stats0, read + n * 64),
             ("time_stats, %d levels" % nl, stats, read + n * 64 + nl * n * 40),
             ("energy", energy, B * n * S * 8 + n * (16 + 8 + 8)),
             ("M.time_stats(par, levels)", public, read + n * 64 + nl * n * 40))
    for rot in (False, True):
        times = {}
        for name, fn, nbytes in cases:
            dt = times[name] = timed(lambda k: fn(k, rot), reps)
            lines.append("%-9s %-28s %9.2f us per call   %8.3f MB compulsory   %6.3f TB/s"
                         % ("rotating" if rot else "same run", name, 1e6 * dt, nbytes / 1e6, nbytes / dt / 1e12))
        t0, tl, te, _ = (times[c[0]] for c in cases)
        lines.append("%-9s time_stats without levels %.2f x energy, with %d levels %.2f x energy; %.3f ns per node and snapshot without levels"
                     % ("rotating" if rot else "same run", t0 / te, nl, tl / te, 1e9 * t0 / (B * n)))
    st = M.time_stats(par, levels)
    lines.append("run: total dose %.9g  peak %.9g  trough %.9g  total variation %.9g" % (st.total, st.peak, st.trough, st.total_variation))
    lines.append("     levels %s" % np.array2string(levels, precision=6))
    lines.append("     reached measure %s" % np.array2string(st.reached_measure, precision=9))
    lines.append("     last arrival %s" % np.array2string(st.last_arrival, precision=6))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
