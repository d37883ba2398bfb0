"""The fused backward sweep of the device Cholesky (backward_fused_kernel) against the per-height launches it replaces:
bit for bit.  One linear solve on the finest level through solve_linear(..., solver="gpu") per schedule; the knobs are
read once per process, so every schedule runs in a fresh child process under its own timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import mgb_amd as M
kind, L, out = sys.argv[2], int(sys.argv[3]), sys.argv[4]
geo = getattr(M, kind + "_mpi")(L)
A = M.AMG(geo, p=1.0)
dim = {"fem1d": 1, "fem2d": 2, "fem3d": 3}[kind]
x = geo.x.to_numpy()
A.set_c(np.vstack([M.DEFAULT_F[dim](xi) for xi in x]))
A.set_z(np.vstack([M.DEFAULT_G[dim](xi) for xi in x]).reshape(-1, order="F"))
l = A.L - 1
N = A.level_size(l)[0]
H, lower = A.f2(l, np.zeros(N), 1.0)
g = A.f1(l, np.zeros(N), 1.0)
xg = A.solve_linear(l, lower, g, solver="gpu")
xg2 = A.solve_linear(l, lower, g, solver="gpu")
xh = A.solve_linear(l, lower, g, solver="host") if len(sys.argv) > 5 else np.zeros(0)
np.savez(out, xg=xg, xg2=xg2, xh=xh, res=np.linalg.norm(H @ xg - g) / np.linalg.norm(g))
"""

# schedule variants: environment on top of the default (fused, cut 2, fronts up to 384, 512 threads)
VARIANTS = {
    "old": {"MGB_CHOL_BWD_FUSED": "0"},
    "fused": {"MGB_CHOL_BWD_FUSED": "1"},
    "cut4": {"MGB_CHOL_BWD_FUSED": "1", "MGB_CHOL_BWD_CUT": "4"},
    "cut1_256": {"MGB_CHOL_BWD_FUSED": "1", "MGB_CHOL_BWD_CUT": "1", "MGB_CHOL_BWD_FUSED_THREADS": "256"},
}
# h_top below the root: the per-height launches above it, the fused launch below (mixed schedule).  The threshold sits between
# the largest fronts of two neighbouring heights of that tree (tools/tree_stats.py); the fem1d trees have their largest
# fronts at the leaves, so no threshold splits them.
MIXED = {("fem2d", 4): "44", ("fem2d", 5): "80", ("fem2d", 6): "150", ("fem2d", 7): "150", ("fem3d", 3): "200"}


def _solve(tmp_path, kind, L, name, env, host=False):
    out = str(tmp_path / ("%s_%d_%s.npz" % (kind, L, name)))
    e = dict(os.environ)
    for k in ("MGB_CHOL_BWD_FUSED", "MGB_CHOL_BWD_CUT", "MGB_CHOL_BWD_FUSED_NF", "MGB_CHOL_BWD_FUSED_THREADS", "MGB_CHOL_PROF"):
        e.pop(k, None)
    e.update(env)
    cmd = [sys.executable, "-c", CHILD, ROOT, kind, str(L), out] + (["host"] if host else [])
    r = subprocess.run(cmd, env=e, timeout=240, capture_output=True, text=True)
    assert r.returncode == 0, "%s %s: exit %d\n%s" % (name, env, r.returncode, r.stderr[-2000:])
    return np.load(out)


@pytest.mark.parametrize("kind,L", [("fem1d", 8), ("fem2d", 4), ("fem2d", 5), ("fem2d", 6), ("fem2d", 7), ("fem3d", 3)])
def test_fused_backward_sweep_is_bitwise_the_per_height_sweep(gpu_required, tmp_path, kind, L):
    ref = _solve(tmp_path, kind, L, "old", VARIANTS["old"], host=True)
    xo, xh = ref["xg"], ref["xh"]
    assert np.all(np.isfinite(xo)) and np.array_equal(xo, ref["xg2"])
    # the tolerance of test_device_cholesky_matches_host_on_large_level
    assert np.linalg.norm(xo - xh) / np.linalg.norm(xh) < 1e-10
    variants = dict(VARIANTS)
    del variants["old"]
    if (kind, L) in MIXED:
        variants["mixed"] = {"MGB_CHOL_BWD_FUSED": "1", "MGB_CHOL_BWD_FUSED_NF": MIXED[(kind, L)]}
        variants["mixed_cut2"] = {"MGB_CHOL_BWD_FUSED": "1", "MGB_CHOL_BWD_FUSED_NF": MIXED[(kind, L)], "MGB_CHOL_BWD_CUT": "2"}
    for name, env in variants.items():
        got = _solve(tmp_path, kind, L, name, env)
        x = got["xg"]
        print("%s L=%d %-10s max |x - x_old| = %.3e  residual %.3e" % (kind, L, name, np.abs(x - xo).max(), float(got["res"])))
        assert np.array_equal(x, got["xg2"]), name
        assert np.array_equal(x, xo), name
        assert np.linalg.norm(x - xh) / np.linalg.norm(xh) < 1e-10, name


def test_fused_backward_sweep_reproduces_the_1024_thread_heights(gpu_required, tmp_path):
    """fem2d L=8 without a front-size limit: the fused launch then also takes the heights whose fronts (up to 765) ran
    backward_kernel<1024>, with its slice counts 16 / 8 / 5 / 4 / 3 / 2 in the panel updates."""
    xo = _solve(tmp_path, "fem2d", 8, "old", VARIANTS["old"])["xg"]
    assert np.all(np.isfinite(xo))
    for name, env in {"nolimit": {"MGB_CHOL_BWD_FUSED_NF": "0"}, "default": {}}.items():
        x = _solve(tmp_path, "fem2d", 8, name, env)["xg"]
        print("fem2d L=8 %-8s max |x - x_old| = %.3e" % (name, np.abs(x - xo).max()))
        assert np.array_equal(x, xo), name
