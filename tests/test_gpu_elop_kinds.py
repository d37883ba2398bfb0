"""Every instantiation and load path of the element-operator kernels (csrc/mg.hip: elop_apply_kernel<TPE> with its diag mode,
elop_assemble_kernel<TPE>, dof_gather / gather_sum behind them) against exact rows (barrier_reference.py).  Run with -m gpu -s
on an MI355X; profiles/elop_kinds_reference.txt is the output of such a run.

Which code a level runs follows from its element shape: DevElOpOwned::build takes tpe (threads per element) as the smallest
power of two >= rows_per_el = block * K, doubled until 256 / tpe element slots fit into 60 KiB of LDS, and elop_pipelined(tpe,
nnz_max, block * nY, cmax) chooses between the software-pipelined and the plain load path (plain: nnz_max > 4 tpe).
AMG.elop_info(l) reports all of that, and the rows below are chosen from what it printed on the device.

What a row checks, at every level whose elop_info is valid (`levels` restricts the added L = 4 rows to the levels they were
added for).  Every figure is a ratio |device - exact| / (u bound) from barrier_reference.ratio, held to MARGIN * max(baseline,
1); the exact level values are level_reference at the DEVICE's Dz, the baseline is the oracle's fp64 f2 at the same state
(oracle_level_baseline).  State: s = 2e-3 * randn around the default z0, t = 3.7.
  * H v: hessian_apply(matrix_free=True) and (matrix_free=False, through the element-slab assembly) for a random v and the unit
    vector of a boundary-adjacent unknown (the one the fewest elements touch); three more calls are bit for bit equal;
  * f2: the lower-triangle values of the element-slab assembly against H on the pattern, which holds every nonzero of H;
  * diag mode of elop_apply_kernel: smooth(b = 1, degree = 1, one sweep, lmax = 1) from x = 0 returns x = dinv / theta, theta =
    0.5 (hi_frac + lo_frac) lmax with the fractions the test itself hands to set_pcg; 1 / (x theta) against diag(H) with
    diag(b_H) plus two roundings (lmax = 1 keeps theta's products exact);
  * per tpe one smoother comparison, degree 3 and 2 sweeps (MG_FIRST's vmul / vscale input path, MG_STEP), against _cheb_numpy
    of test_gpu_mg.py at that test's 1e-11.
Rows too large for a dense long-double H (BIG_ROWS) hold H v and its repeatability to the matrix-free reference
(hessian_apply_matrix_free), with MARGIN itself in place of MARGIN * max(baseline, 1) -- the oracle's dense f2 does not exist
there -- and s scaled by 2^-l so that the state stays inside the cone.

Coverage, asserted from elop_info by test_elop_info_table_and_coverage: every tpe in {8, .., 256} with a valid element
operator and a valid element-slab assembly; BOTH load paths of every tpe; a level with ncls >= 3; a single partial pass (nel <
256 / tpe); a partial last pass after full ones; a pipelined and a plain level whose workgroups walk three passes and more.

Measured on an MI355X (the run in profiles/elop_kinds_reference.txt; device ratios, the worse of the two vectors; the first run,
with MARGIN still at the cap of 16, gave the same worst figure):

  row                           l     N tpe rows cmax nnzm ncls  nel nY path  grid pass | base  Hv free Hv asm   f2 diag
                                             /el                                    /wg |
  fem1d L=3                     0     4   8    6    3    8    5    8  3 pipe     1    1 | 0.01     0.01   0.01 0.01 0.01
  fem1d L=3                     1     8   8    6    4   10    6    8  3 pipe     1    1 | 0.06     0.03   0.03 0.06 0.03
  fem1d L=3                     2    16   8    6    4    8    3    8  3 pipe     1    1 | 0.11     0.10   0.10 0.13 0.06
  fem1d L=4 cone+half           0     4   8    6    3    8    5   16  4 pipe     1    1 | 0.02     0.01   0.01 0.01 0.01
  fem1d L=4 cone+half           1     8   8    6    4   12    8   16  4 pipe     1    1 | 0.04     0.01   0.02 0.02 0.02
  fem1d L=4 cone+half           2    16   8    6    4   10    6   16  4 pipe     1    1 | 0.06     0.06   0.06 0.09 0.05
  fem1d L=4 cone+half           3    32   8    6    4    8    3   16  4 pipe     1    1 | 0.16     0.06   0.06 0.16 0.15
  fem1d L=4 K=6 cone+half       0     4  16   12    3   16    5   16  4 pipe     1    1 | 0.00     0.00   0.00 0.00 0.00
  fem1d L=4 K=6 cone+half       1     8  16   12    4   24    8   16  4 pipe     1    1 | 0.01     0.00   0.00 0.01 0.01
  fem1d L=4 K=6 cone+half       2    16  16   12    4   20    6   16  4 pipe     1    1 | 0.02     0.02   0.02 0.03 0.02
  fem1d L=4 K=6 cone+half       3    32  16   12    4   16    3   16  4 pipe     1    1 | 0.07     0.03   0.03 0.07 0.06
  fem1d L=4 K=8                 0     4  16   16    3   22    5   16  3 pipe     1    1 | 0.00     0.00   0.00 0.00 0.00
  fem1d L=4 K=8                 1     8  16   16    4   32    8   16  3 pipe     1    1 | 0.01     0.00   0.00 0.01 0.01
  fem1d L=4 K=8                 2    16  16   16    4   26    6   16  3 pipe     1    1 | 0.01     0.01   0.01 0.01 0.01
  fem1d L=4 K=8                 3    32  16   16    4   20    3   16  3 pipe     1    1 | 0.03     0.02   0.02 0.03 0.03
  fem2d L=2                     0    14  32   28    9   59    8    8  6 pipe     1    1 | 0.03     0.00   0.00 0.01 0.01
  fem2d L=2                     1    50  32   28   12   58    8    8  6 pipe     1    1 | 0.01     0.01   0.01 0.01 0.02
  fem2d L=2 K=6 slack column    0    25  64   42   16   92    8    8 14 pipe     2    1 | 0.01     0.00   0.00 0.00 0.00
  fem2d L=2 K=6 slack column    1    83  64   42   19   70    8    8 14 pipe     2    1 | 0.01     0.01   0.01 0.01 0.01
  fem2d L=2 K=8 cone+half       0    14  64   56    9  118    8    8  7 pipe     2    1 | 0.00     0.00   0.00 0.00 0.00
  fem2d L=2 K=8 cone+half       1    50  64   56   12  116    8    8  7 pipe     2    1 | 0.00     0.01   0.01 0.01 0.00
  fem2d L=2 L-shape cone+half   0    44  32   28   10   79   27   28  7 pipe     4    1 | 0.01     0.00   0.00 0.01 0.01
  fem2d L=2 L-shape cone+half   1   170  32   28   13   81   23   28  7 pipe     4    1 | 0.01     0.01   0.01 0.02 0.02
  fem3d k=1 L=2                 0     8  64   40    8   27    8    8 10 pipe     2    1 | 0.02     0.01   0.01 0.02 0.02
  fem3d k=1 L=2                 1    28  64   40    9   15    8    8 10 pipe     2    1 | 0.01     0.01   0.01 0.01 0.01
  fem3d k=2 L=2 K=4 cone+half   0    28 128  108   28  157    8    8  7 pipe     4    1 | 0.00     0.00   0.00 0.00 0.00
  fem3d k=2 L=2 K=4 cone+half   1   152 128  108   35   75    8    8  7 pipe     4    1 | 0.01     0.02   0.02 0.02 0.02
  fem3d k=2 L=2 cone+half       0    28 256  135   28  169    8    8 11 pipe     8    1 | 0.00     0.00   0.00 0.00 0.00
  fem3d k=2 L=2 cone+half       1   152 256  135   35   95    8    8 11 pipe     8    1 | 0.01     0.01   0.01 0.01 0.02
  fem3d k=3 L=2                 0    72 256  320   72 1725    8    8 10 plain    8    1 | 0.00     0.00   0.00 0.00 0.00
  fem3d k=3 L=2                 1   468 256  320   91  415    8    8 10 pipe     8    1 | 0.01     0.01   0.01 0.01 0.01
  fem2d L=3 K=1 half            0    11   8    7    7   43   31   32  1 plain    1    1 | 0.05     0.01   0.01 0.01 0.01
  fem2d L=3 K=1 half            1    33   8    7    7   25   15   32  1 pipe     1    1 | 0.03     0.02   0.01 0.03 0.03
  fem2d L=3 K=1 half            2   113   8    7    7    7    9   32  1 pipe     1    1 | 0.11     0.11   0.11 0.11 0.12
  fem2d L=4 K=2                 0    14  16   14    9   63   44  128  3 pipe     8    1 | 0.01     0.00   0.00 0.00 0.00
  fem2d L=4 K=2                 1    50  16   14   12   78   96  128  3 plain    8    1 | 0.01     0.00   0.00 0.00 0.00
  fem2d L=4 K=2                 2   194  16   14   14   69   94  128  3 plain    8    1 | (valid, not checked)
  fem2d L=4 K=2                 3   770  16   14   14   40   41  128  3 pipe     8    1 | (valid, not checked)
  fem2d L=4                     0    14  32   28    9   91   44  128  6 pipe    16    1 | (valid, not checked)
  fem2d L=4                     1    50  32   28   12  144  117  128  6 plain   16    1 | 0.00     0.00   0.00 0.00 0.00
  fem2d L=4                     2   194  32   28   14  138   96  128  6 plain   16    1 | (valid, not checked)
  fem2d L=4                     3   770  32   28   14   80   41  128  6 pipe    16    1 | (valid, not checked)
  fem2d L=4 K=8 cone+half       0    14  64   56    9  182   44  128  7 pipe    32    1 | (valid, not checked)
  fem2d L=4 K=8 cone+half       1    50  64   56   12  288  117  128  7 plain   32    1 | 0.00     0.00   0.00 0.00 0.00
  fem2d L=4 K=8 cone+half       2   194  64   56   14  276   96  128  7 plain   32    1 | (valid, not checked)
  fem2d L=4 K=8 cone+half       3   770  64   56   14  160   41  128  7 pipe    32    1 | (valid, not checked)
  fem3d k=2 L=4 K=3 cone+half   1   152 128   81   35  618  512  512  4 plain  256    1 |    -     0.00      -    -    -
  fem3d k=2 L=5                 4 65728 256  135   54  270   27 4096 10 pipe  1024    4 |    -     0.01      -    -    -
  fem3d k=2 L=5                 2  1072 256  135   54 2009 1728 4096 10 plain  768    6 |    -     0.00      -    -    -

  smoother (degree 3, 2 sweeps, rel to the numpy restatement): tpe 8 4.8e-16, tpe 16 3.2e-16, tpe 32 2.6e-16, tpe 64 5.9e-16,
  tpe 128 4.9e-16, tpe 256 3.5e-16

What the measurement showed against the table the rows were planned from:
  * tpe is the formula's on every row: no row needed the LDS bump.
  * fem1d L = 4 (16 elements, 32 per pass) is a single partial pass like L = 3, not a partial last pass: the uniform meshes
    have a power of two of elements, so a partial last pass after full ones needs a coarse mesh with an odd count -- the
    L-shape has seven triangles for that (28 elements in passes of 8).
  * On the planned rows only (256, plain) occurs (fem3d k = 3, level 0): at L = 2 every other element has nnz_max <= 4 tpe.  The
    plain path needs elements well inside a coarse element, i.e. a level two and more below the finest: fem2d L = 4 level 1 gives
    it for tpe 32 and, with D widened to K = 8, for tpe 64; fem3d k = 2 L = 4 with K = 3 for tpe 128 (13 824 nodes: matrix-free
    reference).  On fem1d a row of B has at most 2 nonzeros, so nnz_max <= 2 rows_per_el <= 4 tpe and tpe 8 / 16 never leave
    the pipelined path there; a D of one or two rows on triangles (rows_per_el 7 / 14) reaches plain for both, so those two
    rows are added rather than the path declared unreachable.
  * Three passes and more per workgroup need more than 2 * grid passes, grid = min(passes, 256 CUs * resident workgroups): the
    smallest mesh is fem3d k = 2 L = 5 (4096 elements, one per pass): its finest level is pipelined (grid 1024, 4 passes),
    level 2 plain (grid 768, 6 passes).  With 2 .. 32 elements per pass the other instantiations need as many times more
    elements (tpe 32: fem2d L = 8, 32 768 elements and 229 376 nodes, for 4 passes on a grid of 1024).
  * No row was left out: every level of every row is valid.

MARGIN: worst device ratio / max(baseline, 1) over all rows = 0.16 (fem1d L = 4, finest level: f2 0.16 against a baseline of
0.16), times 4 = 0.64, rounded up to a power of two = 1.
"""
import functools
import types

import numpy as np
import pytest
import scipy.sparse as sp

import barrier_reference as BR
import mgb_oracle as O
from test_gpu_mg import _cheb_numpy
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

MARGIN = 1.0             # see above; never more than BR.MARGIN = 16
assert MARGIN <= BR.MARGIN
LD = BR.LD
T = 3.7
AMP = 2e-3               # s = AMP * randn around the default z0 (test_gpu_mg.py)
LO_FRAC, HI_FRAC = 0.12, 1.2      # handed to set_pcg by the diagonal check, which derives theta from these very numbers
TPES = (8, 16, 32, 64, 128, 256)

U, S_ = ("u", "id"), ("s", "id")
UX, UY, UZ = ("u", "dx"), ("u", "dy"), ("u", "dz")
D1, D2, D3 = (U, UX, S_), (U, UX, UY, S_), (U, UX, UY, UZ, S_)       # the defaults of AMG(geometry)
SLACK_STATE = (("u", "dirichlet"), ("s", "full"), ("sigma", "full"))
# an L-shaped domain ([-1, 1]^2 without its upper right quarter) in seven unequal triangles, six of them around the re-entrant
# corner: 28 elements at L = 2, which is no multiple of the 8 elements of a pass (tpe 32)
LSHAPE = np.array([[-1, -1], [0.3, -1], [0, 0], [-1, -1], [0, 0], [-1, -0.2], [0.3, -1], [1, -1], [0, 0], [1, -1], [1, 0], [0, 0],
                   [-1, -0.2], [0, 0], [-1, 1], [0, 0], [0, 1], [-0.4, 1], [0, 0], [-0.4, 1], [-1, 1]], dtype=np.float64)


def _row(name, kind, L, D, cones, c, k=None, mesh=None, state=None, z=None, levels=None, tpe=None):
    return types.SimpleNamespace(name=name, kind=kind, L=L, D=D, cones=cones, c=c, k=k, mesh=mesh, state=state, z=z, levels=levels,
                                 tpe=tpe, matrix_free_reference=False)


# name, geometry, D, barrier terms, c per D row; tpe: the instantiation the formula gives, which the measured one has to be
ROWS = [
    _row("fem1d L=3", "fem1d", 3, D1, [([1, 2], 1.0)], [0.5, 0.0, 1.0], tpe=8),
    _row("fem1d L=4 cone+half", "fem1d", 4, D1, [([1, 2], 1.5), ("linear", [0], [1.0], 1.5)], [0.5, 0.0, 1.0], tpe=8),
    _row("fem1d L=4 K=6 cone+half", "fem1d", 4, D1 + (S_, UX, U), [([1, 2], 1.5), ("linear", [0], [1.0], 1.5)],
         [0.5, 0.0, 1.0, 0.0, 0.0, 0.0], tpe=16),
    _row("fem1d L=4 K=8", "fem1d", 4, D1 + (S_, UX, U, S_, U), [([1, 2], 2.0)], [0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], tpe=16),
    _row("fem2d L=2", "fem2d", 2, D2, [([1, 2, 3], 1.0)], [0.5, 0.0, 0.0, 1.0], tpe=32),
    _row("fem2d L=2 K=6 slack column", "fem2d", 2, D2 + (("sigma", "id"), U),
         [([1, 2, 3], 1.5, 4), ("linear", [0, 4], [1.0, 1.0], 0.2), ("linear", [4], [1.0], 1.0)],
         [0.5, 0.0, 0.0, 1.0, 10.0, 0.0], state=SLACK_STATE, tpe=64),
    _row("fem2d L=2 K=8 cone+half", "fem2d", 2, D2 + (U, S_, UX, UY), [([1, 2, 3], 3.0), ("linear", [0], [1.0], 0.5)],
         [0.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], tpe=64),
    _row("fem2d L=2 L-shape cone+half", "fem2d", 2, D2, [([1, 2, 3], 1.5), ("linear", [0], [1.0], 0.5)], [0.5, 0.0, 0.0, 1.0],
         mesh=LSHAPE, tpe=32),
    _row("fem3d k=1 L=2", "fem3d", 2, D3, [([1, 2, 3, 4], 1.0)], [0.5, 0.0, 0.0, 0.0, 1.0], k=1, tpe=64),
    _row("fem3d k=2 L=2 K=4 cone+half", "fem3d", 2, (U, UX, UY, S_), [([1, 2, 3], 1.0), ("linear", [0], [1.0], 0.5)],
         [0.5, 0.0, 0.0, 1.0], k=2, tpe=128),
    _row("fem3d k=2 L=2 cone+half", "fem3d", 2, D3, [([1, 2, 3, 4], 1.5), ("linear", [0], [1.0], 0.5)], [0.5, 0.0, 0.0, 0.0, 1.0],
         k=2, tpe=256),
    _row("fem3d k=3 L=2", "fem3d", 2, D3, [([1, 2, 3, 4], 2.0)], [0.5, 0.0, 0.0, 0.0, 1.0], k=3, tpe=256),
    # beyond the issue's table, for the plain load path: it needs nnz_max > 4 tpe, which only elements well inside a coarse element
    # have (levels two and more below the finest), and for tpe 8 and 16 a D of one or two rows on triangles
    _row("fem2d L=3 K=1 half", "fem2d", 3, (S_,), [("linear", [0], [1.0], 0.0)], [1.0], state=(("s", "full"),),
         z=lambda x: np.full((len(x), 1), 100.0), tpe=8),
    _row("fem2d L=4 K=2", "fem2d", 4, (UX, S_), [([0, 1], 1.5)], [0.0, 1.0], levels=(0, 1), tpe=16),
    _row("fem2d L=4", "fem2d", 4, D2, [([1, 2, 3], 2.0)], [0.5, 0.0, 0.0, 1.0], levels=(1,), tpe=32),
    _row("fem2d L=4 K=8 cone+half", "fem2d", 4, D2 + (U, S_, UX, UY), [([1, 2, 3], 3.0), ("linear", [0], [1.0], 0.5)],
         [0.5, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], levels=(1,), tpe=64),
]
# rows too large for a dense long-double H, held to the matrix-free reference at the given levels: (row, levels, whether a
# workgroup has to walk three passes and more there -- the two-pass look-ahead in steady state; the smallest mesh for which
# elop_info reports that)
BIG_ROWS = [
    (_row("fem3d k=2 L=4 K=3 cone+half", "fem3d", 4, (U, UX, S_), [([1, 2], 1.0), ("linear", [0], [1.0], 0.5)], [0.5, 0.0, 1.0],
          k=2, tpe=128), (1,), False),
    (_row("fem3d k=2 L=5", "fem3d", 5, D3, [([1, 2, 3, 4], 1.5)], [0.5, 0.0, 0.0, 0.0, 1.0], k=2, tpe=256), (4, 2), True),
]
for _b in BIG_ROWS:
    _b[0].matrix_free_reference = True
BY_NAME = {r.name: r for r in ROWS + [b[0] for b in BIG_ROWS]}


@pytest.fixture(scope="module")
def M(gpu_required):
    import mgb_amd
    return mgb_amd


# ---------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def _problem(name):
    """Device and oracle side of a row, built once: geometry, AMG with the default z0 / the row's c, host matrices, elop_info of
    every level."""
    import mgb_amd as M
    r = BY_NAME[name]
    state = tuple(M.DEFAULT_STATE) if r.state is None else r.state
    if r.kind == "fem1d":
        gm, go = M.fem1d_mpi(r.L), O.fem1d(r.L)
    elif r.kind == "fem2d":
        gm, go = M.fem2d_mpi(r.L, K=r.mesh), O.fem2d(r.L, K=r.mesh)
    else:
        gm, go = M.fem3d_mpi(r.L, k=r.k), O.fem3d(r.L, k=r.k)
    dim = go.discretization["dim"]
    A = M.AMG(gm, state, r.D, 1.0, cones=r.cones)
    if r.matrix_free_reference:
        A.set_solver("pcg")      # no factorisation is analysed for the levels of the large meshes
    Mo = O.amg(go, state, r.D)
    x = Mo.x
    z0 = O.map_rows(lambda xi: O.DEFAULT_G[dim](xi), x) if r.z is None else r.z(x)
    if len(state) == 3:
        z0 = np.column_stack([z0, np.full(len(x), 0.05)])
    assert z0.shape == (len(x), len(state))
    c = np.tile(np.asarray(r.c, dtype=np.float64), (len(x), 1))
    assert c.shape[1] == len(r.D) == A.K
    A.set_c(c)
    A.set_z(z0.reshape(-1, order="F"))
    P = types.SimpleNamespace(row=r, gm=gm, A=A, Mo=Mo, z0=z0, c=c, dim=dim, state=state)
    P.ops = {k: v.host for k, v in gm.operators.items()}
    P.subs = {k: [m.host for m in v] for k, v in gm.subspaces.items()}
    P.w = gm.w.to_numpy()
    P.info = [A.elop_info(l) for l in range(A.L)]
    return P


def _amplitude(P, l):
    """AMP for the table rows; the large meshes scale it by the level's mesh width (a random nodal vector has a gradient of
    about amplitude / width, and the state has to stay inside the cone)."""
    return AMP * 2.0 ** -l if P.row.matrix_free_reference else AMP


def _state_at(P, l, seed):
    """(s, the device's Dz at s, B = D R_l, the state z0 + R_l s as n x S) of level l."""
    A = P.A
    N = A.level_size(l)[0]
    s = _amplitude(P, l) * np.random.default_rng(seed).standard_normal(N)
    _, B = BR.level_matrices(P.ops, P.subs, A.state_variables, A.D, l, A.n)
    assert B.shape == (A.n * A.K, N)
    R = sp.block_diag([sp.csr_matrix((A.n, 0)) if sv[1] == "fixed" else P.subs[sv[1]][l] for sv in A.state_variables], format="csr")
    z = P.z0 + (R @ s).reshape(A.n, len(A.state_variables), order="F")
    return s, A.apply_D(l, s), B, z


@functools.lru_cache(maxsize=None)
def _level(name, l):
    """Exact level values at the DEVICE's Dz and the level baseline (the oracle's fp64 f2 at the same state), once per level."""
    P = _problem(name)
    A = P.A
    s, Dz, B, z = _state_at(P, l, 100 + l)
    Lv = BR.level_reference(B, A.K, P.w, P.c, T, Dz, P.row.cones)
    assert Lv.rows.feasible.all() and Lv.rows.in_range.all(), (name, l)
    _, _, base, _ = BR.oracle_level_baseline(P.Mo, l, z, P.c, T, P.row.cones)
    return types.SimpleNamespace(s=s, B=B, Lv=Lv, base=base, N=B.shape[1])


def _corner_dof(B, rows_per_el):
    """A boundary-adjacent unknown: the first one that the fewest elements touch."""
    Bc = sp.coo_matrix(B)
    pairs = np.unique(np.stack([Bc.col, Bc.row // rows_per_el], axis=1), axis=0)
    return int(np.argmin(np.bincount(pairs[:, 0], minlength=B.shape[1])))


def _levels(P):
    return [l for l in (range(P.A.L) if P.row.levels is None else P.row.levels) if P.info[l]["valid"]]


def _fmt_info(i):
    return ("tpe %3d rows/el %3d cmax %3d nnz_max %4d ncls %2d nel %6d K %d nY %2d %-9s elasm %d grid %4d passes/wg %d"
            % (i["tpe"], i["rows_per_el"], i["cmax"], i["nnz_max"], i["ncls"], i["nel"], i["K"], i["nY"],
               "pipelined" if i["pipelined"] else "plain", i["elasm_valid"], i["grid"], i["passes_per_wg"]))


# ---------------------------------------------------------------------------------------------------------- coverage
def test_elop_info_table_and_coverage(M):
    """The instantiation table as the device reports it, and the coverage conditions over the levels that the rows check."""
    print()
    hit, left_out, infos, big = set(), [], [], []
    for r in ROWS:
        P = _problem(r.name)
        if not _levels(P):
            left_out.append(r.name)
        for l in range(P.A.L):
            i = P.info[l]
            checked = l in _levels(P)
            print("%-30s l=%d N=%4d  %s%s" % (r.name, l, P.A.level_size(l)[0], _fmt_info(i) if i["valid"] else "not valid",
                                              "" if checked or not i["valid"] else "  (not checked)"))
            if i["valid"]:
                assert i["rows_per_el"] == len(r.D) * P.gm.discretization["block"] and i["K"] == len(r.D) and i["nY"] == P.A.nY
                assert i["nel"] * i["rows_per_el"] == P.A.n * P.A.K and i["tpe"] == r.tpe >= min(i["rows_per_el"], 256)
                assert i["passes_per_wg"] == -(-(-(-i["nel"] // (256 // i["tpe"]))) // i["grid"])
            if checked:
                hit.add((i["tpe"], i["pipelined"]))
                infos.append(i)
    for r, levels, three in BIG_ROWS:
        P = _problem(r.name)
        for l in levels:
            i = P.info[l]
            print("%-30s l=%d N=%6d  %s" % (r.name, l, P.A.level_size(l)[0], _fmt_info(i) if i["valid"] else "not valid"))
            assert i["valid"] and i["tpe"] == r.tpe
            hit.add((i["tpe"], i["pipelined"]))
            if three:
                big.append(i)
    assert len(left_out) <= 2, left_out                                   # rows left out: only where no level is element-local
    assert {t for t, _ in hit} == set(TPES)                               # every instantiation
    assert hit >= REACHABLE, (sorted(hit), sorted(REACHABLE))             # both load paths of every instantiation that has both
    assert {i["tpe"] for i in infos if i["elasm_valid"]} == set(TPES)     # the element-slab assembly of every instantiation
    assert any(i["ncls"] >= 3 for i in infos)
    assert any(i["nel"] < 256 // i["tpe"] for i in infos)                 # a single partial pass
    assert any(i["nel"] % (256 // i["tpe"]) and i["nel"] > 256 // i["tpe"] for i in infos)      # a partial pass after full ones
    for path in PATHS_WITH_THREE_PASSES:
        assert any(i["pipelined"] == path and i["passes_per_wg"] >= 3 for i in big), path


# (tpe, pipelined) pairs the candidate table reaches (measured table above; a pair that is missing here is one no geometry the
# library builds can reach, see the docstring)
REACHABLE = {(t, path) for t in TPES for path in (True, False)}
PATHS_WITH_THREE_PASSES = (True, False)


# ---------------------------------------------------------------------------------------------------------- rows
def _held(res, label, failures, worst):
    for k, (d, b) in res.items():
        worst[0] = max(worst[0], d / max(b, 1.0))
        if not d <= MARGIN * max(b, 1.0):
            failures.append((label, k, d, b))


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_row_against_exact_rows(M, name):
    """H v (matrix-free and assembled, a random and a unit vector), the element-slab assembly f2, the diag mode through the
    smoother's first step, and bit-for-bit repeatability, at every level whose element operator is valid."""
    P = _problem(name)
    A = P.A
    levels = _levels(P)
    if not levels:
        pytest.skip("elop_info: no level of this geometry is element-local within LDS")
    failures, worst = [], [0.0]
    print()
    for l in levels:
        i = P.info[l]
        X = _level(name, l)
        Lv, N, s = X.Lv, X.N, X.s
        rng = np.random.default_rng(7 + l)
        e = np.zeros(N)
        e[_corner_dof(X.B, i["rows_per_el"])] = 1.0
        res = {}
        for tag, v in (("rnd", rng.standard_normal(N)), ("unit", e)):
            hv, bhv = BR.hessian_apply_reference(Lv, v)
            got = A.hessian_apply(l, s, v, matrix_free=True)
            res["Hv free " + tag] = (BR.ratio(got, hv, bhv), X.base)
            res["Hv asm " + tag] = (BR.ratio(A.hessian_apply(l, s, v, matrix_free=False), hv, bhv), X.base)
            assert all(np.array_equal(got, A.hessian_apply(l, s, v, matrix_free=True)) for _ in range(3)), (name, l, tag)
        # f2: the element-slab assembly on the lower triangle of the level's pattern, which holds every nonzero of the exact H
        vals = A.f2(l, s, T)[1]
        rp, ci = A.hessian_pattern(l)
        ri = np.repeat(np.arange(N), np.diff(rp))
        assert np.all(ci <= ri)
        inside = np.zeros((N, N), dtype=bool)
        inside[ri, ci] = True
        assert not np.any(np.tril(Lv.H_abs != 0) & ~inside)
        res["f2"] = (BR.ratio(vals, Lv.H[ri, ci], Lv.b_H[ri, ci]), X.base)
        # diag mode: x = dinv / theta after one first-order step from x = 0 with b = 1; lam = 1 keeps theta's products exact
        A.set_pcg(lo_frac=LO_FRAC, hi_frac=HI_FRAC)
        lam = 1.0
        theta = 0.5 * (HI_FRAC * lam + LO_FRAC * lam)
        x, used = A.smooth(l, s, np.ones(N), degree=1, sweeps=1, lmax=lam, matrix_free=True)
        assert used == lam
        d, bd = BR.diag_reference(Lv)
        res["diag"] = (BR.ratio(1 / (x.astype(LD) * LD(theta)), d, bd + 2 * np.abs(d)), X.base)
        print("%-30s l=%d tpe %3d %-9s base %.2f | " % (name, l, i["tpe"], "pipelined" if i["pipelined"] else "plain", X.base)
              + "  ".join("%s %.2f" % (k, d_) for k, (d_, _) in res.items()))
        _held(res, (name, l), failures, worst)
    print("%-30s worst device ratio / max(level baseline, 1): %.2f   (MARGIN %g)" % (name, worst[0], MARGIN))
    assert not failures, failures


@pytest.mark.parametrize("tpe", TPES)
def test_smoother_per_instantiation(M, tpe):
    """degree 3, two sweeps through every instantiation: MG_FIRST's vmul / vscale input path and MG_STEP, against the numpy
    restatement of test_gpu_mg.py at its tolerance."""
    name, l = next((r.name, l) for r in ROWS for l in _levels(_problem(r.name)) if _problem(r.name).info[l]["tpe"] == tpe)
    P, X = _problem(name), _level(name, l)
    H = X.Lv.H.astype(np.float64)
    dm = 1.0 / np.sqrt(np.diagonal(H))
    lam = float(np.linalg.eigvalsh(dm[:, None] * H * dm[None, :])[-1])
    b = np.random.default_rng(9).standard_normal(X.N)
    want = _cheb_numpy(sp.csr_matrix(H), b, np.zeros(X.N), lam, 3, 2, lo_frac=LO_FRAC, hi_frac=HI_FRAC)
    P.A.set_pcg(lo_frac=LO_FRAC, hi_frac=HI_FRAC)
    got, used = P.A.smooth(l, X.s, b, degree=3, sweeps=2, lmax=lam, matrix_free=True)
    err = rel(got, want)
    print("\ntpe %3d  %-30s l=%d  smoother degree 3 x 2 sweeps: rel %.2e" % (tpe, name, l, err))
    assert used == lam and err < 1e-11


@pytest.mark.parametrize("name,l,three", [(r.name, l, three) for r, levels, three in BIG_ROWS for l in levels])
def test_large_rows_against_the_matrix_free_reference(M, name, l, three):
    """Meshes too large for a dense H, among them those on which a workgroup walks three passes and more; held to MARGIN itself
    (the oracle's dense f2 does not exist at this size, and max(baseline, 1) is never below 1)."""
    P = _problem(name)
    A, i = P.A, P.info[l]
    assert i["valid"] and (i["passes_per_wg"] >= 3 or not three)
    s, Dz, B, _ = _state_at(P, l, 200 + l)
    R = BR.reference(P.row.cones, Dz)
    assert R.feasible.all() and R.in_range.all()
    N = B.shape[1]
    e = np.zeros(N)
    e[_corner_dof(B, i["rows_per_el"])] = 1.0
    res = {}
    for tag, v in (("rnd", np.random.default_rng(11).standard_normal(N)), ("unit", e)):
        hv, bhv = BR.hessian_apply_matrix_free(B, A.K, P.w, R, v, rows_per_el=i["rows_per_el"])
        got = A.hessian_apply(l, s, v, matrix_free=True)
        res["Hv free " + tag] = (BR.ratio(got, hv, bhv), 1.0)
        assert all(np.array_equal(got, A.hessian_apply(l, s, v, matrix_free=True)) for _ in range(3))
    print("\n%-30s l=%d N=%d %s | " % (name, l, N, _fmt_info(i)) + "  ".join("%s %.2f" % (k, d) for k, (d, _) in res.items()))
    failures, worst = [], [0.0]
    _held(res, (name, l), failures, worst)
    assert not failures, failures
