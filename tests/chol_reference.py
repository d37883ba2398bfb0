"""Reference solves for the checks of the device and host multifrontal Cholesky (test_gpu_chol_kinds.py,
test_chol_reference.py): plain numpy / scipy on the CPU.  A helper module, not a test module.

Matrices live on a level's lower-triangle pattern (rowptr, colidx), values in pattern order (what solve_linear takes):

  (a) random_spd: standard normal off the diagonal, each diagonal entry the row's absolute sum plus U(0.5, 2) -- SPD by
      Gershgorin, and random values catch index and permutation mistakes that the regular Hessian values can hide;
  (b) scaled: (a) scaled symmetrically by exp(U(-6, 6)) per unknown;
  (c), (d): the real Newton Hessians (taken on the GPU by the caller).

Every error is measured on the equilibrated system S = D^-1 H D^-1, y = D x with D = 2^round(log2 sqrt(diag H)) (powers
of two: the scaling is exact).  Cholesky is invariant to that scaling, partial-pivoting LU is not: without it, splu's
forward error on (b) is ~1000 times larger and would give the solver under test that much room.

  x_ref    splu of S (MMD_AT_PLUS_A) plus three steps of iterative refinement with the residual g - H x in long double
  baseline the same splu solve in plain fp64, no refinement: an independent fp64 direct solver, the yardstick for what
           fp64 arithmetic costs on this matrix
  eta      ||D^-1 (g - H x)||_inf / (||S||_inf ||D x||_inf + ||D^-1 g||_inf), residual in long double
  phi      ||D (x - x_ref)||_2 / ||D x_ref||_2

Bounds (Reference.metrics()): eta <= 16 max(eta_baseline, u) and phi <= 16 max(phi_baseline, u), u = 2^-53.  The device factor is as
backward stable as the baseline but adds in another order (rank-32 / 64 MFMA updates, per-slice fma chains in the
substitutions); a constant factor covers that, and the fp64 solvers measured sit within about 1 - 5 u of each other.  A
wrong or missing tile, extend-add entry or pivot block changes part of the factor by O(1) relative, which gives eta and
phi of 1e-10 or more, four orders of magnitude past the bound.  phi is checked only where the reference is exact: the
last refinement step changed D x by at most u ||D x_ref||_2."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from mesh_cases import MESHES

U = 2.0 ** -53
MARGIN = 16.0
LD = np.longdouble


# ---------------------------------------------------------------------------------------------------------- matrices
def full_matrix(rp, ci, lower, N):
    """The full symmetric CSR matrix from lower-triangle values in pattern order."""
    Lo = sp.csr_matrix((np.asarray(lower, dtype=np.float64), ci, rp), shape=(N, N))
    H = (Lo + sp.tril(Lo, -1).T).tocsr()
    H.sort_indices()
    return H


def _rows(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def random_spd(rp, ci, seed):
    """(a): lower-triangle values, SPD by Gershgorin (diagonal = absolute row sum of the FULL row + U(0.5, 2))."""
    rng = np.random.default_rng(seed)
    N = len(rp) - 1
    rows = _rows(rp)
    off = rows != ci
    v = np.zeros(len(ci))
    v[off] = rng.standard_normal(int(off.sum()))
    rowsum = np.bincount(rows[off], np.abs(v[off]), N) + np.bincount(ci[off], np.abs(v[off]), N)
    diag = rowsum + rng.uniform(0.5, 2.0, N)
    v[~off] = diag[rows[~off]]
    if np.count_nonzero(~off) != N:
        raise ValueError("pattern without a full diagonal")
    return v


def scaled(rp, ci, lower, seed):
    """(b): lower-triangle values scaled symmetrically by exp(U(-6, 6)) per unknown."""
    rng = np.random.default_rng(seed)
    d = np.exp(rng.uniform(-6.0, 6.0, len(rp) - 1))
    return lower * d[_rows(rp)] * d[ci]


def rhs(N, seed):
    """standard normal times exp(U(-3, 3))"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) * np.exp(rng.uniform(-3.0, 3.0))


def diagonal_positions(rp, ci):
    """index into the pattern-order values of every diagonal entry (row order)"""
    pos = np.flatnonzero(ci == _rows(rp))
    assert len(pos) == len(rp) - 1
    return pos


# ---------------------------------------------------------------------------------------------------------- reference
class Reference:
    """Equilibrated splu of one matrix; solve() gives the refined reference and the fp64 baseline for one right-hand
    side, metrics() the errors of any solution.  factor=False: eta() alone (no splu: the largest sizes)."""

    def __init__(self, rp, ci, lower, N, factor=True):
        self.N = N
        self.H = full_matrix(rp, ci, lower, N)
        diag = self.H.diagonal()
        if not np.all(diag > 0):
            raise ValueError("matrix has a non-positive diagonal entry")
        self.D = np.exp2(np.round(np.log2(np.sqrt(diag))))
        Di = 1.0 / self.D                                           # exact: powers of two
        S = sp.diags(Di) @ self.H @ sp.diags(Di)
        self.S_inf = float(abs(S).sum(axis=1).max())
        self.lu = spla.splu(S.tocsc(), permc_spec="MMD_AT_PLUS_A") if factor else None
        self._data = self.H.data.astype(LD)
        self._starts = self.H.indptr[:-1]

    def residual(self, x, g):
        """g - H x in long double, row by row over the CSR arrays"""
        xl = np.asarray(x).astype(LD)
        prod = self._data * xl[self.H.indices]
        return np.asarray(g).astype(LD) - np.add.reduceat(prod, self._starts)

    def solve(self, g):
        """dict: x_ref (long double), baseline (fp64), refine_eta (eta of x_ref), exact (last step <= u ||D x_ref||_2)"""
        D = self.D.astype(LD)
        base = self.lu.solve(g / self.D) / self.D
        x = base.astype(LD)
        last = np.inf
        for _ in range(3):
            r = self.residual(x, g)
            dy = self.lu.solve(np.asarray(r / D, dtype=np.float64))
            x = x + dy.astype(LD) / D
            last = float(np.linalg.norm(dy))
        dx = float(np.linalg.norm(np.asarray(D * x, dtype=np.float64)))
        return dict(x_ref=x, baseline=base, exact=last <= U * dx, refine_step=last / dx, refine_eta=self.eta(x, g))

    def eta(self, x, g):
        r = self.residual(x, g) / self.D.astype(LD)
        num = float(np.abs(r).max())
        den = self.S_inf * float(np.abs(np.asarray(x, dtype=LD) * self.D.astype(LD)).max()) + float(np.abs(g / self.D).max())
        return num / den

    def phi(self, x, x_ref):
        D = self.D.astype(LD)
        d = np.asarray((np.asarray(x).astype(LD) - x_ref) * D, dtype=np.float64)
        return float(np.linalg.norm(d) / np.linalg.norm(np.asarray(x_ref * D, dtype=np.float64)))

    def metrics(self, x, g, ref):
        """errors of x and of the baseline, their ratios to the bounds' scale, and whether each bound holds"""
        eb, pb = self.eta(ref["baseline"], g), self.phi(ref["baseline"], ref["x_ref"])
        e, p = self.eta(x, g), self.phi(x, ref["x_ref"])
        return dict(eta=e, phi=p, eta_base=eb, phi_base=pb, eta_ratio=e / max(eb, U), phi_ratio=p / max(pb, U),
                    exact=ref["exact"], eta_ok=e <= MARGIN * max(eb, U), phi_ok=p <= MARGIN * max(pb, U))


# ---------------------------------------------------------------------------------------------------------- the cases
# The 14 launch kinds of the device chain (Kind of csrc/chol_plan.hpp, the codes of mgb_amg_chol_schedule, AMG.CHOL_KINDS)
KINDS = ("Leaf", "Single", "SingleNarrow", "SingleDense", "SingleDenseNarrow", "Start", "Step", "Step2", "Panel2", "Update2",
         "BwdRect", "Bwd256", "Bwd1024", "BwdFused")

# knob settings (environment of a fresh process: the knobs are read once per process, MGB_LEAF on every analysis)
VARIANTS = {
    "default": {},
    "STEP2=0": {"MGB_CHOL_STEP2": "0"},
    "STEP2_TILES=0": {"MGB_CHOL_STEP2_TILES": "0"},
    "STEP2_TILES=0 WIDE=0": {"MGB_CHOL_STEP2_TILES": "0", "MGB_CHOL_WIDE": "0"},
    "DENSE_TILES=0": {"MGB_CHOL_DENSE_TILES": "0"},
    "START_PIVOT=0": {"MGB_CHOL_START_PIVOT": "0"},
    "GRAPH=0": {"MGB_CHOL_GRAPH": "0"},
    "LEAF=0 SINGLE=0": {"MGB_CHOL_LEAF": "0", "MGB_CHOL_SINGLE": "0"},
    "BWD_FUSED=0 SPLIT_NF=0": {"MGB_CHOL_BWD_FUSED": "0", "MGB_BWD_SPLIT_NF": "0"},
    "BWD_FUSED=0": {"MGB_CHOL_BWD_FUSED": "0"},
    "MGB_LEAF=8": {"MGB_LEAF": "8"},
    "MGB_LEAF=160": {"MGB_LEAF": "160"},
}
# these give bitwise the factor (and solution) of the default configuration
BITWISE = ("STEP2=0", "STEP2_TILES=0", "STEP2_TILES=0 WIDE=0", "DENSE_TILES=0", "START_PIVOT=0", "GRAPH=0")
# every environment variable that steers the factorisation; removed from a child's environment before its variant
KNOB_PREFIXES = ("MGB_CHOL_", "MGB_BWD_")
KNOB_NAMES = ("MGB_LEAF",)

_DEF_SMALL = ("Leaf", "Single", "SingleNarrow", "BwdFused")
_DEF_MID = _DEF_SMALL + ("Start", "Step2")
_G4_DEF = ("Start", "Step2", "Step", "Single", "Bwd256", "BwdRect", "Bwd1024", "BwdFused")      # fem2d L = 4 on graded4
_MID = {      # fem2d L = 6, 7: variant -> (kinds the schedule must contain, kinds it must not)
    "default": (_DEF_MID, ()),
    "STEP2=0": (("Step",), ("Step2",)),
    "STEP2_TILES=0": (("Panel2", "Update2"), ()),
    "STEP2_TILES=0 WIDE=0": (("Step",), ()),
    "DENSE_TILES=0": (("SingleDense", "SingleDenseNarrow"), ()),
    "START_PIVOT=0": (_DEF_MID, ()),
    "GRAPH=0": (_DEF_MID, ()),
    "LEAF=0 SINGLE=0": (("Start", "Step", "Step2", "Panel2", "Update2"), ()),
    "BWD_FUSED=0 SPLIT_NF=0": (("BwdRect", "Bwd256"), ()),
    "MGB_LEAF=8": (("Leaf", "SingleNarrow"), ()),
    "MGB_LEAF=160": (("Start", "Step", "Step2"), ()),
}
# (kind, L, mesh) -> variant -> (must contain, must not contain), in run order (default first: the bitwise yardstick); mesh: a
# name of mesh_cases.MESHES, None for the default interval, square and cube
CASES = {
    ("fem1d", 8, None): {"default": (("Leaf", "SingleNarrow", "BwdFused"), ()),
                   "DENSE_TILES=0": (("SingleDenseNarrow",), ()),
                   "LEAF=0 SINGLE=0": (("Start", "Step", "Step2"), ())},
    ("fem2d", 4, None): {"default": (_DEF_SMALL, ()),
                   "DENSE_TILES=0": (("SingleDense", "SingleDenseNarrow"), ())},
    ("fem2d", 6, None): dict(_MID),
    ("fem2d", 7, None): dict(_MID, **{"MGB_LEAF=8": (("Bwd256", "SingleDenseNarrow"), ("BwdFused",))}),
    ("fem3d", 2, None): {"default": (("Start", "Step2"), ()),
                   "STEP2_TILES=0": (("Panel2", "Update2"), ()),
                   "MGB_LEAF=8": (("Start",), ())},
    ("fem3d", 3, None): {"default": (("Start", "Step2"), ()),
                   "STEP2_TILES=0": (("Panel2", "Update2"), ()),
                   "MGB_LEAF=8": (("Start",), ())},
    # the trees of graded and L-shaped coarse meshes (mesh_cases): the kinds that the default meshes reach only at fem2d L = 8
    # or under forced knobs run here in the default schedule, at sizes where the refined reference is exact
    ("fem2d", 4, "graded4"): {          # N = 11 522, largest ns / nf 228 / 394; no Leaf launch
        "default": (_G4_DEF, ("Leaf",)),
        "STEP2=0": (("Step",), ("Step2",)),
        "STEP2_TILES=0": (("Panel2", "Update2"), ()),
        "DENSE_TILES=0": (("SingleDense",), ()),
        "LEAF=0 SINGLE=0": (("Start", "Step", "Step2"), ("Single", "Leaf")),
        "BWD_FUSED=0 SPLIT_NF=0": (("Bwd256", "BwdRect", "Bwd1024"), ("BwdFused",)),
        "BWD_FUSED=0": (("Bwd256", "BwdRect", "Bwd1024"), ("BwdFused",)),
        "MGB_LEAF=8": (("Leaf",) + _G4_DEF, ()),
        "MGB_LEAF=160": (("Panel2", "Update2"), ()),
        "GRAPH=0": (_G4_DEF, ("Leaf",)),
        "START_PIVOT=0": (_G4_DEF, ("Leaf",))},
    ("fem2d", 3, "graded4"): {          # N = 2 882, 112 / 197
        "default": (("Start", "Step2", "Step", "Single", "BwdFused"), ("Leaf",)),
        "MGB_LEAF=8": (("Leaf", "Start", "Step", "Step2", "Single", "BwdFused"), ())},
    ("fem2d", 4, "graded7"): {          # N = 18 434, 498 / 671: five Bwd1024 heights above the fused launch
        "default": (("Start", "Panel2", "Update2", "Single", "Step2", "Step", "Bwd1024", "BwdRect", "BwdFused"), ("Leaf",)),
        "STEP2_TILES=0": (("Panel2", "Update2"), ("Step2",))},
    ("fem2d", 5, "lshape"): {           # N = 9 218, 127 / 243
        "default": (("Leaf", "Single", "Start", "Step2", "Step", "BwdFused"), ()),
        "BWD_FUSED=0 SPLIT_NF=0": (("Bwd256", "BwdRect"), ("BwdFused",))},
    ("fem2d", 4, "two_squares"): {      # N = 1 540, 43 / 64: the root has no own column and two children, a Start launch
        "default": (("Leaf", "SingleNarrow", "Single", "Start", "BwdFused"), ())},
}
# the two largest sizes: matrix (a) alone, eta alone (no splu reference), eta <= 16 u
LARGE = {
    ("fem2d", 8, None): {"default": (("Panel2", "Update2", "SingleDense", "SingleDenseNarrow", "BwdRect", "Bwd1024", "BwdFused"), ()),
                   "BWD_FUSED=0": (("Panel2", "Update2", "SingleDense", "SingleDenseNarrow", "BwdRect", "Bwd1024", "Bwd256"),
                                   ("BwdFused",))},
    ("fem3d", 4, None): {"default": (("Panel2", "Update2", "Step2", "SingleDense", "BwdRect", "Bwd1024", "BwdFused"), ())},
}
# the workloads of CASES on coarse meshes of mesh_cases, main case first (test_chol_reference.py pins N and the largest ns / nf)
NEW_TREES = (("fem2d", 4, "graded4"), ("fem2d", 3, "graded4"), ("fem2d", 4, "graded7"), ("fem2d", 5, "lshape"),
             ("fem2d", 4, "two_squares"))
# replay with new values and pivot failures: (kind, L, mesh, variant)
REPLAY = (("fem2d", 6, None, "default"), ("fem2d", 6, None, "STEP2_TILES=0"), ("fem2d", 6, None, "DENSE_TILES=0"),
          ("fem3d", 3, None, "MGB_LEAF=8"), ("fem2d", 4, "graded4", "default"))
# the tree shapes at the tile edges, and where they occur (test_tree_shapes_cover_the_tile_edges): (kind, L, mesh, MGB_LEAF)
SHAPE_TREES = (("fem1d", 8, None, None), ("fem1d", 8, None, "160"), ("fem2d", 4, None, None), ("fem2d", 6, None, None),
               ("fem2d", 7, None, None), ("fem2d", 8, None, None), ("fem2d", 6, None, "8"), ("fem2d", 7, None, "8"),
               ("fem2d", 6, None, "160"), ("fem2d", 7, None, "160"), ("fem3d", 2, None, None), ("fem3d", 3, None, None),
               ("fem3d", 2, None, "8"), ("fem3d", 3, None, "8")) + tuple((k, L, m, None) for k, L, m in NEW_TREES)


def case_id(kind, L, mesh, *rest):
    """pytest id of a case: the default meshes keep the ids they had before the mesh name joined the key"""
    return "-".join([kind, str(L)] + ([] if mesh is None else [mesh]) + [str(r) for r in rest])


def child_env(base, variant):
    """base environment without any factorisation knob, plus the variant's"""
    e = {k: v for k, v in base.items() if not (k.startswith(KNOB_PREFIXES) or k in KNOB_NAMES)}
    e.update(VARIANTS[variant])
    return e


# ---------------------------------------------------------------------------------------------------------- host plans
def plan(kind, L, mesh=None):
    """(geometry handle, plan handle, dim, N, nnz) of the finest level of the default problem, host-only; mesh: a name of
    mesh_cases.MESHES (fem2d alone), None for the default mesh"""
    import mgb_amd as M
    from mgb_amd import _lib
    call, dptr, iptr, f64, i32 = _lib.call, _lib.dptr, _lib.iptr, _lib.f64, _lib.i32
    if mesh is not None and kind != "fem2d":
        raise ValueError("a coarse mesh needs fem2d")
    g = M.fem3d(L, 3) if kind == "fem3d" else (M.fem2d(L, MESHES[mesh]) if mesh is not None else getattr(M, kind)(L))
    dim = {"fem1d": 1, "fem2d": 2, "fem3d": 3}[kind]
    x = f64(np.asarray(g.x).reshape(np.asarray(g.x).shape[0], -1))
    Lv = len(g.refine)
    h = C.c_void_p()
    call("mgb_geo_create", x.shape[0], x.shape[1], Lv, 1, dptr(x), dptr(f64(g.w)), C.byref(h))
    for name, S in [("op:" + k, S) for k, S in g.operators.items()] + \
                   [("sub:%s:%d" % (k, l), S) for k, v in g.subspaces.items() for l, S in enumerate(v)]:
        S = sp.csr_matrix(S)
        S.sort_indices()
        call("mgb_geo_set_matrix", h, name.encode(), S.shape[0], S.shape[1], iptr(i32(S.indptr)), iptr(i32(S.indices)),
             dptr(f64(S.data)))
    state, D = M.DEFAULT_STATE, M.DEFAULT_D[dim]
    K = len(D)
    idx = list(range(K - dim - 1, K))
    iq = (C.c_int * (len(idx) - 1))(*idx[:-1])
    p = C.c_void_p()
    call("mgb_plan_create", h, len(state), _lib.str_array(state), K, _lib.str_array(D), len(idx) - 1, iq, idx[-1], Lv - 1,
         C.byref(p))
    N, nz, nT, nB = (C.c_int() for _ in range(4))
    call("mgb_plan_sizes", p, C.byref(N), C.byref(nz), C.byref(nT), C.byref(nB))
    return h, p, dim, N.value, nz.value


def plan_pattern(p, N, nz):
    from mgb_amd import _lib
    rp, ci = np.empty(N + 1, dtype=np.int32), np.empty(nz, dtype=np.int32)
    _lib.call("mgb_plan_pattern", p, _lib.iptr(rp), _lib.iptr(ci))
    return rp, ci


def plan_tree(p, dim):
    """(ns, nf, parent) of the plan's elimination tree in postorder (MGB_LEAF is read on every analysis)"""
    from mgb_amd import _lib
    nn = C.c_int()
    _lib.call("mgb_plan_chol_tree", p, dim, 0, C.byref(nn), None, None, None)
    ns, nf, par = (np.zeros(nn.value, dtype=np.int32) for _ in range(3))
    _lib.call("mgb_plan_chol_tree", p, dim, nn.value, C.byref(nn), _lib.iptr(ns), _lib.iptr(nf), _lib.iptr(par))
    return ns, nf, par


# CholKnobs (csrc/chol_plan.hpp) in field order: the environment variable and the default of each
KNOBS = (("MGB_CHOL_GRAPH", 1), ("MGB_CHOL_PROF", 0), ("MGB_CHOL_LEAF", 1), ("MGB_CHOL_SINGLE", 1), ("MGB_CHOL_STEP2", 1),
         ("MGB_CHOL_WIDE", 1), ("MGB_CHOL_START_PIVOT", 1), ("MGB_CHOL_STEP2_TILES", 224), ("MGB_CHOL_DENSE_TILES", 512),
         ("MGB_BWD_SPLIT_NF", 192), ("MGB_CHOL_BWD_FUSED", 1), ("MGB_CHOL_BWD_CUT", 2), ("MGB_CHOL_BWD_FUSED_NF", 384),
         ("MGB_CHOL_BWD_FUSED_THREADS", 512), ("MGB_CHOL_PREMAP", 1), ("MGB_CHOL_PREMAP_TILES", 400))


def variant_knobs(variant):
    """the variant's knob values as {environment variable: int}, defaults filled in (MGB_LEAF is not a chain knob)"""
    return {name: int(VARIANTS[variant].get(name, dflt)) for name, dflt in KNOBS}


def plan_schedule(p, dim, knobs=None, world=1, rank=0):
    """The host plan of the device chain (mgb_plan_chol_schedule).  knobs: None (the values this process reads from the
    environment) or a dict as variant_knobs() gives.  Per launch: kind (name), ofs, cnt, block, lds, p, npiv, rect,
    consumer, producers; the job arrays; own_bwd / top_fwd; world (what the tree was split over)."""
    from mgb_amd import _lib
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    kn = None if knobs is None else np.array([knobs[name] for name, _ in KNOBS], dtype=np.int32)
    info = np.zeros(10, dtype=np.int32)
    head = (p, dim, None if kn is None else ip(kn), world, rank, ip(info))
    _lib.call("mgb_plan_chol_schedule", *head, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None)
    nl, own_bwd, top_fwd, nlists, nstarts, ntiles, nsingles, nrects, nasm, split = (int(v) for v in info)
    launch = np.zeros((nl, 10), dtype=np.int32)
    lists, apos, asrc = np.zeros(nlists, dtype=np.int32), np.zeros(nasm, dtype=np.int32), np.zeros(nasm, dtype=np.int32)
    starts, tiles = np.zeros((nstarts, 5), dtype=np.int32), np.zeros((ntiles, 3), dtype=np.int32)
    singles, rects = np.zeros((nsingles, 3), dtype=np.int32), np.zeros((nrects, 2), dtype=np.int32)
    _lib.call("mgb_plan_chol_schedule", *head, nl, ip(launch), nlists, ip(lists), nstarts, ip(starts), ntiles, ip(tiles), nsingles,
              ip(singles), nrects, ip(rects), nasm, ip(apos), ip(asrc))
    names = ("ofs", "cnt", "block", "lds", "p", "npiv", "rect", "consumer", "producers")
    out = {n: launch[:, i + 1] for i, n in enumerate(names)}
    out.update(kinds=[KINDS[k] for k in launch[:, 0]], own_bwd=own_bwd, top_fwd=top_fwd, lists=lists, starts=starts, tiles=tiles,
               singles=singles, rects=rects, apos=apos, asrc=asrc, world=split)
    return out


def free_plan(h, p):
    from mgb_amd import _lib
    _lib.call("mgb_plan_destroy", p)
    _lib.call("mgb_geo_destroy", h)
