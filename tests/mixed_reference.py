"""Independent numpy / math.fsum restatement of mixed boundary conditions, the yardstick of
test_mixed_host.py and test_gpu_mixed.py.  Not a test.

Column rule: subspaces[name][l] = the columns of subspaces["full"][l] without those that have a non-zero value in a pinned row of
the finest mesh; stored zeros do not count, kept columns keep their order, their bits and their stored zeros.  The pinned rows
are the rows of the selected boundary facets, found as tests/boundary_reference.py finds facets.
Loads: l_i = fsum(omega_fj h_fj over the selected facet nodes (f, j) at row i) / w_i on the distinct rows of the facet nodes in
ascending order; a row with no selected incidence carries 0.  The bar of a row is KTOL = 1e-12 (the bar of
test_boundary_host.py) times its own absolute sum  sum omega |h| / w.
Solves: O.amgb_core on the CPU oracle's geometry with u in the mixed space and the load added to the (u, id) column of the cost;
the parabolic loop of tests/parabolic_reference.py with the same two changes."""
import math

import numpy as np
import scipy.sparse as sp

import boundary_reference as BR
import mgb_oracle as O
import parabolic_reference as PR

KTOL = BR.KTOL
ZTOL = 1e-10      # the project's solve bar (tests/test_gpu_parity.py)


def pinned_rows(F, sel):
    """Sorted rows of the selected facets (sel: (nf,) bool)."""
    return np.unique(F["nodes"][np.asarray(sel, dtype=bool)].reshape(-1))


def column_rule(full, rows):
    """(kept columns of `full` as CSR with stored zeros as they were, indices of the dropped columns)."""
    A = sp.csr_matrix(full)
    hit = np.zeros(A.shape[1], dtype=bool)
    for r in rows:
        lo, hi = A.indptr[r], A.indptr[r + 1]
        hit[A.indices[lo:hi][A.data[lo:hi] != 0.0]] = True
    newcol = np.cumsum(~hit) - 1
    keep = ~hit[A.indices]
    row_of = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    out = sp.coo_matrix((A.data[keep], (row_of[keep], newcol[A.indices[keep]])), shape=(A.shape[0], int((~hit).sum()))).tocsr()
    return out, np.flatnonzero(hit)


def mixed_subspaces(geometry, sel, F=None):
    """One matrix per level for the selection sel of the facets of `geometry` (native library or oracle Geometry)."""
    F = BR.facets(geometry) if F is None else F
    rows = pinned_rows(F, sel)
    return [column_rule(getattr(S, "host", S), rows)[0] for S in geometry.subspaces["full"]]


def canonical(S):
    """(indptr, indices, data) after dropping stored zeros, rows sorted: equal patterns and bits compare equal."""
    S = sp.csr_matrix(getattr(S, "host", S)).copy()
    S.eliminate_zeros()
    S.sort_indices()
    return S.shape, S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data


def same_matrix(a, b):
    (sa, pa, ia, da), (sb, pb, ib, db) = canonical(a), canonical(b)
    return sa == sb and np.array_equal(pa, pb) and np.array_equal(ia, ib) and da.tobytes() == db.tobytes()


def incidence(F):
    """(rows (nb,), start (nb + 1,), idx): the row-sorted incidence table of the facet nodes."""
    nodes = F["nodes"].reshape(-1)
    order = np.lexsort((np.arange(nodes.size), nodes))
    rows, first = np.unique(nodes[order], return_index=True)
    return rows, np.concatenate([first, [nodes.size]]), order


def load(F, w, h, sel=None):
    """(rows, l (nb,), absolute sums (nb,)) of the field h (nf, q) on the facets sel (None: all); values of unselected facets
    are not read."""
    nf, q = F["nodes"].shape
    sel = np.ones(nf, dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    rows, start, idx = incidence(F)
    om, h = F["weights"].reshape(-1), np.asarray(h, dtype=float).reshape(-1)
    out, ab = np.zeros(len(rows)), np.zeros(len(rows))
    for r in range(len(rows)):
        inc = [fj for fj in idx[start[r]:start[r + 1]] if sel[fj // q]]
        if inc:
            out[r] = math.fsum(om[fj] * h[fj] for fj in inc) / w[rows[r]]
            ab[r] = math.fsum(om[fj] * abs(h[fj]) for fj in inc) / w[rows[r]]
    return rows, out, ab


def facet_values(F, x, h, t=None):
    """h(x) or h(t, x) at the facet nodes, (nf, q)."""
    xs = np.asarray(x, dtype=float).reshape(len(x), -1)[F["nodes"]]
    return np.array([[float(h(xi) if t is None else h(t, xi)) for xi in xf] for xf in xs])


def check_load(name, got, want, ab, tol=KTOL):
    gap = np.abs(np.asarray(got) - want)
    j = int((gap - tol * ab).argmax()) if len(want) else 0
    if len(want):
        print("%s: load off by %.3e at row %d (bar %.3e, value %.17g)" % (name, gap[j], j, tol * ab[j], want[j]))
    assert np.shape(got) == np.shape(want) and np.isfinite(got).all()
    assert (gap <= tol * ab).all(), np.argwhere(gap > tol * ab)


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ------------------------------------------------------------------------------------------------ solves through the oracle
def oracle_geometry(kind, L, k=None):
    return O.fem3d(L, k) if kind == "fem3d" else getattr(O, kind)(L)


def stationary(go, p, where, h=None, f=None, g=None, tol=None):
    """The mixed stationary solve on the oracle geometry `go`: Dirichlet g on the facets where(centre), the load of h (None, a
    callable h(x) or an (nf, q) array) on the others.  Returns dict(z (n, S), dirichlet_rows, its)."""
    dim = go.discretization["dim"]
    f = O.DEFAULT_F[dim] if f is None else f
    g = O.DEFAULT_G[dim] if g is None else g
    tol = math.sqrt(np.finfo(np.float64).eps) if tol is None else tol
    F = BR.facets(go)
    sel = np.array([bool(where(c)) for c in F["centre"]])
    go.subspaces["mixed_ref"] = mixed_subspaces(go, sel, F)
    try:
        M = O.amg(go, (("u", "mixed_ref"), ("s", "full")), None)
    finally:
        del go.subspaces["mixed_ref"]
    x = M.x
    z0 = O.map_rows(lambda xi: g(xi), x)
    c = O.map_rows(lambda xi: f(xi), x)
    if h is not None:
        hv = facet_values(F, x, h) if callable(h) else np.asarray(h, dtype=float)
        rows, l, _ = load(F, M.w, hv, ~sel)
        c[rows, 0] += l
    Q = O.convex_Euclidian_power(idx=list(range(1, dim + 2)), p=p)
    B = O.Barrier(Q)
    zvec = z0.reshape(-1, order="F")
    Dz = B.apply_D(M.D, zvec)
    if not np.all(np.isfinite(Q.F(x, Dz))):
        zvec, _ = O.amgb_phase1(go, M.state_variables, M.Dspec, Q, zvec, Dz, tol)
    SOL = O.amgb_core(B, M, zvec, c, tol)
    return dict(z=SOL["z"].reshape(z0.shape, order="F"), dirichlet_rows=pinned_rows(F, sel), its=int(SOL["its"].sum()), g=z0)


def parabolic(go, p, ts, where, h, f1=None, g=None, tol=None):
    """The loop of parabolic_reference.reference_loop with u in the mixed space and the load of h(t_{k+1}, x) on the facets not
    selected added to column 0 of the step's cost.  g(x) is static.  Returns (snapshots, lifts)."""
    dim = go.discretization["dim"]
    g = O.DEFAULT_G[dim] if g is None else g
    f1 = (lambda xi: 0.5) if f1 is None else f1
    tol = math.sqrt(np.finfo(np.float64).eps) if tol is None else tol
    F = BR.facets(go)
    sel = np.array([bool(where(c)) for c in F["centre"]])
    state, D, K, cones, ops = O.parabolic_problem(go, p)
    state = (("u", "mixed_ref"),) + tuple(state[1:])
    go.subspaces["mixed_ref"] = mixed_subspaces(go, sel, F)
    try:
        M = O.amg(go, state, D)
    finally:
        del go.subspaces["mixed_ref"]
    B = O.Barrier(O.ConeIntersection([O.convex_Euclidian_power(idx, pp) for idx, pp in cones]))
    x, n = M.x, M.x.shape[0]
    grad_ops = [go.operators[o] for o in ops]
    ts = np.asarray(ts, dtype=np.float64)
    z = O.parabolic_initial(go, p, g)
    fgrid = np.array([f1(xi) for xi in x], dtype=np.float64)
    u, lifts = [z.reshape(n, 3, order="F").copy()], np.zeros((len(ts) - 1, 2))
    for k in range(len(ts) - 1):
        rows, l, _ = load(F, M.w, facet_values(F, x, h, ts[k + 1]), ~sel)
        f = fgrid.copy()
        f[rows] += l
        c, z, _, lifts[k] = PR.step_transition(z, n, K, p, ts[k + 1] - ts[k], f, [], None, grad_ops)
        z = O.amgb_core(B, M, z, c, tol)["z"]
        u.append(z.reshape(n, 3, order="F").copy())
    return u, lifts


_CACHE = {}


def cached(key, fn):
    """fn() computed once per key and shared; callers must not modify the result."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]
