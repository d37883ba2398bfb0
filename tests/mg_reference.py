"""Exact restatement of the V-cycle and of the preconditioned CG of solver="pcg" (csrc/amg_mg.cpp, csrc/mg.hip) for
test_gpu_vcycle.py and test_mg_reference.py: plain numpy on the CPU, generic over the dtype (float64 and np.longdouble).
A helper module, not a test module.

Inputs, all from the oracle (nothing from the library under test but P_l, which test_gpu_mg.py already holds to
R_{l+1} P_l = R_l, and which `nodal_prolongation` restates here for the CPU tests):

  H_l   the oracle's f2 on R_l at the top-level point z0 + R_top s: R_l' (sum_jk D_j' diag(w y_jk) D_k) R_l, the Galerkin
        operators P_l' H_{l+1} P_l of one another because the levels are nested
  lam_l lambda_max(D^-1 H_l) from scipy's eigsh (handed to the device through AMG.pin_lmax: the device's own warm-started
        estimate differs from call to call, and the V-cycle moves by about 0.4 delta for a relative change delta of it)

  cheb    one Chebyshev-Jacobi sweep (Saad, Iterative Methods, Alg. 12.1) on [lo_frac, hi_frac] * lam
  Vcycle  x = cheb(0); r = b - H x; x += P Vcycle(P' r); x = cheb(x); an exact solve on the coarsest level c0, the largest
          level with 0 < N <= 128 unknowns (level 0 where there is none: the coarse meshes of mesh_cases.py, where the
          device's coarse solve is its sparse Cholesky and the dense factor here restates that too)
  pcg     the textbook recurrence with the stop rule of pcg_dot_kernel, every iterate kept

The long-double run of the same code is the reference; its distance to the float64 run is what rounding alone does to
the recurrence in another order of summation, and the tolerances of test_gpu_vcycle.py are multiples of that distance
(profiles/vcycle_reference.txt lists them)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mgb_oracle as O
from mesh_cases import MESHES

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "mg_reference needs an extended-precision long double (x87); there is no fallback"

DENSE_MAX = 128                  # kDenseMax of csrc/mg.hpp: the largest coarsest level
LO_FRAC, HI_FRAC = 0.12, 1.2     # PcgOptions defaults (csrc/amg.hpp), the fractions test_gpu_mg.py uses too
T = 10.0                         # the barrier parameter of every Newton system here (test_gpu_mg.py: t = 10)
S_SCALE = 1e-3                   # s = S_SCALE * randn
SEED = 4                         # of s
B_SEED, U_SEED = 7, 8            # of the vectors b (= g of the operator tests) and u that V is applied to

# (kind, L): levels c0 .. top = L - 1 and why
SHAPES = (("fem2d", 4),      # 1 .. 3: N = 50, 194, 770, one intermediate level
          ("fem2d", 5),      # 1 .. 4: N = 50, 194, 770, 3074, two intermediate levels
          ("fem3d", 3),      # 0 .. 2: N = 72, 468, 3528
          ("fem1d", 7),      # 5 .. 6: N = 128, 256: the largest dense inverse
          ("fem1d", 6),      # 5 .. 5: N = 128, top == c0
          ("fem2d", 2),      # 1 .. 1: N = 50, top == c0
          # coarse meshes of mesh_cases (a case then carries the mesh name: (kind, L, p, mesh)), p = 1 and 1.5
          ("fem2d", 3, "graded4"),      # 0 .. 2: N = 182, 722, 2882: no level has N <= 128, so c0 = 0 and the coarse solve is
                                        # the device Cholesky (mg_prepare), not the dense inverse
          ("fem2d", 4, "lshape"))       # 0 .. 3: N = 38, 146, 578, 2306: the dense inverse under an irregular hierarchy
CASES = tuple((k, L, p) for k, L in SHAPES[:6] for p in ((1.0, 1.5, 2.0) if k == "fem2d" else (1.0, 1.5))) + \
    tuple((k, L, p, m) for k, L, m in SHAPES[6:] for p in (1.0, 1.5))
# test 5 (iteration count at rtol = 1e-11): (kind, L, p, degree) -> seed of `count_rhs`.  The seed is chosen on the long-double
# restatement so that <r, V r> / (rtol^2 <r0, V r0>) is above 4 at the last iteration but one and below 0.25 at the last: rounding
# cannot move the count then.  Convergence per iteration is about a factor 8 in <r, V r> at degree 1 on the 2-D and 3-D
# hierarchies, so no right-hand side of 270 tried there leaves that factor 16 at the stop (the best: 3.0 and 0.35); degree 1 is
# counted on the two-level fem1d hierarchy, where one does.
COUNT_CASES = {("fem2d", 4, 1.0, 2): 233, ("fem2d", 4, 1.0, 3): 0, ("fem2d", 4, 1.5, 2): 108, ("fem2d", 4, 1.5, 3): 2,
               ("fem3d", 3, 1.0, 2): 217, ("fem3d", 3, 1.0, 3): 0, ("fem1d", 7, 1.0, 1): 40, ("fem1d", 7, 1.5, 1): 198}
COUNT_RTOL = 1e-11
FLOOR, FACTOR = 1e-11, 100.0     # bound of a device result = max(FLOOR, FACTOR * |float64 run - long-double run|)
MULTI = tuple(c for c in CASES if c[:2] not in (("fem1d", 6), ("fem2d", 2)))
COARSE = tuple(c for c in CASES if c[:2] in (("fem1d", 6), ("fem2d", 2)))


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    d = np.asarray(a, dtype=LD) - np.asarray(b, dtype=LD)
    return float(np.sqrt(d @ d) / max(np.sqrt(np.asarray(b, dtype=LD) @ np.asarray(b, dtype=LD)), LD(1e-300)))


# ------------------------------------------------------------------------------------------------ linear algebra in any dtype
class Mat:
    """CSR matrix with values in `dtype` (scipy has no long-double kernels): products by one gather and one segmented sum."""

    def __init__(self, A, dtype):
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.shape, self.dtype = A.shape, dtype
        self.rp, self.ci, self.v = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(dtype)
        self._rows = np.flatnonzero(self.rp[:-1] < self.rp[1:])
        self._src = A
        self._T = None

    def __matmul__(self, x):
        out = np.zeros(self.shape[0], dtype=self.dtype)
        if len(self.v):
            out[self._rows] = np.add.reduceat(self.v * x[self.ci], self.rp[:-1][self._rows])
        return out

    @property
    def T(self):
        if self._T is None:
            self._T = Mat(self._src.T.tocsr(), self.dtype)
        return self._T

    def diagonal(self):
        return self._src.diagonal().astype(self.dtype)

    def dense(self):
        return self._src.toarray().astype(self.dtype)


def cholesky(A):
    """Lower Cholesky factor of a dense SPD matrix in its own dtype; LinAlgError if a pivot is not positive."""
    A = np.array(A, copy=True)
    n = A.shape[0]
    for k in range(n):
        d = A[k, k]
        if not (d > 0) or not np.isfinite(d):
            raise np.linalg.LinAlgError("matrix is not positive definite (pivot %d)" % k)
        A[k, k] = np.sqrt(d)
        A[k + 1:, k] /= A[k, k]
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
    return np.tril(A)


def chol_solve(Lc, b):
    """x = (Lc Lc')^-1 b, b a vector or a matrix of columns."""
    x = np.array(b, dtype=Lc.dtype, copy=True)
    n = Lc.shape[0]
    for k in range(n):
        x[k] = x[k] / Lc[k, k]
        x[k + 1:] -= np.multiply.outer(Lc[k + 1:, k], x[k]) if x.ndim > 1 else Lc[k + 1:, k] * x[k]
    for k in range(n - 1, -1, -1):
        x[k] = x[k] / Lc[k, k]
        x[:k] -= np.multiply.outer(Lc[k, :k], x[k]) if x.ndim > 1 else Lc[k, :k] * x[k]
    return x


# ------------------------------------------------------------------------------------------------ the recurrences
def cheb(H, b, x, lam, degree, lo_frac=LO_FRAC, hi_frac=HI_FRAC):
    """One sweep of `degree` applications of H from x: the recurrence of test_gpu_mg._cheb_numpy in the dtype of b."""
    dt = b.dtype.type
    dinv = dt(1) / H.diagonal()
    hi, lo = dt(hi_frac) * dt(lam), dt(lo_frac) * dt(lam)
    theta, delta = dt(0.5) * (hi + lo), dt(0.5) * (hi - lo)
    sigma = theta / delta
    r = b - H @ x
    rho = dt(1) / sigma
    d = dinv * r / theta
    for _ in range(1, degree):
        x = x + d
        r = r - H @ d
        rn = dt(1) / (dt(2) * sigma - rho)
        d = rn * rho * d + (dt(2) * rn / delta) * (dinv * r)
        rho = rn
    return x + d


class Vcycle:
    """x = V(b) on the levels c0 .. top.  H, P, lam: dicts by level of scipy matrices (P[l]: level l -> l + 1) and floats."""

    def __init__(self, H, P, lam, c0, top, degree, dtype, lo_frac=LO_FRAC, hi_frac=HI_FRAC):
        self.c0, self.top, self.degree, self.dtype, self.fr = c0, top, degree, dtype, (lo_frac, hi_frac)
        self.H = {l: Mat(H[l], dtype) for l in range(c0, top + 1)}
        self.P = {l: Mat(P[l], dtype) for l in range(c0, top)}
        self.lam = dict(lam)
        self.Lc = cholesky(self.H[c0].dense())

    def __call__(self, b, l=None):
        l = self.top if l is None else l
        b = np.asarray(b, dtype=self.dtype)
        if l == self.c0:
            return chol_solve(self.Lc, b)
        H, P = self.H[l], self.P[l - 1]
        x = cheb(H, b, np.zeros_like(b), self.lam[l], self.degree, *self.fr)
        r = b - H @ x
        x = x + P @ self(P.T @ r, l - 1)
        return cheb(H, b, x, self.lam[l], self.degree, *self.fr)


class PcgResult:
    """x[k]: iterate k (x[0] = 0); alpha[k], beta[k]: of iteration k + 1; rz[k] = <r_k, V r_k>; code: 1 converged, 2 breakdown,
    3 iteration cap (the codes of pcg_dot_kernel)."""

    def __init__(self):
        self.x, self.alpha, self.beta, self.rz, self.it, self.code = [], [], [], [], 0, 0

    def relres(self, k=None):
        k = self.it if k is None else k
        return float(np.sqrt(abs(self.rz[k]) / self.rz[0])) if self.rz[0] > 0 else 0.0


def pcg(H, V, g, rtol, maxit):
    """CG on H x = g preconditioned by V, from x = 0.  Stop rule of pcg_dot_kernel after iteration `it` >= 1: a negative or
    non-finite <r, z> is code 2; then <r, z> <= rtol^2 <r0, z0> is code 1; then it >= maxit is code 3.  At iteration 0 a zero
    <r0, z0> is code 1 (zero right-hand side: x = 0 solves it), a negative or non-finite one code 2.  <p, H p> <= 0 is code 2."""
    dt = g.dtype.type
    out = PcgResult()
    x, r = np.zeros_like(g), g.copy()
    z = V(r)
    rz = r @ z
    out.x.append(x.copy())
    out.rz.append(rz)
    if not (rz > 0) or not np.isfinite(rz):
        out.code = 1 if rz == 0 else 2
        return out
    p = z.copy()
    tol2 = dt(rtol) * dt(rtol)
    while True:
        Ap = H @ p
        pap = p @ Ap
        if not (pap > 0) or not np.isfinite(pap):
            out.code = 2
            return out
        alpha = rz / pap
        x = x + alpha * p
        r = r - alpha * Ap
        z = V(r)
        rzn = r @ z
        out.it += 1
        beta = rzn / rz
        out.x.append(x.copy())
        out.alpha.append(alpha)
        out.beta.append(beta)
        out.rz.append(rzn)
        if not np.isfinite(rzn) or rzn < 0:
            out.code = 2
        elif rzn <= tol2 * out.rz[0]:
            out.code = 1
        elif out.it >= maxit:
            out.code = 3
        if out.code:
            return out
        rz = rzn
        p = z + beta * p


# ------------------------------------------------------------------------------------------------ the systems, from the oracle
def coarsest(sizes, top):
    """Amg::mg_coarsest: the largest level <= top with 0 < N <= 128 (level 0, or the first non-empty one, if there is none; the
    device then solves that level with its sparse Cholesky, the restatement with the same dense factor as ever)."""
    c0 = 0
    for l in range(top + 1):
        if 0 < sizes[l] <= DENSE_MAX:
            c0 = l
    while c0 < top and sizes[c0] == 0:
        c0 += 1
    return c0


def nodal_prolongation(Rf, Rc):
    """P with Rf P = Rc for nested nodal levels: row i of P is the row of Rc at a finest-mesh node that carries unknown i of
    the finer level alone (csrc/amg_mg.cpp build_prolongation, restated)."""
    Rf, Rc = sp.csr_matrix(Rf), sp.csr_matrix(Rc)
    Rf.eliminate_zeros()
    single = np.flatnonzero(np.diff(Rf.indptr) == 1)
    single = single[np.abs(Rf.data[Rf.indptr[single]] - 1.0) < 1e-12]
    cols = Rf.indices[Rf.indptr[single]]
    rep = np.full(Rf.shape[1], -1)
    rep[cols[::-1]] = single[::-1]      # the first such node of each unknown
    assert (rep >= 0).all(), "the level hierarchy is not nodal"
    P = Rc[rep].tocsr()
    assert abs(Rf @ P - Rc).max() < 1e-12
    return P


def lambda_max(H):
    """lambda_max(D^-1 H) of an SPD matrix through the symmetric D^-1/2 H D^-1/2."""
    H = sp.csr_matrix(H)
    s = sp.diags(H.diagonal() ** -0.5)
    return float(spla.eigsh(s @ H @ s, k=1, which="LA", return_eigenvectors=False, v0=np.ones(H.shape[0]), tol=1e-13)[0])


class System:
    """One Newton system of the oracle in the oracle's numbering: levels c0 .. top = L - 1, s = S_SCALE randn(seed), the
    Hessians H_l at z0 + R_top s with t = T, the gradient g of the top level, lam_l and the transfers P_l."""

    def __init__(self, kind, L, p, mesh=None, seed=SEED):
        self.kind, self.L, self.p, self.top, self.mesh = kind, L, p, L - 1, mesh
        go = getattr(O, kind)(L) if mesh is None else O.fem2d(L, MESHES[mesh])
        dim = go.discretization["dim"]
        self.Mo = Mo = O.amg(go)
        self.z0 = z0 = O.map_rows(lambda xi: O.DEFAULT_G[dim](xi), Mo.x).reshape(-1, order="F")
        self.c = c = O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), Mo.x)
        self.B = B = O.Barrier(O.convex_Euclidian_power(list(range(1, dim + 2)), p))
        self.sizes = [R.shape[1] for R in Mo.R]
        self.c0 = coarsest(self.sizes, self.top)
        self.N = self.sizes[self.top]
        self.s = S_SCALE * np.random.default_rng(seed).standard_normal(self.N)
        z = z0 + Mo.R[self.top] @ self.s
        # the guard of every case: strictly inside the cone, and the top Hessian positive definite
        Dz = B.apply_D(Mo.D, z)
        self.inside = bool(np.all(B.Q.phi(Dz) > 0) and np.all(Dz[:, -1] > 0))
        self.H = {l: sp.csr_matrix(B.f2(np.zeros(self.sizes[l]), Mo.x, Mo.w, T * c, Mo.R[l], Mo.D, z))
                  for l in range(self.c0, self.top + 1)}
        self.g = B.f1(self.s, Mo.x, Mo.w, T * c, Mo.R[self.top], Mo.D, z0)
        self.lam = {l: lambda_max(self.H[l]) for l in range(self.c0 + 1, self.top + 1)}
        self.P = {l: nodal_prolongation(Mo.R[l + 1], Mo.R[l]) for l in range(self.c0, self.top)}
        self._V, self._cg = {}, {}

    def is_spd(self):
        """True if the top Hessian has a Cholesky factor."""
        try:
            np.linalg.cholesky(self.H[self.top].toarray())
            return True
        except np.linalg.LinAlgError:
            return False

    def V(self, degree, dtype, lam=None):
        """The V-cycle of this system (cached per degree and dtype while lam is the pinned one)."""
        if lam is not None:
            return Vcycle(self.H, self.P, lam, self.c0, self.top, degree, dtype)
        key = (degree, dtype)
        if key not in self._V:
            self._V[key] = Vcycle(self.H, self.P, self.lam, self.c0, self.top, degree, dtype)
        return self._V[key]

    def random(self, seed):
        return np.random.default_rng(seed).standard_normal(self.N)

    def cg(self, degree, rtol, maxit, dtype, count_seed=None):
        """pcg on H_top x = g (the gradient, or count_rhs(count_seed)) with the V-cycle of `degree`, cached."""
        key = (degree, rtol, maxit, dtype, count_seed)
        if key not in self._cg:
            g = self.g if count_seed is None else count_rhs(self, count_seed)
            self._cg[key] = pcg(Mat(self.H[self.top], dtype), self.V(degree, dtype), g.astype(dtype), rtol, maxit)
        return self._cg[key]

    def direct(self, g):
        return spla.spsolve(sp.csc_matrix(self.H[self.top]), g)


def bound(d64):
    """The bound of a device result whose float64 restatement is `d64` away from the long-double one: 100 times that (the
    device sums in another order), at least 1e-11 (what test_gpu_mg.py gives the same recurrences)."""
    return max(FLOOR, FACTOR * d64)


def count_rhs(S, seed):
    """Right-hand side of the iteration-count test: standard normal entries scaled by 10^U(-3, 3) each."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(S.N) * 10.0 ** rng.uniform(-3, 3, S.N)


def count_margins(res, rtol=COUNT_RTOL):
    """<r, V r> / (rtol^2 <r0, V r0>) at the last two iterations of a pcg result."""
    thr = LD(rtol) ** 2 * LD(res.rz[0])
    return float(res.rz[-2] / thr), float(res.rz[-1] / thr)


_systems = {}


def system(kind, L, p, mesh=None):
    """The shared System of a case: computed once per process and left unchanged."""
    key = (kind, L, float(p), mesh)
    if key not in _systems:
        _systems[key] = System(kind, L, float(p), mesh)
    return _systems[key]


def case_id(c):
    return "%s-L%d-p%g" % c[:3] + ("" if len(c) == 3 else "-" + c[3])
