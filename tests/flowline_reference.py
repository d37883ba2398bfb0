"""Independent numpy restatement, in np.longdouble, of the flow-line rule of include/mgb_hip.h: the
yardstick of test_flowline_reference.py, test_flowline_host.py and test_gpu_flow_lines.py.  Not a test.  It takes x, the block
size and one nodal column and shares no code with the library: the inverse element maps, the containment rule, the search for
the lowest containing element (brute force over all elements, no bins), the P2 + bubble and the tensor Lagrange bases, the two
stages, the stops and the exit bisection are all written out again here.

trace() follows one line from its seed; step() takes ONE step of the rule from a given point in a given element (the one-step
replay: a library path is checked point by point, so its roundings never accumulate against the yardstick).  With a step comes
the bar a double-precision evaluation of that step is held to:

  bar = 2 ds (E_1 + E_m) + 16 eps (max|x| + ds),      E_s = (C eps S_s + R_s) / a_s     for the stages s = 1 (at x_k), m (midpoint)

  S_s = | (sum_j |d_c N_j| |z_j|)_c |: a sum of n = block products carries at most (n - 1) eps S from the additions, eps S from
        the products and a few eps S from the basis values and the map to physical axes: C = 2 block + 2, the 16 of
        levelset_reference.py for the seven-term sums (there it appears as 32 eps S because two corners move its quotient);
  R_s = the move of the gradient when the reference coordinates move by their own rounding, 4 eps max(1, |r|) per coordinate
        (a difference, two products, a difference and a division): sum_c |grad(r + delta_c) - grad(r)|, taken in longdouble;
  2 / a_s: d = g / |g| moves by at most 2 |dg| / |g|; the error of stage 1 moves the midpoint by ds E_1 and through it g_m by
        |H| ds E_1, which the factor 2 on E_1 covers while |H| ds <= 2 a_m (lines that stay a step away from critical points);
  16 eps (max|x| + ds): the two updates x + c d, the 8 eps (span + max|x|) of levelset_reference.py doubled for the two stages.

A step is UNDECIDED when a stage point lies so close to the boundary of an element that double and longdouble may locate it
differently: some containment inequality of some element is within tau + bar (in reference coordinates) of its threshold.
The exit point of a line is held to |q - x_k| 2^-40 + 2 bar: both bisections bracket the same crossing to 2^-40 of the
segment, and the crossing itself moves by at most the bar on either side."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TAU = LD(1e-12)
EXIT, STALLED, MAXSTEPS, OUTSIDE, NONFINITE = 0, 1, 2, 3, 4
BISECT = 40


def _lagrange(K, t):
    """values and d/dt of the degree-K Lagrange basis on the nodes j / K at t (longdouble)."""
    nodes = [LD(j) / LD(K) for j in range(K + 1)]
    v, d = [], []
    for j in range(K + 1):
        prod = LD(1)
        for i in range(K + 1):
            if i != j:
                prod = prod * (t - nodes[i]) / (nodes[j] - nodes[i])
        s = LD(0)
        for m in range(K + 1):
            if m == j:
                continue
            q = LD(1) / (nodes[j] - nodes[m])
            for i in range(K + 1):
                if i != j and i != m:
                    q = q * (t - nodes[i]) / (nodes[j] - nodes[i])
            s = s + q
        v.append(prod)
        d.append(s)
    return np.array(v, dtype=LD), np.array(d, dtype=LD)


class Mesh:
    """x (n, dim) float64 and the block size: 7 in 2-D, (k + 1)^3 in 3-D."""

    def __init__(self, x, block):
        x = np.asarray(x, dtype=np.float64)
        self.dim, self.block = x.shape[1], block
        self.nel = x.shape[0] // block
        self.X = x.astype(LD).reshape(self.nel, block, self.dim)
        self.xmax = LD(np.abs(x).max())
        if self.dim == 2:
            assert block == 7
            self.v0 = self.X[:, 0]
            self.a, self.b = self.X[:, 1] - self.v0, self.X[:, 2] - self.v0
            self.det = self.a[:, 0] * self.b[:, 1] - self.a[:, 1] * self.b[:, 0]
            inv = np.stack([np.abs(self.b[:, 1]) + np.abs(self.b[:, 0]), np.abs(self.a[:, 1]) + np.abs(self.a[:, 0])], axis=1)
            self.stretch = 2 * inv.max(axis=1) / np.abs(self.det)      # |dr| <= stretch |dx| for r0, r1 and 1 - r0 - r1
        else:
            assert self.dim == 3
            self.k = round(block ** (1.0 / 3.0)) - 1
            assert (self.k + 1) ** 3 == block
            self.A, self.B = self.X[:, 0], self.X[:, -1]
            self.stretch = (1 / np.abs(self.B - self.A)).max(axis=1)
        ext = (self.X.max(axis=1) - self.X.min(axis=1)).max(axis=1)
        self.default_ds = float(ext.min()) / 4

    def _ref(self, sel, q):
        if self.dim == 2:
            px, py = q[0] - self.v0[sel, 0], q[1] - self.v0[sel, 1]
            a, b, det = self.a[sel], self.b[sel], self.det[sel]
            return np.stack([(px * b[..., 1] - py * b[..., 0]) / det, (a[..., 0] * py - a[..., 1] * px) / det], axis=-1)
        return (q - self.A[sel]) / (self.B[sel] - self.A[sel])

    def _slack(self, r):
        """the containment inequalities as values that must be >= -tau, last axis"""
        if self.dim == 2:
            return np.stack([1 - r[..., 0] - r[..., 1], r[..., 0], r[..., 1]], axis=-1)
        return np.concatenate([r, 1 - r], axis=-1)

    def ref(self, e, q):
        r = self._ref(e, q)
        with np.errstate(invalid="ignore"):
            return r, bool((self._slack(r) >= -TAU).all())

    def find(self, q):
        if not np.isfinite(q.astype(np.float64)).all():
            return -1
        with np.errstate(invalid="ignore"):
            inside = (self._slack(self._ref(slice(None), q)) >= -TAU).all(axis=-1)
        hit = np.nonzero(inside)[0]
        return int(hit[0]) if len(hit) else -1

    def locate(self, e, q):
        return e if self.ref(e, q)[1] else self.find(q)

    def undecided(self, q, bar):
        """some inequality of some element within tau + bar (reference units) of its threshold"""
        s = self._slack(self._ref(slice(None), q))
        band = TAU + bar * self.stretch
        return bool((np.abs(s + TAU) < band[:, None]).any())

    def basis_grad(self, e, r):
        """(block, dim) physical gradients of the nodal basis of element e at reference coordinates r"""
        if self.dim == 2:
            xi, et = r
            l = [1 - xi - et, xi, et]
            dl = np.array([[-1, -1], [1, 0], [0, 1]], dtype=LD)
            b = l[0] * l[1] * l[2]
            db = dl[0] * l[1] * l[2] + l[0] * dl[1] * l[2] + l[0] * l[1] * dl[2]
            G = [(4 * l[i] - 1) * dl[i] + 3 * db for i in range(3)]
            G += [4 * (l[i] * dl[(i + 1) % 3] + l[(i + 1) % 3] * dl[i]) - 12 * db for i in range(3)]
            G.append(27 * db)
            G = np.array(G, dtype=LD)
            a, bb, det = self.a[e], self.b[e], self.det[e]
            return np.stack([(bb[1] * G[:, 0] - a[1] * G[:, 1]) / det, (-bb[0] * G[:, 0] + a[0] * G[:, 1]) / det], axis=1)
        K = self.k
        L = [_lagrange(K, r[d]) for d in range(3)]
        h = self.B[e] - self.A[e]
        G = np.empty((self.block, 3), dtype=LD)
        for m in range(K + 1):
            for j in range(K + 1):
                for i in range(K + 1):
                    n = i + (K + 1) * (j + (K + 1) * m)
                    G[n] = [L[0][1][i] * L[1][0][j] * L[2][0][m] / h[0], L[0][0][i] * L[1][1][j] * L[2][0][m] / h[1],
                            L[0][0][i] * L[1][0][j] * L[2][1][m] / h[2]]
        return G

    def basis_val(self, e, r):
        if self.dim == 2:
            xi, et = r
            l = [1 - xi - et, xi, et]
            b = l[0] * l[1] * l[2]
            N = [l[i] * (2 * l[i] - 1) + 3 * b for i in range(3)] + [4 * l[i] * l[(i + 1) % 3] - 12 * b for i in range(3)] + [27 * b]
            return np.array(N, dtype=LD)
        K = self.k
        L = [_lagrange(K, r[d])[0] for d in range(3)]
        return np.array([L[0][i] * L[1][j] * L[2][m] for m in range(K + 1) for j in range(K + 1) for i in range(K + 1)], dtype=LD)


class Field:
    """one nodal column z (n,) on a Mesh"""

    def __init__(self, mesh, z):
        self.mesh = mesh
        self.z = np.asarray(z, dtype=np.float64).astype(LD).reshape(mesh.nel, mesh.block)

    def value(self, e, q):
        r, _ = self.mesh.ref(e, q)
        with np.errstate(invalid="ignore"):
            return (self.mesh.basis_val(e, r) * self.z[e]).sum()

    def value_bar(self, e, q):
        """C eps sum_j |N_j| |z_j|: what a double evaluation of value() may be off by"""
        r, _ = self.mesh.ref(e, q)
        with np.errstate(invalid="ignore"):
            return (2 * self.mesh.block + 2) * EPS * (np.abs(self.mesh.basis_val(e, r)) * np.abs(self.z[e])).sum()

    def grad(self, e, q):
        """g (dim,), and E = (C eps S + R) / |g| of the bar (inf where it cannot be formed)"""
        M = self.mesh
        r, _ = M.ref(e, q)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            G = M.basis_grad(e, r)
            g = (G * self.z[e][:, None]).sum(axis=0)
            a = np.sqrt((g * g).sum())
            S = np.sqrt(((np.abs(G) * np.abs(self.z[e])[:, None]).sum(axis=0) ** 2).sum())
            R = LD(0)
            for c in range(M.dim):
                rr = r.copy()
                rr[c] = rr[c] + 4 * EPS * max(LD(1), abs(r[c]))
                R = R + np.abs((M.basis_grad(e, rr) * self.z[e][:, None]).sum(axis=0) - g).sum()
            E = ((2 * M.block + 2) * EPS * S + R) / a if np.isfinite(a) and a > 0 else LD(np.inf)
        return g, a, E


def slowness(a, p):
    return LD(1) if p == 1 else 1 / a if p == 2 else a ** (LD(1) - LD(p))


class Step:
    """kind: one of 'step', 'exit', STALLED, MAXSTEPS, NONFINITE (the stops keep the point); x, e: the next (or end) point and
    its element; recorded: whether it is recorded; dlength, dtime and their bars lbar, tbar (the relative error of a^(1-p) is
    |1 - p| times that of a: E_m + 2 E_1 by the reasoning of the module text, plus 4 eps for pow, product and sum; an exit moves
    lo |q - x_k| by its exit bar); v: the value at the START point; bar; undecided."""


def step(F, x, e, k, p, sgn, ds, max_steps, gmin):
    M = F.mesh
    out = Step()
    out.x, out.e, out.recorded, out.dlength, out.dtime, out.bar, out.undecided = x, e, False, LD(0), LD(0), LD(0), False
    out.lbar = out.tbar = LD(0)
    ds, sgn, gmin = LD(ds), LD(sgn), LD(gmin)
    out.v = F.value(e, x)
    g, a, E1 = F.grad(e, x)
    if not (np.isfinite(out.v) and np.isfinite(g).all()):
        out.kind = NONFINITE
        return out
    if not a > gmin:
        out.kind = STALLED
        return out
    if k == max_steps:
        out.kind = MAXSTEPS
        return out
    out.a = a
    upd = 16 * EPS * (M.xmax + ds)
    q = x + (ds / 2) * (sgn * g / a)
    out.bar = 2 * ds * E1 + upd
    out.undecided = M.undecided(q, out.bar)
    em = M.locate(e, q)
    if em >= 0:
        gm, am, Em = F.grad(em, q)
        if not np.isfinite(gm).all():
            out.kind = NONFINITE
            return out
        if not am > gmin:
            out.kind = STALLED
            return out
        q = x + ds * (sgn * gm / am)
        out.bar = 2 * ds * (E1 + Em) + upd
        out.undecided = out.undecided or M.undecided(q, out.bar)
        en = M.locate(em, q)
        if en >= 0:
            out.kind, out.x, out.e, out.recorded = "step", q, en, True
            out.dlength, out.dtime = ds, ds * slowness(am, p)
            out.lbar, out.tbar = EPS * ds, out.dtime * (abs(1 - LD(p)) * (Em + 2 * E1) + 4 * EPS)
            return out
    lo, hi, er, dq = LD(0), LD(1), e, q - x
    for _ in range(BISECT):
        th = (lo + hi) / 2
        ee = M.locate(e, x + th * dq)
        if ee >= 0:
            lo, er = th, ee
        else:
            hi = th
    span = np.sqrt((dq * dq).sum())
    out.kind, out.x, out.e, out.recorded = "exit", x + lo * dq, er, bool(lo > 0)
    out.dlength, out.dtime = lo * span, lo * span * slowness(a, p)
    out.exit_bar = span * LD(2) ** -BISECT + 2 * out.bar
    out.lbar = out.exit_bar + 4 * EPS * out.dlength
    out.tbar = out.exit_bar * slowness(a, p) + out.dtime * (abs(1 - LD(p)) * E1 + 4 * EPS)
    return out


class Line:
    """status, count, length, time, u_start, u_end, end (dim,), end_element, pts (count, dim), elems (count,), undecided = the
    number of steps whose decisions a double evaluation may take differently."""


def trace(mesh, z, seed, p=2.0, direction=1, ds=None, max_steps=1024, gmin=1e-12):
    F = z if isinstance(z, Field) else Field(mesh, z)
    ds = mesh.default_ds if ds is None else ds
    out = Line()
    x = np.asarray(seed, dtype=np.float64).astype(LD)
    e = mesh.find(x)
    nan = LD(np.nan)
    out.undecided, out.steps = 0, 0
    if e < 0:
        out.status, out.count, out.length, out.time, out.u_start, out.u_end = OUTSIDE, 0, nan, nan, nan, nan
        out.end, out.end_element, out.pts, out.elems = np.full(mesh.dim, nan), -1, np.empty((0, mesh.dim), dtype=LD), np.empty(0, dtype=int)
        return out
    pts, elems = [x], [e]
    out.length, out.time = LD(0), LD(0)
    k = 0
    while True:
        s = step(F, x, e, k, p, direction, ds, max_steps, gmin)
        if k == 0:
            out.u_start = s.v
        out.u_end = s.v
        out.undecided += int(s.undecided)
        out.steps += 1
        out.length, out.time = out.length + s.dlength, out.time + s.dtime
        x, e = s.x, s.e
        if s.recorded:
            pts.append(x), elems.append(e)
        if s.kind == "step":
            k += 1
            continue
        if s.kind == "exit":
            out.status, out.u_end = EXIT, F.value(e, x)
        else:
            out.status = s.kind
        break
    out.count, out.end, out.end_element = len(pts), x, e
    out.pts, out.elems = np.array(pts, dtype=LD), np.array(elems, dtype=int)
    return out
