"""Reference time loop of parabolic_solve with time-dependent data, in numpy, built from the CPU oracle's pieces
(O.parabolic_problem, O.parabolic_initial, O.parabolic_cost, O.amgb_core); the yardstick of test_parabolic_reference.py
and test_gpu_parabolic_time.py.  Not a test.

Step from t_k to t_{k+1} = t_k + h (implicit Euler: forcing and boundary data at t_{k+1}), DESIGN.md section 4f:
  cost        c = O.parabolic_cost(n, K, p, h, f, u_k)                     (u_k: the OLD u, old boundary values included)
  boundary    u[b] = gb on the boundary nodes b = the empty rows of subspaces["dirichlet"][-1]
  violations  v1 = max_i (u_i^2 - s1_i),  v2 = max_i ((sum_d (op_d u)_i^2)^(p/2) - s2_i)
  lifts       lift_j = 1 + v_j if v_j >= 0 else exactly 0;  s_j += lift_j at every node (a column with lift 0 is not touched)
  solve       O.amgb_core from the lifted z."""
import math

import numpy as np

import mgb_oracle as O

# fixture data of the issue: non-uniform steps, none a power of two; data that depend on t
TS = np.array([0.0, 0.3, 0.5, 1.0])
G_T = {1: lambda t, x: np.array([x[0] * (1 + 0.5 * t) + 0.3 * t, 0.0]),
       2: lambda t, x: np.array([(x[0] ** 2 + x[1] ** 2) * (1 + 0.5 * t) + 0.3 * t * x[0], 0.0])}
F_T = {1: lambda t, x: 0.5 + t * x[0],
       2: lambda t, x: 0.5 + t * x[0] - 0.25 * t ** 2 * x[1]}


def boundary_nodes(dirichlet_finest):
    """Nodes that carry Dirichlet data: the rows of the finest `dirichlet` subspace matrix that have no entry."""
    return np.flatnonzero(np.diff(dirichlet_finest.tocsr().indptr) == 0)


def lift_of(v):
    return 1.0 + v if v >= 0 else 0.0


def step_transition(z, n, K, p, h, f, bidx, gb, grad_ops):
    """One transition on z = [u; s1; s2] (3 n values, not modified).  Returns (c, z_new, (v1, v2), (lift_1, lift_2))."""
    c = O.parabolic_cost(n, K, p, h, np.asarray(f, dtype=np.float64), z[:n])
    z = z.copy()
    if gb is not None:
        z[np.asarray(bidx)] = gb
    u, s1, s2 = z[:n], z[n:2 * n], z[2 * n:]
    grad2 = sum((op @ u) ** 2 for op in grad_ops)
    v1 = float(np.max(u * u - s1))
    v2 = float(np.max(grad2 ** (p / 2.0) - s2))
    l1, l2 = lift_of(v1), lift_of(v2)
    if l1 != 0.0:
        z[n:2 * n] = s1 + l1
    if l2 != 0.0:
        z[2 * n:] = s2 + l2
    return c, z, (v1, v2), (l1, l2)


def reference_loop(geo, p, ts, f1, g, tol=None):
    """Snapshots (list of (n, 3) arrays, one per entry of ts) and lifts ((len(ts) - 1, 2)) of the loop with f1(t, x), g(t, x)."""
    tol = math.sqrt(np.finfo(np.float64).eps) if tol is None else tol
    state, D, K, cones, ops = O.parabolic_problem(geo, p)
    M = O.amg(geo, state, D)
    B = O.Barrier(O.ConeIntersection([O.convex_Euclidian_power(idx, pp) for idx, pp in cones]))
    x = M.x
    n = x.shape[0]
    bidx = boundary_nodes(geo.subspaces["dirichlet"][-1])
    grad_ops = [geo.operators[o] for o in ops]
    ts = np.asarray(ts, dtype=np.float64)
    z = O.parabolic_initial(geo, p, lambda xi: g(ts[0], xi))
    u = [z.reshape(n, 3, order="F").copy()]
    lifts = np.zeros((len(ts) - 1, 2))
    for k in range(len(ts) - 1):
        t_new, h = ts[k + 1], ts[k + 1] - ts[k]
        f = np.array([f1(t_new, xi) for xi in x], dtype=np.float64)
        gb = np.array([g(t_new, x[b])[0] for b in bidx], dtype=np.float64)
        c, z, _, lifts[k] = step_transition(z, n, K, p, h, f, bidx, gb, grad_ops)
        z = O.amgb_core(B, M, z, c, tol)["z"]
        u.append(z.reshape(n, 3, order="F").copy())
    return u, lifts


_CACHE = {}


def fixture_loop(kind, L, p):
    """reference_loop on the fixture data, computed once per (kind, L, p) and shared; callers must not modify the result."""
    key = (kind, L, float(p))
    if key not in _CACHE:
        geo = getattr(O, kind)(L)
        dim = geo.discretization["dim"]
        _CACHE[key] = (geo,) + reference_loop(geo, p, TS, F_T[dim], G_T[dim])
    return _CACHE[key]
