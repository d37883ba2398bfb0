"""Independent numpy restatement, in np.longdouble, of the path-line rule of include/mgb_hip.h: the
yardstick of test_pathline_reference.py, test_pathline_host.py and test_gpu_path_lines.py.  Not a test.  It stands on
flowline_reference.py's Mesh and Field (inverse maps, containment rule, brute-force search for the lowest containing element,
bases) and shares no code with the library: the blend in time, the fractions, the velocity, the rest, the two stages, the exit
and the bookkeeping of times are written out again here.

trace() follows one particle from its seed; step() takes ONE step of the rule from a given point in a given element at a given
place (slab j, step i) in time: the one-step replay, in which a library path is checked point by point so that its roundings
never accumulate against the yardstick.  With a step comes the bar a double-precision evaluation of that step is held to:

  bar = dt (W_1 + W_m) + 16 eps (max|x| + dt |w_m|)                          for the stages s = 1 (at x_k), m (midpoint)

  D_s = (1 - th) D_a + th D_b + 4 eps (|g_a| + |g_b|): what the blended gradient may be off by; D_a, D_b = C eps S + R of each
        snapshot, the gradient bar of flowline_reference.py (C = 2 block + 2, S the sum of absolute terms, R the move of the
        gradient when the reference coordinates move by their own rounding), taken absolutely, not divided by |g|; the last
        term covers the difference, the product with th (itself rounded once, (double) i / n) and the sum;
  W_s = speed a^(p-2) (1 + |p - 2|) D_s + 4 eps |w_s| [+ 4 eps |w_s| for pow when p is none of 1, 1.5, 2]: w = speed sgn
        a^(p-2) g moves by a^(p-2) |dg| through g and by |p - 2| a^(p-3) |g| |dg| through a; the products, the quotient and the
        square root add a few eps |w|;
  dt W_1 stands for the error of stage 1 carried through the midpoint: it moves q_m by (dt / 2) W_1 and through it w_m by
        |dw/dx| (dt / 2) W_1, which dt W_1 covers while dt |dw/dx| <= 2 (steps shorter than the time in which the velocity
        changes by itself; a midpoint that may change its element is undecided, below);
  16 eps (max|x| + dt |w|): the two updates x + c w with dt = (ts[j+1] - ts[j]) / n rounded once, as in section 4q.

A step is UNDECIDED when a stage point lies within tau + bar (in reference coordinates) of a containment threshold of some
element, or when |g| of a stage lies within its own D_s of gmin (the rest rule may be taken differently).  The exit point of a
particle is held to |q - x_k| 2^-40 + 2 bar, its exit time to span 2^-40 + 2 bar / |w| of the stage that left."""
import numpy as np

import flowline_reference as FR

LD = FR.LD
EPS = FR.EPS
DONE, EXIT, OUTSIDE, NONFINITE = 0, 1, 2, 3
BISECT = 40


def _grad_abs(F, e, q):
    """g (dim,) of one snapshot and D = C eps S + R, absolute"""
    M = F.mesh
    r, _ = M.ref(e, q)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        G = M.basis_grad(e, r)
        g = (G * F.z[e][:, None]).sum(axis=0)
        S = np.sqrt(((np.abs(G) * np.abs(F.z[e])[:, None]).sum(axis=0) ** 2).sum())
        R = LD(0)
        for c in range(M.dim):
            rr = r.copy()
            rr[c] = rr[c] + 4 * EPS * max(LD(1), abs(r[c]))
            R = R + np.abs((M.basis_grad(e, rr) * F.z[e][:, None]).sum(axis=0) - g).sum()
    return g, (2 * M.block + 2) * EPS * S + R


def blend(Fa, Fb, e, q, th):
    """v, g of the field in time and D, the bar of g"""
    th = LD(th)
    va, vb = Fa.value(e, q), Fb.value(e, q)
    ga, Da = _grad_abs(Fa, e, q)
    gb, Db = _grad_abs(Fb, e, q)
    with np.errstate(invalid="ignore", over="ignore"):
        v = va + th * (vb - va)
        g = ga + th * (gb - ga)
        D = (1 - th) * Da + th * Db + 4 * EPS * (np.sqrt((ga * ga).sum()) + np.sqrt((gb * gb).sum()))
    return v, g, D


def value_bar(Fa, Fb, e, q):
    return Fa.value_bar(e, q) + Fb.value_bar(e, q) + 4 * EPS * (abs(Fa.value(e, q)) + abs(Fb.value(e, q)))


def velocity(g, D, p, sgn, speed, gmin):
    """w, its bar W, whether the particle moves, whether that decision is within its bar"""
    a = np.sqrt((g * g).sum())
    near = bool(abs(a - gmin) <= D)
    if not a > gmin:
        return np.zeros(len(g), dtype=LD), LD(0), False, near
    p = LD(p)
    f = LD(1) / a if p == 1 else LD(1) if p == 2 else 1 / np.sqrt(a) if p == 1.5 else a ** (p - 2)
    w = speed * (sgn * g * f)
    wn = np.sqrt((w * w).sum())
    W = speed * f * (1 + abs(p - 2)) * D + 4 * EPS * wn + (0 if p in (1, 1.5, 2) else 4 * EPS * wn)
    return w, W, True, near


class Step:
    """kind: 'step', 'exit' or NONFINITE (which keeps the point); x, e: the next (or end) point and its element; recorded;
    moved: False when the accepted step rested; dlength; bar; exit_bar, time and time_bar of an exit; v: the blended value at
    the START point; undecided."""


def step(Fa, Fb, t0, t1, n, i, x, e, p, sgn, speed, gmin):
    M = Fa.mesh
    out = Step()
    out.x, out.e, out.recorded, out.moved, out.dlength, out.bar, out.undecided = x, e, False, True, LD(0), LD(0), False
    sgn, speed, gmin, n = LD(sgn), LD(speed), LD(gmin), int(n)
    slab = LD(t1) - LD(t0)
    dt = slab / n
    th, thm, tk = LD(i) / n, LD(2 * i + 1) / (2 * n), LD(t0) + i * dt
    out.tk = tk
    out.v, g, D1 = blend(Fa, Fb, e, x, th)
    if not (np.isfinite(out.v) and np.isfinite(g).all()):
        out.kind = NONFINITE
        return out
    w, W1, _, near = velocity(g, D1, p, sgn, speed, gmin)
    out.undecided = near
    span = dt / 2
    q = x + span * w
    wn = np.sqrt((w * w).sum())
    out.bar = dt * W1 + 16 * EPS * (M.xmax + dt * wn)
    out.undecided = out.undecided or M.undecided(q, out.bar)
    em = M.locate(e, q)
    if em >= 0:
        _, gm, Dm = blend(Fa, Fb, em, q, thm)
        if not np.isfinite(gm).all():
            out.kind = NONFINITE
            return out
        w, Wm, moved, near = velocity(gm, Dm, p, sgn, speed, gmin)
        wn = np.sqrt((w * w).sum())
        span = dt
        q = x + dt * w
        out.bar = dt * (W1 + Wm) + 16 * EPS * (M.xmax + dt * wn)
        out.undecided = out.undecided or near or M.undecided(q, out.bar)
        en = M.locate(em, q)
        if en >= 0:
            out.kind, out.x, out.e, out.recorded, out.moved = "step", q, en, True, moved
            out.dlength = dt * wn
            out.lbar = out.bar
            return out
    lo, hi, er, dq = LD(0), LD(1), e, q - x
    for _ in range(BISECT):
        mid = (lo + hi) / 2
        ee = M.locate(e, x + mid * dq)
        if ee >= 0:
            lo, er = mid, ee
        else:
            hi = mid
    seg = np.sqrt((dq * dq).sum())
    out.kind, out.x, out.e, out.recorded = "exit", x + lo * dq, er, bool(lo > 0)
    out.dlength = lo * seg
    out.exit_bar = seg * LD(2) ** -BISECT + 2 * out.bar
    out.lbar = out.exit_bar + 4 * EPS * out.dlength
    out.time = tk + lo * span
    out.time_bar = span * LD(2) ** -BISECT + (2 * out.bar / wn if wn > 0 else LD(np.inf)) + 4 * EPS * abs(out.time)
    out.th_end = th + lo * span / slab
    return out


class Line:
    """status, count, rested, length, time, u_start, u_end, max_step, end (dim,), end_element, pts (count, dim), elems
    (count,), steps = the steps taken, undecided = how many of them a double evaluation may decide differently."""


def trace(mesh, fields, ts, seed, release, stop, substeps, p=2.0, direction=-1, speed=1.0, gmin=1e-12):
    F = [z if isinstance(z, FR.Field) else FR.Field(mesh, z) for z in fields]
    out = Line()
    x = np.asarray(seed, dtype=np.float64).astype(LD)
    e = mesh.find(x)
    nan = LD(np.nan)
    out.undecided, out.steps, out.rested = 0, 0, 0
    if e < 0:
        out.status, out.count, out.length, out.time, out.u_start, out.u_end, out.max_step = OUTSIDE, 0, nan, nan, nan, nan, nan
        out.end, out.end_element, out.pts, out.elems = np.full(mesh.dim, nan), -1, np.empty((0, mesh.dim), dtype=LD), np.empty(0, dtype=int)
        return out
    pts, elems = [x], [e]
    out.length, out.max_step, out.status, out.time, out.u_start = LD(0), LD(0), DONE, LD(ts[stop]), None
    for j in range(release, stop):
        for i in range(substeps):
            s = step(F[j], F[j + 1], ts[j], ts[j + 1], substeps, i, x, e, p, direction, speed, gmin)
            if out.u_start is None:
                out.u_start = s.v
            out.undecided += int(s.undecided)
            out.steps += 1
            out.length = out.length + s.dlength
            x, e = s.x, s.e
            if s.recorded:
                pts.append(x), elems.append(e)
            if s.kind == "step":
                out.max_step = max(out.max_step, s.dlength)
                out.rested += int(not s.moved)
                continue
            if s.kind == "exit":
                out.status, out.time = EXIT, s.time
                out.u_end = blend(F[j], F[j + 1], e, x, s.th_end)[0]
            else:
                out.status, out.time = NONFINITE, s.tk
                out.u_end = s.v if not np.isfinite(s.v) else nan
            break
        if out.status != DONE:
            break
    if out.status == DONE:
        out.u_end = F[stop].value(e, x)
    out.count, out.end, out.end_element = len(pts), x, e
    out.pts, out.elems = np.array(pts, dtype=LD), np.array(elems, dtype=int)
    return out
