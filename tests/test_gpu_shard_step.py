"""Every kernel and table a SHARDED Newton step adds to the single-GPU step, each held to an exact restatement -- not through the z
of a whole solve, which a damped Newton iteration reaches from a wrong Hessian, a wrong |g|^2 or a worse direction just as well.
Run with -m gpu -s -x under an outer timeout on an MI355X; profiles/shard_step_reference.txt is the output of such a run.

Processes as in test_shard.py (spawn, gloo, be.set_comm(rank, world, torch_allreduce(dist, 0)), all ranks on the one GPU), with this
discipline: workers assert nothing, they compute and put plain arrays on the queue, every rank runs the same sequence of collectives
whatever the values are (expected MGBErrors become codes; anything else is recorded and, by a summed abort double in front of every
case, makes ALL ranks skip the rest of that shape); all assertions are in the parent; all shapes and cases of one (world,
MGB_RANK_ALIGNED) pair run in ONE spawn; the parent waits GROUP_TIMEOUT (3 x the slowest measured group) and on a timeout or a
non-zero exit code terminates the workers and fails.

State (test_gpu_elop_kinds.py's): s = 2e-3 randn around the default z0, t = 3.7, default cone p = 1.5, finest level.  Reference:
barrier_reference.level_reference at the DEVICE's Dz (apply_D_global, asserted bit for bit equal to the unsharded apply_D); its
bounds hold for any order of summation, so they cover rank partial sums followed by a collective.  Ratios are held to MARGIN *
max(baseline, 1), baseline = oracle_level_baseline at the same state (shapes without a dense H: MARGIN itself).  Matrices: (a') =
shard_reference.dyadic(chol_reference.random_spd), whose rank shares add up exactly in any order; (c) = the real Hessian.  Solutions
are held to chol_reference.Reference.metrics: eta <= 16 max(eta_baseline, u), phi <= 16 max(phi_baseline, u) where the reference
is exact; shapes beyond a dense factor: eta <= 16 u alone.

Cases, and what each would catch (csrc/gpuchol.hip, csrc/kernels.hip, csrc/amg.cpp):
  A  public f0(parts) / f1 / f2 on a sharded context against f0F, f0C, g, H; bit-identical across ranks.  The allreduce branches of
     dev_f0 / dev_f1 / f2 and the row partition of B, BT and the assembly.
  B  (aligned) the kind table of GpuChol::build: every unknown kind 1 on exactly one rank and 0 on the others, or 2 on all; no
     pattern entry couples kind-1 unknowns of two ranks (what dof_rank_masks is for); chol_info()["exchange_doubles"] = sum over the
     subtree roots of nb (nb + 3) / 2 + top values, from chol_schedule's tree and the kinds.  `kind` and, through C, `top_unk`.
  C  f1_owner: g where kind >= 1 against g (gather_top_kernel, the collective, scatter_top_norm_kernel: a top entry missing from
     top_unk, gathered from or scattered to the wrong place, or dropped by the multi-pass loop over ntop > 256, is an O(1) error in
     g); top entries bit-identical across ranks; |g|^2 against the exact dot of the gradient assembled from the owners
     (dot_owned_kernel with count_top = 0 plus scatter_top_norm_kernel's sum: counting the top on every rank, or on none, is an error
     of the size of the top's share of |g|^2).  The owner-local branch of dev_f1.
  D  f2_local: the long-double sum over the ranks against H (values_stay_local: no allreduce); exactly zero on entries with an
     endpoint of kind 0; at least one top entry is non-zero on two ranks, else nothing rides along.
  E  solve_linear_local on exact shares of (a'), g poisoned where kind = 0: x == 0 where kind = 0 (x_local_kernel), x assembled from
     the owners within eta / phi (schur_pack_kernel / schur_unpack_kernel: a wrong packed offset or a dropped right-hand-side row
     i = nb changes the top's matrix or right-hand side by O(1); vals_pack_kernel / vals_unpack_kernel: a share dropped or counted
     twice changes a top-top entry by a binary fraction of itself; factor_solve_split's order of chain segments), top part of x
     bit-identical across ranks, <g, x> against the exact dot (dot_owned_kernel with count_top = (rank == 0): counting the top on
     every rank adds (world - 1) times the top's share), flag 0 (flag_to_double_kernel and the scal[3..10] collective), vals_after
     == the exact value on top-top entries and == the input elsewhere (vals_unpack_kernel's indices, top_value_indices).
     The owner-local branch of dev_f2_solve.
  F  the same on the values of D: the path of a Newton step from assembly to direction.  The matrix handed to Reference is the fp64
     sum of the shares in rank order, which differs from what the collective formed by at most (world - 1) u per entry: a backward
     perturbation of that size is what the factor 16 of the eta bound covers next to the solver's own.
  G  solve_linear(solver="gpu") on the sharded context (values_summed: no ride-along), both trees: x complete and bit-identical on
     every rank within eta / phi (xsol_pack_kernel / xsol_unpack_kernel and the `own` table: an unknown nobody or two ranks
     contribute comes back 0 or doubled).
  H  a diagonal entry of (a') set to -1 at an unknown of the last rank's subtree, at a top unknown (the -1 in one rank's share, zero
     in the others) and in rank 0's subtree: flag == 1 on every rank (local), MGB_E_NUMERIC on every rank (summed); (a') solved again
     is bit for bit the first solution (the flag re-armed, the fronts not poisoned).
  R  (not aligned) the three entry points refuse with MGB_E_ARG on every rank.

Coverage, asserted from the device's own tree (chol_schedule + kinds; on the geometric tree the subtree roots are the nodes
log2(world) levels below the root, tied to the device by exchange_doubles):
  (i)   a subtree root with nb > 64 (the y-grid of schur_pack / schur_unpack is capped at 64: strided column loop), both trees;
  (ii)  more than 256 top unknowns (scatter_top_norm's second pass, gather_top's second workgroup);
  (iv)  more than 256 top values at world 4 (vals_pack / vals_unpack past one workgroup), and at least 3 at fem1d L = 4.
(iii) nb + 1 > 256 (thread-strided inner loop of the pack kernels) needs fem2d L = 7: not run, see the profile.

Measured on an MI355X (profiles/shard_step_reference.txt holds every figure): worst ratio / max(baseline, 1) of the barrier
quantities 0.24 (world 4, geometric tree, fem1d L = 7, f1), |g|^2 and <g, x> at most 0.04 of their bound, eta at most 1.7 and phi at
most 4.2 times the baseline's.  MARGIN: the first run had it at the cap of 16 and gave the same figures; 0.24 rounded up to a power
of two is 0.25, times 4 for other devices and compilers = 1.  Groups take 3 to 4 s, the one of 8 ranks 36 to 107 s: eight
processes take turns on one GPU and every collective is staged through the host, so its two full shapes cost 20 to 60 s each.
"""
import os
import queue
import sys
import time
import types

import numpy as np
import pytest

import barrier_reference as BR
import chol_reference as CR
import mgb_oracle as O
import shard_reference as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1.0             # see above; never more than BR.MARGIN = 16
assert MARGIN <= BR.MARGIN
LD = BR.LD
T, AMP, P = 3.7, 2e-3, 1.5
POISON = 1e6             # what g holds where kind = 0 in the owner-local solves: the device must never read it
GROUP_TIMEOUT = 320.0    # seconds; 3 x the slowest group of the measured runs (world 8 aligned, 36 to 107 s: profiles/shard_step_reference.txt)
E_ARG, E_NUMERIC = -1, -3


def _shape(kind, L, cases, ref="full", need=()):
    """cases: letters; ref: "full" (dense H and factor), "grad" (no H, eta only); need: coverage conditions this shape must meet"""
    return types.SimpleNamespace(kind=kind, L=L, cases=cases, ref=ref, need=tuple(need), key="%s L=%d" % (kind, L))


ALL = "ABCDEFGH"
SUMMED = "ARGh"          # h: the summed part of H only
GROUPS = {
    "world 2 aligned": (2, "1", [_shape("fem1d", 4, ALL, need=["ride3"]), _shape("fem2d", 2, ALL), _shape("fem2d", 4, ALL),
                                 _shape("fem2d", 6, "BCE", ref="grad", need=["nb64"])]),
    "world 4 aligned": (4, "1", [_shape("fem1d", 4, ALL, need=["ride3"]), _shape("fem2d", 2, ALL),
                                 _shape("fem2d", 4, ALL, need=["vals256"])]),
    "world 8 aligned": (8, "1", [_shape("fem1d", 4, ALL, need=["ride3"]), _shape("fem2d", 2, ALL),
                                 _shape("fem2d", 5, "BCE", ref="grad", need=["nb64"]),
                                 _shape("fem2d", 6, "BC", ref="grad", need=["top256"])]),
    "world 2 geometric": (2, "0", [_shape("fem1d", 7, SUMMED), _shape("fem2d", 3, SUMMED),
                                   _shape("fem2d", 6, "Gh", ref="grad", need=["nb64"])]),
    "world 4 geometric": (4, "0", [_shape("fem1d", 7, SUMMED), _shape("fem2d", 3, SUMMED)]),
}


# ---------------------------------------------------------------------------------------------------------- workers
def _state(N, L):
    return AMP * np.random.default_rng(1000 + L).standard_normal(N)


def _matrix_a(rp, ci, L):
    return SR.dyadic(rp, ci, CR.random_spd(rp, ci, seed=40 + L))


def _rhs(N, L):
    return np.array([CR.rhs(N, seed=300 + 10 * L + k) for k in range(2)])


def _picks(owner, world):
    """the three unknowns of case H: in the last rank's subtree, in the top, in rank 0's subtree"""
    return [int(np.flatnonzero(owner == world - 1)[0]), int(np.flatnonzero(owner < 0)[0]), int(np.flatnonzero(owner == 0)[-1])]


def _worker(rank, world, port, q, shapes):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for pth in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, pth)
    import torch
    import torch.distributed as dist
    import mgb_amd as M
    from mgb_amd._lib import MGBError
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        be = M.backend_hip(0)
        be.set_comm(rank, world, M.torch_allreduce(dist, 0))
        out = {}
        for sh in shapes:
            t0 = time.time()
            res = dict(errors=[], skipped=[], codes={})

            def abort():      # summed over the ranks: all skip or none does
                flag = torch.tensor([1.0 if res["errors"] else 0.0], dtype=torch.float64)
                dist.all_reduce(flag)
                return flag.item() > 0

            def run(name, fn, *a):
                try:
                    return fn(*a)
                except MGBError as e:
                    res["codes"][name] = e.code
                except Exception as e:      # recorded; the parent fails on it
                    res["errors"].append("%s: %r" % (name, e))
                return None

            def gather(a):
                parts = [torch.zeros_like(torch.from_numpy(a)) for _ in range(world)]
                dist.all_gather(parts, torch.from_numpy(np.ascontiguousarray(a)))
                return np.stack([p.numpy() for p in parts])

            g = getattr(M, sh.kind + "_mpi")(sh.L, backend=be)
            dim = g.discretization["dim"]
            A = M.AMG(g, p=P)
            x = g.x.to_numpy()
            A.set_c(M._rows(M.DEFAULT_F[dim], x))
            A.set_z(M._rows(M.DEFAULT_G[dim], x).reshape(-1, order="F"))
            l = A.L - 1
            N, nz = A.level_size(l)
            rp, ci = A.hessian_pattern(l)
            sched = A.chol_schedule(l)
            res.update(N=N, nz=nz, rp=rp, ci=ci, info=A.chol_info(l), row0=A.row0, n_local=A.n_local,
                       tree={k: sched[k] for k in ("ns", "nf", "parent", "unknown_node")})
            s = _state(N, sh.L)
            res["Dz"] = run("apply_D_global", A.apply_D_global, l, s)
            a, rhs = _matrix_a(rp, ci, sh.L), _rhs(N, sh.L)
            owner = None
            for case in sh.cases:
                if abort():
                    res["skipped"].append(case)
                    continue
                if case == "A":
                    res["f0"] = run("f0", A.f0, l, s, T, True)
                    res["f1"] = run("f1", A.f1, l, s, T)
                    f2 = run("f2", A.f2, l, s, T)
                    res["f2"] = None if f2 is None else f2[1]
                elif case == "R":
                    run("f1_owner", A.f1_owner, l, s, T)
                    run("f2_local", A.f2_local, l, s, T)
                    run("solve_linear_local", A.solve_linear_local, l, a, rhs[0])
                elif case == "B":
                    pass      # tables only: the parent works on info, tree and the kinds of C
                elif case == "C":
                    got = run("f1_owner", A.f1_owner, l, s, T)
                    res["f1_owner"] = got
                    kinds = gather(got[2] if got is not None else np.zeros(N, dtype=np.int32))
                    res["kinds"] = kinds
                    owner = run("owner_of", SR.owner_of, kinds)
                    if owner is None and not res["errors"]:
                        res["errors"].append("no owner table")
                elif case == "D":
                    res["f2_local"] = run("f2_local", A.f2_local, l, s, T)
                elif case in "EF":
                    if case == "E":
                        mine = SR.split_shares(rp, ci, a, owner, world, seed=7 + sh.L)[rank]
                    else:
                        mine = res["f2_local"]
                    kind = res["kinds"][rank]
                    sols = []
                    for gk in rhs:
                        sols.append(run("solve_linear_local " + case, A.solve_linear_local, l, mine, np.where(kind == 0, POISON, gk)))
                    res[case] = sols
                elif case == "G":
                    mats = [("a", a)] + ([("c", res["f2"])] if res.get("f2") is not None else [])
                    res["G"] = {nm: [run("solve_linear " + nm, A.solve_linear, l, m, gk, "gpu") for gk in rhs] for nm, m in mats}
                elif case in "Hh":
                    if owner is None:      # geometric tree: no kind table is handed out there
                        owner = SR.geometric_node_owner(sched["parent"], world)[sched["unknown_node"]]
                    picks = _picks(owner, world)
                    res["picks"] = picks
                    diag = CR.diagonal_positions(rp, ci)
                    if case == "H":
                        shares = SR.split_shares(rp, ci, a, owner, world, seed=7 + sh.L)
                        flags = []
                        for u in picks:
                            bad, _ = SR.set_diagonal_share(rp, ci, shares, owner, u, -1.0, owner[u] if owner[u] >= 0 else 1 % world)
                            got = run("solve_linear_local H", A.solve_linear_local, l, bad[rank], rhs[0])
                            flags.append(None if got is None else got[2])
                        res["H_flags"] = flags
                        res["H_again"] = run("solve_linear_local again", A.solve_linear_local, l, shares[rank],
                                             np.where(res["kinds"][rank] == 0, POISON, rhs[0]))
                    codes = []
                    for k, u in enumerate(picks):
                        bad = a.copy()
                        bad[diag[u]] = -1.0
                        res["codes"].pop("pivot", None)
                        run("pivot", A.solve_linear, l, bad, rhs[0], "gpu")
                        codes.append(res["codes"].pop("pivot", 0))
                    res["H_codes"] = codes
                    res["H_summed_again"] = run("solve_linear again", A.solve_linear, l, a, rhs[0], "gpu")
            res["seconds"] = time.time() - t0
            out[sh.key] = res
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn(world, aligned, shapes):
    """One spawn of `world` workers; the parent waits GROUP_TIMEOUT, fails on a timeout or a non-zero exit code and leaves nothing
    running."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() * 7 + 13 + world) % 2000
    # read once per process, so set around the spawn: the tree mode, and the 16 CPUs of a job shared out among the ranks (every
    # rank would otherwise start 16 threads each for the host analysis, BLAS and OpenMP: 128 threads on 16 cores at 8 ranks)
    env = {"MGB_RANK_ALIGNED": aligned}
    env.update({k: str(max(1, 16 // world)) for k in ("MGB_NUM_THREADS", "OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS")})
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, shapes)) for r in range(world)]
    t0 = time.time()
    try:
        for p in procs:
            p.start()
        out, problem = [], None
        while len(out) < world and problem is None:
            try:
                out.append(q.get(timeout=1.0))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead:
                    problem = "a worker ended with exit code %s" % dead
                elif time.time() - t0 > GROUP_TIMEOUT:
                    problem = "no result after %.0f s" % GROUP_TIMEOUT
        if problem is None:
            for p in procs:
                p.join(timeout=max(1.0, GROUP_TIMEOUT - (time.time() - t0)))
                if p.exitcode != 0:
                    problem = "a worker ended with exit code %s" % p.exitcode
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
    assert problem is None, problem
    return [o[1] for o in sorted(out, key=lambda o: o[0])], time.time() - t0


# ---------------------------------------------------------------------------------------------------------- parent
_REF = {}


def _reference(sh):
    """Parent side of a shape, once: the unsharded device problem (apply_D, pattern), the host matrices, and where the shape has
    a dense reference the oracle's level baseline."""
    if sh.key in _REF:
        return _REF[sh.key]
    import mgb_amd as M
    gm = getattr(M, sh.kind + "_mpi")(sh.L)
    dim = gm.discretization["dim"]
    A = M.AMG(gm, p=P)
    x = gm.x.to_numpy()
    c, z0 = M._rows(M.DEFAULT_F[dim], x), M._rows(M.DEFAULT_G[dim], x)
    A.set_c(c)
    A.set_z(z0.reshape(-1, order="F"))
    l = A.L - 1
    N, nz = A.level_size(l)
    rp, ci = A.hessian_pattern(l)
    s = _state(N, sh.L)
    ops = {k: v.host for k, v in gm.operators.items()}
    subs = {k: [m.host for m in v] for k, v in gm.subspaces.items()}
    _, B = BR.level_matrices(ops, subs, A.state_variables, A.D, l, A.n)
    R = types.SimpleNamespace(N=N, nz=nz, rp=rp, ci=ci, s=s, B=B, K=A.K, n=A.n, w=gm.w.to_numpy(), c=c, Dz=A.apply_D(l, s),
                              terms=BR.default_terms(dim, P), rows=np.repeat(np.arange(N), np.diff(rp)), a=_matrix_a(rp, ci, sh.L),
                              rhs=_rhs(N, sh.L), base=(1.0, 1.0, 1.0))
    if sh.ref == "full":
        import scipy.sparse as sp
        Rl = sp.block_diag([sp.csr_matrix((A.n, 0)) if sv[1] == "fixed" else subs[sv[1]][l] for sv in A.state_variables], format="csr")
        z = z0 + (Rl @ s).reshape(A.n, len(A.state_variables), order="F")
        Mo = O.amg(getattr(O, sh.kind)(sh.L))
        r0, r1, r2, _ = BR.oracle_level_baseline(Mo, l, z, c, T, R.terms)
        R.base = (r0, r1, r2)
    _REF[sh.key] = R
    return R


class _Book:
    """failures and the worst ratio per (shape, label), printed as the profile's table"""

    def __init__(self, group):
        self.group, self.failures, self.rows, self.worst = group, [], [], 0.0

    def check(self, ok, shape, what):
        if not ok:
            self.failures.append("%s | %s: %s" % (self.group, shape, what))

    def ratio(self, shape, label, value, base=1.0, limit=None):
        """a ratio held to MARGIN * max(base, 1) (limit None) or to `limit` itself"""
        bound = MARGIN * max(base, 1.0) if limit is None else limit
        if limit is None:
            self.worst = max(self.worst, value / max(base, 1.0))
        self.rows.append((shape, label, value, base, bound))
        self.check(value <= bound, shape, "%s: ratio %.3g beyond %.3g (baseline %.3g)" % (label, value, bound, base))

    def solution(self, shape, label, ref, x, g, sol):
        """x against chol_reference's bounds: eta always, phi where the reference is exact (sol None: eta <= 16 u alone)"""
        self.check(np.all(np.isfinite(x)), shape, label + ": x is not finite")
        if sol is None:
            eta = ref.eta(x, g)
            self.rows.append((shape, label + " eta/u", eta / CR.U, 1.0, CR.MARGIN))
            self.check(eta <= CR.MARGIN * CR.U, shape, "%s: eta %.3e" % (label, eta))
            return
        r = ref.metrics(x, g, sol)
        self.rows.append((shape, label + " eta", r["eta_ratio"], 1.0, CR.MARGIN))
        self.check(r["eta_ok"], shape, "%s: eta %.3e against baseline %.3e" % (label, r["eta"], r["eta_base"]))
        if r["exact"]:
            self.rows.append((shape, label + " phi", r["phi_ratio"], 1.0, CR.MARGIN))
            self.check(r["phi_ok"], shape, "%s: phi %.3e against baseline %.3e" % (label, r["phi"], r["phi_base"]))

    def report(self, seconds, shape_seconds):
        print()
        for shape, label, value, base, bound in self.rows:
            print("%-18s %-10s %-34s %8.3f  (baseline %.2f, held to %g)" % (self.group, shape, label, value, base, bound))
        print("%-18s worst ratio / max(baseline, 1): %.3f   MARGIN %g   group %.1f s (%s)" % (
            self.group, self.worst, MARGIN, seconds, ", ".join("%s %.1f s" % kv for kv in shape_seconds.items())))


def _same(arrs):
    return all(a is not None and np.array_equal(a, arrs[0]) for a in arrs)


def _assemble(vecs, owner):
    """the vector every unknown's owner holds (top entries from rank 0)"""
    vecs = np.asarray(vecs)
    return vecs[np.where(owner < 0, 0, owner), np.arange(vecs.shape[1])]


def _check_shape(book, world, aligned, sh, ranks):
    key = sh.key
    R = _reference(sh)
    r0 = ranks[0]
    for r, res in enumerate(ranks):
        book.check(not res["errors"] and not res["skipped"], key, "rank %d: errors %s, skipped %s" % (r, res["errors"], res["skipped"]))
    if any(res["errors"] or res["skipped"] for res in ranks):
        return
    N, rp, ci, rows = R.N, R.rp, R.ci, R.rows
    book.check(r0["N"] == N and np.array_equal(r0["rp"], rp) and np.array_equal(r0["ci"], ci), key, "pattern differs from the unsharded one")
    book.check(all(res["info"]["split_world"] == world and res["info"]["values_local"] == aligned for res in ranks), key,
               "chol_info: %s" % [res["info"] for res in ranks])
    book.check(all(np.array_equal(res["Dz"], R.Dz) for res in ranks), key, "apply_D_global differs from the unsharded apply_D")
    Lv = BR.level_reference(R.B, R.K, R.w, R.c, T, R.Dz, R.terms, hessian=sh.ref == "full" and bool(set("AD") & set(sh.cases)))
    book.check(bool(Lv.rows.feasible.all() and Lv.rows.in_range.all()), key, "state outside the cone")
    b0, b1, b2 = R.base
    tree = r0["tree"]
    book.check(all(np.array_equal(res["tree"][k], tree[k]) for res in ranks for k in tree), key, "trees differ between the ranks")
    ref_a = sols_a = None
    if set("EGHh") & set(sh.cases):
        ref_a = CR.Reference(rp, ci, R.a, N, factor=sh.ref == "full")
        sols_a = [ref_a.solve(g) if sh.ref == "full" else None for g in R.rhs]
    owner = None
    if "C" in sh.cases:
        kinds = r0["kinds"]
        try:
            owner = SR.owner_of(kinds)
        except ValueError as e:
            book.check(False, key, "B kind tables: %s" % e)
            return
        book.check(all(np.array_equal(res["kinds"][r], res["f1_owner"][2]) for r, res in enumerate(ranks)), key, "kinds gathered wrongly")
    else:
        owner = SR.geometric_node_owner(tree["parent"], world)[tree["unknown_node"]]
    # ---- coverage from the device's own tree
    nodeown = SR.node_owner(tree["ns"], tree["parent"], tree["unknown_node"], owner)
    roots = SR.subtree_roots(tree["nf"], tree["ns"], tree["parent"], nodeown)
    ntop, ntop_vals = int((owner < 0).sum()), SR.top_value_count(rp, ci, owner)
    want_x = SR.exchange_doubles(roots, ntop_vals) if aligned else SR.exchange_doubles(roots, 0) + N + 1
    print("%-18s %-10s N %5d  roots nb %s  top unknowns %d  top values %d  exchange_doubles %d" % (
        book.group, key, N, [nb for _, _, nb in roots], ntop, ntop_vals, r0["info"]["exchange_doubles"]))
    book.check(len(roots) == world and sorted(r for _, r, _ in roots) == list(range(world)), key, "subtree roots %s" % roots)
    book.check(all(res["info"]["exchange_doubles"] == want_x for res in ranks), key,
               "B exchange_doubles %s, from the tree %d" % (r0["info"]["exchange_doubles"], want_x))
    cover = dict(nb64=max(nb for _, _, nb in roots) > 64, top256=ntop > 256, vals256=ntop_vals > 256, ride3=ntop_vals >= 3)
    for c in sh.need:
        book.check(cover[c], key, "coverage condition %s not met: nb %s, top %d, top values %d" % (c, [nb for _, _, nb in roots], ntop, ntop_vals))
    if "A" in sh.cases:
        for nm in ("f0", "f1", "f2"):
            book.check(all(nm not in res["codes"] for res in ranks), key, "A %s raised %s" % (nm, r0["codes"]))
        book.check(_same([res["f0"][1] for res in ranks]) and _same([res["f1"] for res in ranks]) and _same([res["f2"] for res in ranks]),
                   key, "A: results differ between the ranks")
        book.ratio(key, "A f0 F", BR.ratio(r0["f0"][1][0], Lv.f0F, Lv.b_f0F), b0)
        book.ratio(key, "A f0 c.Dz", BR.ratio(r0["f0"][1][1], Lv.f0C, Lv.b_f0C), b0)
        book.ratio(key, "A f0", BR.ratio(r0["f0"][0], *BR.f0_total(Lv, T)), b0)
        book.ratio(key, "A f1", BR.ratio(r0["f1"], Lv.g, Lv.b_g), b1)
        if sh.ref == "full":
            inside = np.zeros((N, N), dtype=bool)
            inside[rows, ci] = True
            book.check(not np.any(np.tril(Lv.H_abs != 0) & ~inside), key, "H has entries outside the pattern")
            book.ratio(key, "A f2", BR.ratio(r0["f2"], Lv.H[rows, ci], Lv.b_H[rows, ci]), b2)
    if "R" in sh.cases:
        for nm in ("f1_owner", "f2_local", "solve_linear_local"):
            book.check(all(res["codes"].get(nm) == E_ARG for res in ranks), key, "R %s: codes %s" % (nm, [res["codes"].get(nm) for res in ranks]))
    if "B" in sh.cases:
        foreign = (owner[rows] >= 0) & (owner[ci] >= 0) & (owner[rows] != owner[ci])
        book.check(not foreign.any(), key, "B: %d pattern entries couple kind-1 unknowns of two ranks" % int(foreign.sum()))
    if "C" in sh.cases:
        kinds = r0["kinds"]
        gs = [res["f1_owner"][0] for res in ranks]
        for r in range(world):
            m = kinds[r] >= 1
            book.ratio(key, "C g rank %d" % r, BR.ratio(gs[r][m], Lv.g[m], Lv.b_g[m]), b1)
        book.check(_same([g[owner < 0] for g in gs]), key, "C: top entries of g differ between the ranks")
        G = _assemble(gs, owner)
        book.check(_same([np.float64(res["f1_owner"][1]) for res in ranks]), key, "C: |g|^2 differs between the ranks")
        book.ratio(key, "C |g|^2", SR.dot_ratio(r0["f1_owner"][1], G, G, world), limit=1.0)
    if "D" in sh.cases:
        loc = np.array([res["f2_local"] for res in ranks])
        kinds = r0["kinds"]
        book.ratio(key, "D sum f2_local", BR.ratio(loc.astype(LD).sum(axis=0), Lv.H[rows, ci], Lv.b_H[rows, ci]), b2)
        for r in range(world):
            gone = (kinds[r][rows] == 0) | (kinds[r][ci] == 0)
            book.check(not np.any(loc[r][gone] != 0), key, "D: rank %d holds values on entries with a foreign endpoint" % r)
        toptop = (owner[rows] < 0) & (owner[ci] < 0)
        book.check(bool(np.any(np.count_nonzero(loc[:, toptop], axis=0) >= 2)), key, "D: no top entry is shared by two ranks")
    for case in "EF":
        if case not in sh.cases:
            continue
        kinds = r0["kinds"]
        toptop = (owner[rows] < 0) & (owner[ci] < 0)
        if case == "E":
            shares = SR.split_shares(rp, ci, R.a, owner, world, seed=7 + sh.L)
            book.check(SR.shares_exact(shares, R.a) and SR.foreign_weight(rp, ci, shares, owner) == 0.0, key, "E: the shares are not exact")
            ref, sols, exact_vals = ref_a, sols_a, R.a
        else:
            shares = np.array([res["f2_local"] for res in ranks])
            summed = np.zeros(R.nz)
            for sv in shares:
                summed = summed + sv
            ref = CR.Reference(rp, ci, summed, N)
            sols, exact_vals = [ref.solve(g) for g in R.rhs], None
        for k, g in enumerate(R.rhs):
            got = [res[case][k] for res in ranks]
            book.check(all(o is not None for o in got), key, "%s: solve_linear_local raised %s" % (case, r0["codes"]))
            if any(o is None for o in got):
                continue
            xs = [o[0] for o in got]
            for r in range(world):
                book.check(not np.any(xs[r][kinds[r] == 0] != 0), key, "%s rhs %d: x of rank %d is not zero where kind = 0" % (case, k, r))
            book.check(_same([x[owner < 0] for x in xs]), key, "%s rhs %d: top part of x differs between the ranks" % (case, k))
            X = _assemble(xs, owner)
            book.solution(key, "%s rhs %d" % (case, k), ref, X, g, sols[k])
            book.check(_same([np.float64(o[1]) for o in got]), key, "%s rhs %d: <g, x> differs between the ranks" % (case, k))
            book.ratio(key, "%s rhs %d <g,x>" % (case, k), SR.dot_ratio(got[0][1], g, X, world), limit=1.0)
            book.check(all(o[2] == 0 for o in got), key, "%s rhs %d: flags %s" % (case, k, [o[2] for o in got]))
            for r in range(world):
                after = got[r][3]
                book.check(np.array_equal(after[~toptop], shares[r][~toptop]), key, "%s rhs %d: rank %d's values changed outside the top" % (case, k, r))
                if exact_vals is not None:
                    book.check(np.array_equal(after[toptop], exact_vals[toptop]), key, "%s rhs %d: rank %d's top values are not the exact sums" % (case, k, r))
                else:
                    book.check(np.array_equal(after[toptop], ranks[0][case][k][3][toptop]), key, "%s rhs %d: top values differ between the ranks" % (case, k))
    if "G" in sh.cases:
        for nm in r0["G"]:
            if nm == "a":
                ref, sols = ref_a, sols_a
            else:
                ref = CR.Reference(rp, ci, r0["f2"], N)
                sols = [ref.solve(g) for g in R.rhs]
            for k, g in enumerate(R.rhs):
                xs = [res["G"][nm][k] for res in ranks]
                book.check(_same(xs), key, "G (%s) rhs %d: x differs between the ranks or raised %s" % (nm, k, r0["codes"]))
                if xs[0] is not None:
                    book.solution(key, "G (%s) rhs %d" % (nm, k), ref, xs[0], g, sols[k])
        book.check(sh.ref != "full" or "c" in r0["G"] or "A" not in sh.cases, key, "G: (c) was not run")
    if set("Hh") & set(sh.cases):
        picks = r0["picks"]
        book.check(owner[picks[0]] == world - 1 and owner[picks[1]] < 0 and owner[picks[2]] == 0, key, "H: picks %s" % picks)
        if "H" in sh.cases:
            book.check(all(res["H_flags"] == [1, 1, 1] for res in ranks), key, "H: flags %s" % [res["H_flags"] for res in ranks])
            for r, res in enumerate(ranks):
                again, first = res["H_again"], res["E"][0]
                book.check(again is not None and first is not None and np.array_equal(again[0], first[0]) and again[1] == first[1]
                           and again[2] == 0, key, "H: rank %d's (a') after the pivot failures is not the first solution" % r)
        book.check(all(res["H_codes"] == [E_NUMERIC] * 3 for res in ranks), key, "H summed: codes %s" % [res["H_codes"] for res in ranks])
        first = r0["G"]["a"][0] if "G" in sh.cases else None
        xs = [res["H_summed_again"] for res in ranks]
        book.check(_same(xs) and (first is None or np.array_equal(xs[0], first)), key, "H summed: (a') after the pivot failures is not the first solution")
        if first is None and xs[0] is not None:
            book.solution(key, "H summed again", ref_a, xs[0], R.rhs[0], sols_a[0])


@pytest.mark.parametrize("group", list(GROUPS))
def test_sharded_step_against_exact_references(gpu_required, group):
    world, mode, shapes = GROUPS[group]
    for sh in shapes:
        _reference(sh)      # before the spawn: the parent's own device work is not part of the group's time
    out, seconds = _spawn(world, mode, shapes)
    book = _Book(group)
    for sh in shapes:
        _check_shape(book, world, mode == "1", sh, [o[sh.key] for o in out])
    book.report(seconds, {sh.key: max(o[sh.key]["seconds"] for o in out) for sh in shapes})
    assert not book.failures, "\n".join(book.failures)


def test_owner_local_entry_points_refuse_an_unsharded_context(gpu_required):
    import mgb_amd as M
    from mgb_amd._lib import MGBError
    A = M.AMG(M.fem1d_mpi(3), p=P)
    N, nz = A.level_size(A.L - 1)
    for call in (lambda: A.f1_owner(A.L - 1, np.zeros(N), T), lambda: A.f2_local(A.L - 1, np.zeros(N), T),
                 lambda: A.solve_linear_local(A.L - 1, np.ones(nz), np.ones(N))):
        with pytest.raises(MGBError) as e:
            call()
        assert e.value.code == E_ARG and "sharded contexts only" in str(e.value)
