#!/usr/bin/env python3
"""sha256 of every raw output buffer of the Newton-path kernels (csrc/devutil.hpp, kernels_tpl.hpp, kernels.hip, kernels_f32.hip,
mg.hip) on seeded inputs, through the Python API only -- the run behind profiles/newton_kernels_refactor_bits.txt.

  python3 tools/newton_kernel_bits.py run TREE OUT      hash the library of the checkout at TREE (a fresh process per tree)
  python3 tools/newton_kernel_bits.py compare PARENT HEAD   the table of two such files; exit status 1 unless every pair is equal

Lines of OUT:  "lib <path in TREE> sha256 <of the library file that ran>",  "hash <name>\t<sha256>"  and
"path <mesh> level <l>: ..." -- the lanes per row of B = D R (csrc/amg.cpp pick_group, restated by
linesearch_reference.pick_group) and whether apply_D runs the element-local kernel (the rule of DevElCsrOwned::build and its
caller build_level, restated in el_path below), so that a reader sees which instantiations ran."""
import hashlib
import os
import sys

import numpy as np
import scipy.sparse as sp

FUSED_TRIAL_ROWS = 64 * 2048      # csrc/amg.hpp fused_trial_rows_: apply_D goes element-local only on meshes beyond it


def el_path(B, n, K, block):
    """csrc/amg.cpp build_level + DevElCsrOwned::build: the element-local view of B exists iff the mesh is beyond the fused line
    search, the rows come in whole elements, an element's distinct columns fit a 1-byte index and each staged x entry serves at
    least two nonzeros on average."""
    if not (n > FUSED_TRIAL_ROWS and block > 1 and n % block == 0):
        return False
    rpe = block * K
    B = sp.csr_matrix(B)
    if rpe < 2 or B.shape[0] == 0 or B.shape[0] % rpe:
        return False
    nel = B.shape[0] // rpe
    cmax = max(len(np.unique(B.indices[B.indptr[e * rpe]:B.indptr[(e + 1) * rpe]])) for e in range(nel))
    return 1 <= cmax <= 255 and nel * cmax * 2 <= B.nnz


class Run:
    def __init__(self, tree, out):
        for p in (tree, os.path.join(tree, "oracle"), os.path.join(tree, "tests")):
            sys.path.insert(0, p)
        import mgb_amd
        import mgb_oracle
        import barrier_reference
        import linesearch_reference
        self.M, self.O, self.BR, self.LR = mgb_amd, mgb_oracle, barrier_reference, linesearch_reference
        self.out = open(out, "w")
        from mgb_amd import _lib
        assert os.path.realpath(_lib.LIB_PATH).startswith(os.path.realpath(tree) + os.sep), _lib.LIB_PATH      # this tree's library
        self.out.write("lib %s sha256 %s\n" % (os.path.relpath(_lib.LIB_PATH, tree),
                                                hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()))

    def put(self, name, *bufs):
        h = hashlib.sha256()
        for b in bufs:
            b = np.ascontiguousarray(np.asarray(b))
            h.update(str((b.dtype.str, b.shape)).encode())
            h.update(b.tobytes())
        self.out.write("hash %s\t%s\n" % (name, h.hexdigest()))
        self.out.flush()

    def note(self, text):
        self.out.write("path %s\n" % text)
        self.out.flush()

    # ------------------------------------------------------------------------------------------------ one mesh, every level
    def mesh(self, tag, kind, L, p, levels=None, full=True, **kw):
        M, O = self.M, self.O
        gm = getattr(M, kind + "_mpi")(L, **kw)
        dim = gm.discretization["dim"]
        x = gm.x.to_numpy()
        A = M.AMG(gm, p=p)
        z0 = O.map_rows(lambda xi: O.DEFAULT_G[dim](xi), x)
        A.set_c(O.map_rows(lambda xi: O.DEFAULT_F[dim](xi), x))
        A.set_z(np.asarray(z0).reshape(-1, order="F"))
        self.put("%s n=%d K=%d levels=%d" % (tag, A.n, A.K, A.L), x, gm.w.to_numpy())
        ops = {k: v.host for k, v in gm.operators.items()}
        subs = {k: [m.host for m in v] for k, v in gm.subspaces.items()}
        block = int(gm.discretization.get("block", 1))      # nodes per element of the broken space
        for l in (range(A.L) if levels is None else levels):
            N = A.level_size(l)[0]
            B = self.BR.level_matrices(ops, subs, A.state_variables, A.D, l, A.n)[1]
            info = A.elop_info(l)
            self.note("%s level %d: N=%d  lanes per row of B %d  apply_D %s  element operator %s" % (
                tag, l, N, self.LR.pick_group(B), "element-local" if el_path(B, A.n, A.K, block) else "plain CSR",
                "tpe=%d%s" % (info["tpe"], " pipelined" if info["pipelined"] else "") if info["valid"] else "none"))
            rng = np.random.default_rng(1000 * L + 10 * l + dim)
            s, nstep, v, g = (rng.standard_normal(N) for _ in range(4))
            s *= 2e-3
            nstep *= 1e-3
            pre = "%s l=%d " % (tag, l)
            self.put(pre + "apply_D", A.apply_D(l, s))
            y, parts = A.f0(l, s, 3.7, parts=True)
            self.put(pre + "f0 with parts", np.float64(y), parts)
            self.put(pre + "f0_trial", np.float64(A.f0_trial(l, s, s + 0.5 * nstep, 3.7)))
            phi0 = A.trial_set(l, s, None, [0.0])["phi"][0]
            for alphas in ((-1.0,), (-1.0, -0.5), (-1.0, -0.5, -0.25)):
                # the rule against the distances at s (it passes), and against 20 times those (frac = 0.1: it fires in every row)
                for rule, ref in (("no rule", None), ("phi_ref", phi0), ("phi_ref x 20", 20.0 * phi0)):
                    for mode in ("set", "separate", "unfused"):
                        o = A.trial_set(l, s, nstep, alphas, phi_ref=ref, mode=mode)
                        self.put(pre + "trial_set na=%d %s %s" % (len(alphas), rule, mode),
                                 o["dz"], o["phi"], o["sums"], o["sums_host"], o["s_out"])
            self.put(pre + "f1", A.f1(l, s, 3.7))
            if not full:
                continue
            self.put(pre + "f2", A.f2(l, s, 3.7)[1])
            s32 = s.astype(np.float32)
            self.put(pre + "f0_f32", np.float64(A.f0_f32(l, s32, 3.7)))
            self.put(pre + "f1_f32", A.f1_f32(l, s32, 3.7))
            self.put(pre + "f2_f32", A.f2_f32(l, s32, 3.7))
            self.put(pre + "f1_template_f64", A.f1_template_f64(l, s, 3.7))
            self.put(pre + "f2_template_f64", A.f2_template_f64(l, s, 3.7))
            self.put(pre + "hessian_apply matrix-free", A.hessian_apply(l, s, v, matrix_free=True))
            self.put(pre + "hessian_apply assembled", A.hessian_apply(l, s, v, matrix_free=False))
            xs, lam = A.smooth(l, s, g, degree=3, sweeps=2, lmax=0.0, matrix_free=True)
            self.put(pre + "smooth", xs, np.float64(lam))
            A.set_pcg(rtol=1e-10, maxit=200)
            xp, it, rr, ok = A.pcg_solve_linear(l, s, A.f1(l, s, 3.7))
            self.put(pre + "pcg_solve_linear", xp, np.int64(it), np.float64(rr), np.int64(ok))
        return A, gm

    def nodal_exponents(self):
        """fem2d L=3 with one exponent per node (mgb_amg_set_exponents): the a_node / mu_node path of cone_am."""
        M, O = self.M, self.O
        gm = M.fem2d_mpi(3)
        x = gm.x.to_numpy()
        pn = 1.25 + 0.5 * (0.5 + 0.5 * np.sin(3.0 * x[:, 0] + 5.0 * x[:, 1]))
        A = M.AMG(gm, p=pn)
        A.set_c(O.map_rows(lambda xi: O.DEFAULT_F[2](xi), x))
        A.set_z(np.asarray(O.map_rows(lambda xi: O.DEFAULT_G[2](xi), x)).reshape(-1, order="F"))
        for l in range(A.L):
            N = A.level_size(l)[0]
            rng = np.random.default_rng(77 + l)
            s, nstep = 2e-3 * rng.standard_normal(N), 1e-3 * rng.standard_normal(N)
            pre = "fem2d L=3 nodal p l=%d " % l
            y, parts = A.f0(l, s, 2.0, parts=True)
            self.put(pre + "f0 with parts", np.float64(y), parts)
            o = A.trial_set(l, s, nstep, (-1.0, -0.5, -0.25))
            self.put(pre + "trial_set na=3", o["dz"], o["phi"], o["sums"], o["sums_host"])
            self.put(pre + "f1", A.f1(l, s, 2.0))
            self.put(pre + "f2", A.f2(l, s, 2.0)[1])
            self.put(pre + "f0_f32", np.float64(A.f0_f32(l, s.astype(np.float32), 2.0)))
            self.put(pre + "hessian_apply matrix-free", A.hessian_apply(l, s, nstep))

    def barrier_rows(self):
        """map_rows of the barrier's F and F2 through barrier_functions (barrier_rows_F_kernel, expand_hessian_rows_kernel)."""
        M = self.M
        rng = np.random.default_rng(5)
        for name, K, cones in (("power cone p=1.5", 4, [([1, 2, 3], 1.5)]),
                               ("cone + half space", 4, [([1, 2, 3], 1.0), ("linear", [0], [1.0], 0.4)])):
            n = 1000
            Dz = 0.3 * rng.standard_normal((n, K))
            Dz[:, 3] = 1.0 + np.abs(Dz[:, 3])
            Dz[::50, 3] = -1.0      # rows outside the domain: +inf
            F, F1, F2 = M.barrier_functions(cones, K)
            hD = M.HPCMatrix(Dz)
            self.put("map_rows F " + name, M.map_rows(F, hD, hD).to_numpy())
            self.put("map_rows F1 " + name, M.map_rows(F1, hD, hD).to_numpy())
            self.put("map_rows F2 " + name, M.map_rows(F2, hD, hD).to_numpy())

    def reductions(self):
        M, LR = self.M, self.LR
        for n in LR.REDUCTION_SIZES:
            rng = np.random.default_rng(n)
            x, y = M.HPCVector(rng.standard_normal(n)), M.HPCVector(rng.standard_normal(n))
            self.put("HPCVector n=%d dot sum norm" % n, np.float64(x.dot(y)), np.float64(x.sum()), np.float64(x.norm()))
        for name, A, G in LR.spmv_cases():
            rng = np.random.default_rng(A.shape[0] + 7 * G)
            hA = M.HPCSparseMatrix(sp.csr_matrix(A * rng.standard_normal()))
            y = (hA @ M.HPCVector(rng.standard_normal(A.shape[1]))).to_numpy()
            self.put("HPCSparseMatrix @ %s (G=%d)" % (name, G), y)
            self.note("spmv case %s: lanes per row %d" % (name, G))

    def solve(self, tag, kind, L, **kw):
        M = self.M
        sol = M.amgb(getattr(M, kind + "_mpi")(L, **kw), p=1.5)
        self.put("amgb %s p=1.5: z and iteration counts" % tag, M.mpi_to_native(sol).z,
                 np.asarray(sol.SOL_main["its"], dtype=np.int64))


SMALL = (("fem1d L=4", "fem1d", 4, {}), ("fem2d L=3", "fem2d", 3, {}), ("fem3d L=1 k=3", "fem3d", 1, {"k": 3}))


def run(tree, out):
    r = Run(os.path.abspath(tree), out)
    for tag, kind, L, kw in SMALL:
        for p in (1.0, 1.5):
            r.mesh("%s p=%g" % (tag, p), kind, L, p, **kw)
    for p in (1.0, 1.5):
        r.mesh("fem2d L=6 p=%g" % p, "fem2d", 6, p)       # 14336 nodes: 56 blocks of the node kernels, both ticket levels
    # none of the meshes above is beyond the fused line search, so none takes the element-local apply_D: fem2d L=8 (229376
    # nodes) is the smallest fem2d mesh that does; its finest and coarsest level, the kernels that read Dz only
    r.mesh("fem2d L=8 p=1", "fem2d", 8, 1.0, levels=(0, 7), full=False)
    r.nodal_exponents()
    r.barrier_rows()
    r.reductions()
    for tag, kind, L, kw in SMALL:
        r.solve(tag, kind, L, **kw)
    r.out.write("done\n")


def compare(parent, head):
    def read(path):
        hashes, paths, done, lib = {}, [], False, "?"
        for line in open(path):
            line = line.rstrip("\n")
            if line.startswith("hash "):
                name, h = line[5:].split("\t")
                hashes[name] = h
            elif line.startswith("path "):
                paths.append(line[5:])
            elif line.startswith("lib "):
                lib = line[4:]
            elif line == "done":
                done = True
        return hashes, paths, done, lib
    hp, pp, dp, lp = read(parent)
    hh, ph, dh, lh = read(head)
    print("parent library: %s\nhead library:   %s\n" % (lp, lh))
    width = max(len(k) for k in list(hp) + list(hh))
    print("%-*s %-64s %-64s" % (width, "buffer", "parent", "head"))
    bad = 0 if (dp and dh and list(hp) == list(hh) and pp == ph) else 1
    for k in hp:
        same = hh.get(k) == hp[k]
        bad += not same
        print("%-*s %-64s %-64s %s" % (width, k, hp[k], hh.get(k, "missing"), "equal" if same else "DIFFERENT"))
    print()
    print("paths taken (the same in both runs)" if pp == ph else "PATHS DIFFER BETWEEN THE RUNS")
    for line in ph:
        print("  " + line)
    print()
    print("all %d pairs equal" % len(hp) if not bad else "NOT ALL PAIRS EQUAL (or a run did not finish)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
