"""multigridbarriermpi.jl_amd -- MI355X-native multigrid-barrier Newton path.

Host-side mirror (Python, because no Julia toolchain exists in the build image) of the operator
surface of sloisel/MultiGridBarrierMPI.jl, on top of the C ABI in ``include/mgb_hip.h``
(``lib/libmgb_hip.so``, hand-written HIP for gfx950).  Names, argument meaning and error behaviour
follow the reference (src = /root/reference/src/MultiGridBarrierMPI.jl):

  fem1d_mpi / fem2d_mpi                 src:559-565, 626-632
  fem1d_mpi_solve / fem2d_mpi_solve     src:594-600, 661-667
  native_to_mpi / mpi_to_native         src:259-338, 355-517
  amgb (re-export)                      src:748-752
  hooks amgb_zeros, amgb_all_isfinite, amgb_diag, amgb_blockdiag, map_rows, map_rows_gpu,
        _raw_array, _to_cpu_array       src:66-192

There is NO CPU fallback: every entry point that computes needs the HIP library and a GPU and
raises otherwise.  (The importable alias of this package is ``mgb_amd``; the directory name
contains a dot and cannot be imported directly.)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import MGBError, call, dptr, f64, i32, iptr, u8ptr

import ctypes as C

__all__ = [
    "fem1d", "fem2d", "fem3d", "fem1d_mpi", "fem2d_mpi", "fem3d_mpi", "fem1d_mpi_solve", "fem2d_mpi_solve",
    "fem3d_mpi_solve", "parabolic_solve", "ParabolicSOL", "native_to_mpi",
    "mpi_to_native", "amgb", "Geometry", "AMGBSOL", "HPCVector", "HPCMatrix", "HPCSparseMatrix",
    "backend_hip", "amgb_zeros", "amgb_all_isfinite", "amgb_diag", "amgb_blockdiag", "map_rows", "map_rows_gpu",
    "_raw_array", "_to_cpu_array", "MGBError", "device_count", "AMG", "amg", "hcat", "BarrierFn", "barrier_functions",
    "interpolate", "sample_grid", "norms", "error", "convergence", "FieldNorms", "Convergence",
    "energy", "flux", "Energy", "level_sets", "LevelSets", "isosurfaces", "Isosurfaces", "flow_lines", "FlowLines",
    "path_lines", "PathLines", "sections", "Sections", "line_integrals", "project", "LineIntegrals", "boundary", "boundary_flux", "Boundary", "BoundaryFlux",
    "dirichlet_on", "neumann_load", "NeumannLoad",
    "interior", "InteriorFacets", "estimate", "ErrorIndicators", "mark", "refine_triangles", "adapt",
    "estimate_steps", "StepIndicators", "refine_times", "adapt_time", "time_stats", "TimeStats",
]


def device_count() -> int:
    return int(_lib.load().mgb_device_count())


# --------------------------------------------------------------------------- backend / context


class HPCBackend:
    """One GPU + one stream (replaces HPCBackend{T,Ti,Device,Comm,Solver}, src:84-114)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        call("mgb_ctx_create", int(device), C.byref(h))
        self.handle = h
        self.device = device

    def synchronize(self):
        call("mgb_ctx_synchronize", self.handle)

    rank, world = 0, 1

    def set_comm(self, rank: int, world: int, allreduce):
        """Row-block sharding over `world` ranks (one process + GPU per rank), the
        counterpart of the reference's MPI.COMM_WORLD (src:125).  `allreduce(ptr, count)` must sum-allreduce
        `count` fp64 values in place at the DEVICE pointer `ptr` over all ranks and return only when the
        result is visible to other streams; see `torch_allreduce`.  AMGs created afterwards on this backend
        keep only their rank's rows."""

        def thunk(_user, ptr, count):
            try:
                allreduce(int(ptr), int(count))
                return 0
            except Exception as exc:       # never let an exception cross the C boundary
                import sys
                print("mgb allreduce callback failed: %r" % (exc,), file=sys.stderr)
                return 1

        self._allreduce_cb = _lib.ALLREDUCE_FN(thunk)     # keep the trampoline alive
        call("mgb_ctx_set_comm", self.handle, int(rank), int(world), self._allreduce_cb, None)
        self.rank, self.world = int(rank), int(world)

    def set_comm_rccl(self, rank: int, world: int, unique_id: bytes):
        """The same sharding with a communicator the library owns (mgb_ctx_set_comm_rccl -> ncclCommInitRank): every
        collective of the Newton path is an ncclAllReduce on the context stream, no host synchronisation and no Python in the
        loop.  `unique_id` = the 128 bytes rank 0 got from `rccl_unique_id()`, handed to all ranks by the host's own channel
        (see `rccl_comm_from_torch`)."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of rccl_unique_id()")
        call("mgb_ctx_set_comm_rccl", self.handle, bytes(unique_id), int(rank), int(world))
        self._allreduce_cb = None
        self.rank, self.world = int(rank), int(world)

    def comm_stats(self):
        n, b = C.c_longlong(), C.c_double()
        call("mgb_ctx_comm_stats", self.handle, C.byref(n), C.byref(b))
        return dict(calls=n.value, bytes=b.value)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mgb_ctx_destroy(self.handle)
        except Exception:
            pass


def torch_allreduce(dist, device: int, group=None):
    """allreduce callback for HPCBackend.set_comm on top of torch.distributed (plumbing only): backend "nccl"
    (= RCCL over xGMI) reduces in place on the device buffer; any other backend (gloo) stages through the
    host, which is what the single-GPU / CPU rehearsals of the sharded path use."""
    import torch

    class _Raw:
        def __init__(self, ptr, count):
            self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False),
                                             "version": 2, "strides": None}

    on_device = dist.get_backend(group) == "nccl"
    views = {}      # (ptr, count) -> tensor view of the library's buffer: the same few buffers come back every Newton step

    def allreduce(ptr, count):
        t = views.get((ptr, count))
        if t is None:
            if len(views) > 256:
                views.clear()
            t = views[(ptr, count)] = torch.as_tensor(_Raw(ptr, count), device=torch.device("cuda", device))
        if on_device:
            dist.all_reduce(t, group=group)
        else:
            h = t.cpu()
            dist.all_reduce(h, group=group)
            t.copy_(h)
        torch.cuda.synchronize(device)

    return allreduce


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library (call on rank 0, broadcast the 128 bytes)."""
    buf = C.create_string_buffer(128)
    call("mgb_rccl_unique_id", buf)
    return buf.raw


def rccl_comm_from_torch(backend: "HPCBackend", dist, group=None):
    """Give `backend` a library-owned RCCL communicator over the ranks of a torch.distributed job: rank 0 draws the unique id,
    torch.distributed only broadcasts its 128 bytes (setup-time plumbing; nothing of torch stays in the Newton loop)."""
    import torch
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    dev = torch.device("cuda", backend.device) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    t = torch.zeros(129, dtype=torch.uint8, device=dev)      # 128 id bytes + "rank 0 got one": every rank reaches the broadcast
    if rank == 0:
        try:
            t = torch.tensor(list(rccl_unique_id()) + [1], dtype=torch.uint8, device=dev)
        except MGBError:
            pass
    dist.broadcast(t, src=0, group=group)
    raw = bytes(t.cpu().tolist())
    if raw[128] != 1:
        raise MGBError(-2, "rccl_comm_from_torch: rank 0 could not draw an RCCL unique id (librccl not available?)")
    backend.set_comm_rccl(rank, world, raw[:128])


_BACKENDS: Dict[int, HPCBackend] = {}


def backend_hip(device: int = 0) -> HPCBackend:
    """Cached backend instance per device (the reference caches GPU backends the same way, src:84-110)."""
    if device not in _BACKENDS:
        _BACKENDS[device] = HPCBackend(device)
    return _BACKENDS[device]


# --------------------------------------------------------------------------- device array types


class HPCVector:
    """Device fp64 vector (reference HPCVector: `.v` local storage, src:175)."""

    def __init__(self, v, backend: Optional[HPCBackend] = None):
        backend = backend or backend_hip()
        self.backend = backend
        h = C.c_void_p()
        if isinstance(v, (int, np.integer)):
            self.n = int(v)
            call("mgb_vec_create", backend.handle, self.n, None, C.byref(h))
        else:
            a = f64(np.asarray(v).reshape(-1))
            self.n = a.size
            call("mgb_vec_create", backend.handle, self.n, dptr(a), C.byref(h))
        self.handle = h

    def __len__(self):
        return self.n

    @property
    def shape(self):
        return (self.n,)

    def to_numpy(self) -> np.ndarray:
        out = np.empty(self.n)
        call("mgb_vec_download", self.handle, dptr(out))
        return out

    def __array__(self, dtype=None):
        a = self.to_numpy()
        return a if dtype is None else a.astype(dtype)

    def dot(self, other: "HPCVector") -> float:
        out = C.c_double()
        call("mgb_dot", self.handle, other.handle, C.byref(out))
        return out.value

    def norm(self) -> float:            # norm(x), tools/profile_scaling.jl:89-134
        out = C.c_double()
        call("mgb_norm", self.handle, C.byref(out))
        return out.value

    def sum(self) -> float:             # sum(x), tools/profile_barrier.jl:45-59
        out = C.c_double()
        call("mgb_sum", self.handle, C.byref(out))
        return out.value

    def __mul__(self, other):          # w .* y  (test/test_column_extract.jl:65)
        if isinstance(other, HPCVector):
            out = HPCVector(self.n, self.backend)
            call("mgb_mul", self.handle, other.handle, out.handle)
            return out
        return NotImplemented

    def __add__(self, other):
        out = HPCVector(self.n, self.backend)
        call("mgb_axpy", self.handle, 1.0, other.handle, out.handle)
        return out

    def __sub__(self, other):
        out = HPCVector(self.n, self.backend)
        call("mgb_axpy", self.handle, -1.0, other.handle, out.handle)
        return out

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mgb_vec_free(self.handle)
        except Exception:
            pass


class HPCMatrix:
    """Device dense n x k matrix, row-major (reference HPCMatrix: `.A`, src:176)."""

    def __init__(self, A, backend: Optional[HPCBackend] = None):
        A = f64(np.atleast_2d(np.asarray(A)))
        self.shape = A.shape
        self.backend = backend or backend_hip()
        self._v = HPCVector(A.reshape(-1), self.backend)

    def to_numpy(self) -> np.ndarray:
        return self._v.to_numpy().reshape(self.shape)

    def __array__(self, dtype=None):
        a = self.to_numpy()
        return a if dtype is None else a.astype(dtype)

    def column(self, j: int) -> HPCVector:   # y[:, j] -> HPCVector (test/test_column_extract.jl:50), on the device
        n, K = self.shape
        if not 0 <= j < K:
            raise IndexError("column index out of range")
        out = HPCVector(n, self.backend)
        call("mgb_col_extract", self._v.handle, n, K, int(j), out.handle)
        return out


def hpc_partition(m: int, world: int) -> np.ndarray:
    """1-based offsets of the balanced contiguous split of m rows over `world` ranks (first m mod world ranks hold
    one extra row) -- the shape of the reference's `row_partition` / `.partition` vectors (tools/profile_solve.jl:24).
    HPCSparseArrays' own rule is not vendored in the reference [UPSTREAM-UNVERIFIED]."""
    return np.array([1 + (m // world) * r + min(r, m % world) for r in range(world + 1)], dtype=np.int64)


def hpc_local_block(S, rank: int, world: int, Ti=np.int32) -> dict:
    """The fields rank `rank` of `world` holds for the sparse matrix S in the reference's distributed layout
    (HPCSparseMatrix fields src:216-221; local block as dumped by test/test_dump_matrices.jl:62-71): 1-based
    `row_partition` / `col_partition`, the sorted global ids `col_indices` of the columns the local rows touch, and
    the local rows as the CSC of the transposed block (`colptr` over local rows, `rowval` = compressed column index,
    `nzval`), 1-based like the Julia structs.  Host only; for interop and matrix captures."""
    assert 0 <= rank < world
    S = sp.csr_matrix(S)
    S.sort_indices()
    rpart, cpart = hpc_partition(S.shape[0], world), hpc_partition(S.shape[1], world)
    blk = S[rpart[rank] - 1:rpart[rank + 1] - 1]
    cols = np.unique(blk.indices)
    return dict(row_partition=rpart, col_partition=cpart, col_indices=(cols + 1).astype(Ti),
                colptr=(blk.indptr + 1).astype(Ti), rowval=(np.searchsorted(cols, blk.indices) + 1).astype(Ti),
                nzval=np.array(blk.data, dtype=np.float64), nrows_local=int(blk.shape[0]),
                ncols_compressed=int(cols.size), has_sorted_rows=True)


def hpc_from_local_blocks(blocks) -> sp.csr_matrix:
    """Inverse of `hpc_local_block`: stack the per-rank blocks (in rank order) back into one scipy CSR."""
    rpart, cpart = blocks[0]["row_partition"], blocks[0]["col_partition"]
    rows = []
    for b in blocks:
        ci = np.asarray(b["col_indices"], dtype=np.int64)[np.asarray(b["rowval"], dtype=np.int64) - 1] - 1
        rows.append(sp.csr_matrix((b["nzval"], ci, np.asarray(b["colptr"], dtype=np.int64) - 1),
                                  shape=(b["nrows_local"], int(cpart[-1]) - 1)))
    S = sp.vstack(rows, format="csr")
    assert S.shape[0] == int(rpart[-1]) - 1
    return S


class HPCSparseMatrix:
    """Device CSR matrix (reference HPCSparseMatrix local block, src:216-221).  The library keeps the structure it
    uploaded; `.host` / `to_scipy()` read it back through the C ABI (the reference gathers with
    SparseMatrixCSC(x), src:371).  `A @ B`, `A + B`, `A.T`, `hcat`, `amgb_blockdiag` are the library's setup-time
    sparse algebra (mgb_csr_spgemm / add / transpose / hcat / blockdiag), not scipy."""

    def __init__(self, S, backend: Optional[HPCBackend] = None):
        S = sp.csr_matrix(S, dtype=np.float64)
        S.sort_indices()
        S.sum_duplicates()
        self.shape = S.shape
        self.backend = backend or backend_hip()
        h = C.c_void_p()
        rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
        call("mgb_csr_create", self.backend.handle, S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va), C.byref(h))
        self.handle = h
        self._host = None

    @classmethod
    def _wrap(cls, handle, backend) -> "HPCSparseMatrix":
        out = cls.__new__(cls)
        r, c, nz = C.c_int(), C.c_int(), C.c_int()
        call("mgb_csr_dims", handle, C.byref(r), C.byref(c), C.byref(nz))
        out.shape, out.backend, out.handle, out._host = (r.value, c.value), backend, handle, None
        return out

    @property
    def host(self) -> sp.csr_matrix:
        """scipy copy of the matrix the library holds (fetched once through mgb_csr_get)."""
        if self._host is None:
            r, c, nz = C.c_int(), C.c_int(), C.c_int()
            call("mgb_csr_dims", self.handle, C.byref(r), C.byref(c), C.byref(nz))
            rp = np.empty(r.value + 1, dtype=np.int32)
            ci = np.empty(nz.value, dtype=np.int32)
            va = np.empty(nz.value)
            call("mgb_csr_get", self.handle, iptr(rp), iptr(ci), dptr(va))
            self._host = sp.csr_matrix((va, ci, rp), shape=(r.value, c.value))
        return self._host

    @property
    def nnz(self) -> int:
        nz = C.c_int()
        call("mgb_csr_dims", self.handle, None, None, C.byref(nz))
        return nz.value

    def __matmul__(self, x):
        if isinstance(x, HPCVector):                      # A * x  (test/test_nonsquare.jl:43)
            y = HPCVector(self.shape[0], self.backend)
            call("mgb_spmv", self.handle, x.handle, y.handle)
            return y
        if isinstance(x, HPCSparseMatrix):                # A * B  (test/test_basic_ops.jl:39,55)
            h = C.c_void_p()
            call("mgb_csr_spgemm", self.handle, x.handle, C.byref(h))
            return HPCSparseMatrix._wrap(h, self.backend)
        return NotImplemented

    def __add__(self, other):                             # A + B  (test/test_matrix_addition.jl:48-63)
        if not isinstance(other, HPCSparseMatrix):
            return NotImplemented
        h = C.c_void_p()
        call("mgb_csr_add", self.handle, 1.0, other.handle, C.byref(h))
        return HPCSparseMatrix._wrap(h, self.backend)

    def __sub__(self, other):
        if not isinstance(other, HPCSparseMatrix):
            return NotImplemented
        h = C.c_void_p()
        call("mgb_csr_add", self.handle, -1.0, other.handle, C.byref(h))
        return HPCSparseMatrix._wrap(h, self.backend)

    @property
    def T(self):                                            # lazy Adjoint in the reference; materialised here
        h = C.c_void_p()
        call("mgb_csr_transpose", self.handle, C.byref(h))
        return HPCSparseMatrix._wrap(h, self.backend)

    def to_scipy(self):
        return self.host.copy()

    def local_block(self, rank: int, world: int, Ti=np.int32) -> dict:
        """Rank `rank`'s fields of this matrix in the reference's distributed layout (see `hpc_local_block`)."""
        return hpc_local_block(self.host, rank, world, Ti)

    @staticmethod
    def from_local_blocks(blocks, backend: Optional["HPCBackend"] = None) -> "HPCSparseMatrix":
        return HPCSparseMatrix(hpc_from_local_blocks(blocks), backend)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mgb_csr_free(self.handle)
        except Exception:
            pass


def _csr_list_op(name: str, mats) -> "HPCSparseMatrix":
    arr = (C.c_void_p * len(mats))(*[m.handle for m in mats])
    h = C.c_void_p()
    call(name, len(mats), arr, C.byref(h))
    return HPCSparseMatrix._wrap(h, mats[0].backend)


def hcat(*mats: "HPCSparseMatrix") -> "HPCSparseMatrix":
    """hcat(M...) (D0 = hcat(op, Z): test/test_d0_construction.jl:92-100)."""
    return _csr_list_op("mgb_csr_hcat", mats)


class _GeoMatrix(HPCSparseMatrix):
    """A matrix of a geometry the library built itself (mgb_fem*d_native): it already lives in the mgb_geo handle, so
    nothing is copied until somebody asks -- `.host` reads it from the handle, `.handle` (any device operation) uploads it
    on first use.  fem*d_mpi() therefore costs the C++ mesh build only; the solve itself never touches these objects (the
    AMG takes its operators from the mgb_geo handle)."""

    def __init__(self, geo_ref, name: str, backend: "HPCBackend"):
        self._geo_ref, self._name, self.backend, self._host, self._h = geo_ref, name, backend, None, None
        r, c, nz = C.c_int(), C.c_int(), C.c_int()
        call("mgb_geo_matrix_info", geo_ref.handle, name.encode(), C.byref(r), C.byref(c), C.byref(nz))
        self.shape = (r.value, c.value)

    @property
    def host(self) -> sp.csr_matrix:
        if self._host is None:
            self._host = _geo_matrix(self._geo_ref.handle, self._name)
        return self._host

    @property
    def handle(self):
        if self._h is None:
            S = self.host
            h = C.c_void_p()
            rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
            call("mgb_csr_create", self.backend.handle, S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va), C.byref(h))
            self._h = h
        return self._h

    @property
    def nnz(self) -> int:
        return int(self.host.nnz)

    def __del__(self):
        try:
            if self._h is not None:
                _lib.load().mgb_csr_free(self._h)
        except Exception:
            pass


class _GeoRef:
    """Owner of an mgb_geo handle shared by a Geometry and its lazily materialised matrices."""

    def __init__(self, handle):
        self.handle = handle

    def __del__(self):
        try:
            if self.handle is not None:
                _lib.load().mgb_geo_destroy(self.handle)
        except Exception:
            pass


# --------------------------------------------------------------------------- hooks (src:62-192)


def amgb_zeros(like, m, n=None):
    """src:66-75,116: zeros with the storage kind of `like`."""
    if n is None:
        return HPCVector(int(m), getattr(like, "backend", None))
    if isinstance(like, HPCSparseMatrix):
        return HPCSparseMatrix(sp.csr_matrix((m, n)), like.backend)
    return HPCMatrix(np.zeros((m, n)), getattr(like, "backend", None))


def amgb_all_isfinite(z) -> bool:
    """src:121-133: all(isfinite) on the device, one flag back."""
    v = z._v if isinstance(z, HPCMatrix) else z
    out = C.c_int()
    call("mgb_all_isfinite", v.handle, C.byref(out))
    return bool(out.value)


def amgb_diag(like, z, m=None, n=None) -> HPCSparseMatrix:
    """src:137-147: spdiagm(m, n, 0 => z) as a device CSR."""
    backend = getattr(like, "backend", None) or backend_hip()
    if not isinstance(z, HPCVector):
        z = HPCVector(z, backend)
    m = len(z) if m is None else m
    n = len(z) if n is None else n
    h = C.c_void_p()
    call("mgb_diag", backend.handle, z.handle, int(m), int(n), C.byref(h))
    return HPCSparseMatrix._wrap(h, backend)


def amgb_blockdiag(*mats: HPCSparseMatrix) -> HPCSparseMatrix:
    """src:150."""
    return _csr_list_op("mgb_csr_blockdiag", mats)


def _raw_array(x):
    """src:175-176."""
    return x._v if isinstance(x, HPCMatrix) else x


def _to_cpu_array(x):
    """src:183-188: device -> host copy for scalar indexing."""
    return x if isinstance(x, np.ndarray) else x.to_numpy()


def map_rows(f: Callable, A, *args):
    """src:161-163.  Row-wise map over co-partitioned arrays; scalar results -> HPCVector, row results
    -> HPCMatrix.  Arbitrary host closures cannot cross the C ABI: they are evaluated
    on the host on a device->host copy (the same trade as the reference's `_to_cpu_array`, src:183-188)
    and the result is uploaded.  The barrier family used on the Newton hot path never goes through
    here: its F/F1/F2 are the fused HIP kernels behind `AMG.f0/f1/f2`."""
    if isinstance(f, BarrierFn) and len(args) == 1 and isinstance(args[0], HPCMatrix):
        return f.rows(args[0])                      # the barrier family: fused HIP kernels, nothing leaves the device
    arrays = [A, *args]
    backend = next((a.backend for a in arrays if hasattr(a, "backend")), None)
    host = [np.asarray(_to_cpu_array(a), dtype=np.float64) for a in arrays]
    n = host[0].shape[0]
    rows = []
    for i in range(n):
        rows.append(np.asarray(f(*[h[i:i + 1] if h.ndim == 1 else h[i, :] for h in host]), dtype=np.float64))
    if rows and rows[0].ndim == 0:
        return HPCVector(np.array([float(r) for r in rows]), backend)
    return HPCMatrix(np.vstack([r.reshape(1, -1) for r in rows]), backend)


def map_rows_gpu(f: Callable, A, *args):
    """src:168-170."""
    return map_rows(f, A, *args)


# --------------------------------------------------------------------------- Geometry


@dataclass
class Geometry:
    """MultiGridBarrier `Geometry` fields in the reference's order (src:318-330)."""
    discretization: dict
    x: object
    w: object
    subspaces: Dict[str, list]
    operators: Dict[str, object]
    refine: list
    coarsen: list
    _geo: object = field(default=None, repr=False)     # mgb_geo handle (MPI geometries only)
    _geo_ref: object = field(default=None, repr=False) # shared owner of that handle, when the library built the geometry
    _locator: object = field(default=None, repr=False) # mgb_locator handle, made by the first interpolate() and freed here
    _boundary: object = field(default=None, repr=False)      # Boundary (host arrays), made by the first boundary()
    _boundary_dev: object = field(default=None, repr=False)  # mgb_boundary handle, made by the first boundary_flux(); it uses the locator
    _boundary_rows: object = field(default=None, repr=False) # the distinct rows of the facet nodes, ascending (neumann_load)
    _mixed: object = field(default=None, repr=False)         # facet selection (mask bytes) -> name of its dirichlet_on() subspace
    _interior: object = field(default=None, repr=False)      # InteriorFacets (host arrays), made by the first interior()

    def __del__(self):
        try:
            if self._boundary_dev is not None:
                _lib.load().mgb_boundary_destroy(self._boundary_dev)
                self._boundary_dev = None
        except Exception:
            pass
        try:
            if self._locator is not None:
                _lib.load().mgb_locator_destroy(self._locator)
                self._locator = None
        except Exception:
            pass
        try:
            if self._geo is not None and self._geo_ref is None:
                _lib.load().mgb_geo_destroy(self._geo)
        except Exception:
            pass


def _geo_matrix(h, name) -> sp.csr_matrix:
    r, c, nz = C.c_int(), C.c_int(), C.c_int()
    call("mgb_geo_matrix_info", h, name.encode(), C.byref(r), C.byref(c), C.byref(nz))
    rp = np.empty(r.value + 1, dtype=np.int32)
    ci = np.empty(nz.value, dtype=np.int32)
    va = np.empty(nz.value)
    call("mgb_geo_matrix_get", h, name.encode(), iptr(rp), iptr(ci), dptr(va))
    return sp.csr_matrix((va, ci, rp), shape=(r.value, c.value))


def _native_from_handle(h, kind, ops) -> Geometry:
    n, dim, L, block = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(L), C.byref(block))
    x = np.empty((n.value, dim.value))
    w = np.empty(n.value)
    call("mgb_geo_get_xw", h, dptr(x), dptr(w))
    operators = {k: _geo_matrix(h, "op:" + k) for k in ops}
    subspaces = {k: [_geo_matrix(h, "sub:%s:%d" % (k, l)) for l in range(L.value)] for k in ("dirichlet", "full")}
    refine = [_geo_matrix(h, "refine:%d" % l) for l in range(L.value)]
    coarsen = [_geo_matrix(h, "coarsen:%d" % l) for l in range(L.value)]
    disc = dict(kind=kind, L=L.value, dim=dim.value, block=block.value)
    return Geometry(disc, x, w, subspaces, operators, refine, coarsen)


def fem1d(L: int = 4) -> Geometry:
    """Native 1-D geometry (MultiGridBarrier.fem1d, called at src:561)."""
    h = C.c_void_p()
    call("mgb_fem1d_native", int(L), C.byref(h))
    try:
        return _native_from_handle(h, "fem1d", ("id", "dx"))
    finally:
        call("mgb_geo_destroy", h)


def fem2d(L: int = 2, K=None) -> Geometry:
    """Native 2-D geometry (MultiGridBarrier.fem2d, called at src:628)."""
    h = C.c_void_p()
    if K is None:
        call("mgb_fem2d_native", int(L), None, 0, C.byref(h))
    else:
        Kc = f64(K)
        call("mgb_fem2d_native", int(L), dptr(Kc), int(Kc.shape[0]), C.byref(h))
    try:
        return _native_from_handle(h, "fem2d", ("id", "dx", "dy"))
    finally:
        call("mgb_geo_destroy", h)


def native_to_mpi(g_native: Geometry, Ti=np.int32, backend: Optional[HPCBackend] = None) -> Geometry:
    """src:259-338: convert a native Geometry to device types.  Keys are visited in sorted order as in
    the reference (src:276,286).  Index type is Int32 (src:260); other Ti are rejected."""
    if np.dtype(Ti) != np.dtype(np.int32):
        raise ValueError("native_to_mpi: only Ti=Int32 is supported by the HIP path")
    backend = backend or backend_hip()
    x = f64(np.asarray(g_native.x))
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    w = f64(g_native.w)
    n, dim = x.shape
    L = len(g_native.refine)
    h = C.c_void_p()
    call("mgb_geo_create", n, dim, L, int(g_native.discretization.get("block", 1)), dptr(x), dptr(w), C.byref(h))

    def put(name, S):
        S = sp.csr_matrix(S, dtype=np.float64)
        S.sort_indices()
        S.sum_duplicates()
        rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
        call("mgb_geo_set_matrix", h, name.encode(), S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va))
        return HPCSparseMatrix(S, backend)

    try:
        operators = {k: put("op:" + k, g_native.operators[k]) for k in sorted(g_native.operators)}
        subspaces = {k: [put("sub:%s:%d" % (k, l), S) for l, S in enumerate(g_native.subspaces[k])]
                     for k in sorted(g_native.subspaces)}
        refine = [put("refine:%d" % l, S) for l, S in enumerate(g_native.refine)]
        coarsen = [put("coarsen:%d" % l, S) for l, S in enumerate(g_native.coarsen)]
    except Exception:
        call("mgb_geo_destroy", h)
        raise
    return Geometry(dict(g_native.discretization), HPCMatrix(x, backend), HPCVector(w, backend), subspaces,
                    operators, refine, coarsen, _geo=h)


def _mpi_from_native_handle(h, kind, ops, backend: Optional[HPCBackend], extra=None) -> Geometry:
    """fem*d_mpi without the detour through host matrices: the geometry the library's builder just made IS the uploaded
    geometry (native_to_mpi's job, src:259-338); x and w go to the device now, the matrices when first used (_GeoMatrix)."""
    backend = backend or backend_hip()
    ref = _GeoRef(h)
    n, dim, L, block = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    call("mgb_geo_dims", h, C.byref(n), C.byref(dim), C.byref(L), C.byref(block))
    x = np.empty((n.value, dim.value))
    w = np.empty(n.value)
    call("mgb_geo_get_xw", h, dptr(x), dptr(w))
    lazy = lambda name: _GeoMatrix(ref, name, backend)
    operators = {k: lazy("op:" + k) for k in sorted(ops)}                                    # sorted keys as src:276,286
    subspaces = {k: [lazy("sub:%s:%d" % (k, l)) for l in range(L.value)] for k in ("dirichlet", "full")}
    refine = [lazy("refine:%d" % l) for l in range(L.value)]
    coarsen = [lazy("coarsen:%d" % l) for l in range(L.value)]
    disc = dict(kind=kind, L=L.value, dim=dim.value, block=block.value, **(extra or {}))
    return Geometry(disc, HPCMatrix(x, backend), HPCVector(w, backend), subspaces, operators, refine, coarsen, _geo=h,
                    _geo_ref=ref)


def _check_ti(Ti):
    if np.dtype(Ti) != np.dtype(np.int32):
        raise ValueError("only Ti=Int32 is supported by the HIP path")


def fem1d_mpi(L: int = 4, Ti=np.int32, backend=None) -> Geometry:
    """src:559-565."""
    _check_ti(Ti)
    h = C.c_void_p()
    call("mgb_fem1d_native", int(L), C.byref(h))
    return _mpi_from_native_handle(h, "fem1d", ("id", "dx"), backend)


def fem3d(L: int = 2, k: int = 3) -> Geometry:
    """Native 3-D geometry (MultiGridBarrier.fem3d, called at src:698): Q_k hexahedra, k = 3 default."""
    h = C.c_void_p()
    call("mgb_fem3d_native", int(L), int(k), C.byref(h))
    try:
        g = _native_from_handle(h, "fem3d", ("id", "dx", "dy", "dz"))
        g.discretization["k"] = int(k)
        return g
    finally:
        call("mgb_geo_destroy", h)


def fem3d_mpi(L: int = 2, k: int = 3, Ti=np.int32, backend=None) -> Geometry:
    """src:696-702."""
    _check_ti(Ti)
    h = C.c_void_p()
    call("mgb_fem3d_native", int(L), int(k), C.byref(h))
    return _mpi_from_native_handle(h, "fem3d", ("id", "dx", "dy", "dz"), backend, extra=dict(k=int(k)))


def fem2d_mpi(L: int = 2, K=None, Ti=np.int32, backend=None) -> Geometry:
    """src:626-632."""
    _check_ti(Ti)
    h = C.c_void_p()
    if K is None:
        call("mgb_fem2d_native", int(L), None, 0, C.byref(h))
    else:
        Kc = f64(K)
        call("mgb_fem2d_native", int(L), dptr(Kc), int(Kc.shape[0]), C.byref(h))
    return _mpi_from_native_handle(h, "fem2d", ("id", "dx", "dy"), backend)


# --------------------------------------------------------------------------- AMG + amgb

DEFAULT_STATE = (("u", "dirichlet"), ("s", "full"))
DEFAULT_D = {1: (("u", "id"), ("u", "dx"), ("s", "id")),
             2: (("u", "id"), ("u", "dx"), ("u", "dy"), ("s", "id")),
             3: (("u", "id"), ("u", "dx"), ("u", "dy"), ("u", "dz"), ("s", "id"))}              # src:736
class _RowFn:
    """A per-row function f(x_i) -> vector (what the reference's `f` / `g` kwargs are) that also knows its own
    vectorised form over all rows of x: the default problem data of 57 344 rows is then built in microseconds instead
    of 57 344 Python calls (0.08 s of the 0.45 s setup at fem2d L=7)."""

    def __init__(self, row, grid):
        self._row, self.grid = row, grid

    def __call__(self, x):
        return self._row(x)


def _rows(fn, x) -> np.ndarray:
    """fn evaluated at every row of x -> (n, k) array."""
    if hasattr(fn, "grid"):
        return np.ascontiguousarray(fn.grid(x), dtype=np.float64)
    return np.vstack([np.asarray(fn(xi), dtype=np.float64) for xi in x])


def _const_rows(v):
    v = np.asarray(v, dtype=np.float64)
    return _RowFn(lambda x: v.copy(), lambda x: np.tile(v, (x.shape[0], 1)))


DEFAULT_F = {1: _const_rows([0.5, 0.0, 1.0]), 2: _const_rows([0.5, 0.0, 0.0, 1.0]), 3: _const_rows([0.5, 0.0, 0.0, 0.0, 1.0])}   # src:737
DEFAULT_G = {1: _RowFn(lambda x: np.array([x[0], 2.0]), lambda x: np.column_stack([x[:, 0], np.full(x.shape[0], 2.0)])),
             2: _RowFn(lambda x: np.array([x[0] ** 2 + x[1] ** 2, 100.0]),
                       lambda x: np.column_stack([x[:, 0] ** 2 + x[:, 1] ** 2, np.full(x.shape[0], 100.0)])),
             3: _RowFn(lambda x: np.array([x[0] ** 2 + x[1] ** 2 + x[2] ** 2, 100.0]),
                       lambda x: np.column_stack([x[:, 0] ** 2 + x[:, 1] ** 2 + x[:, 2] ** 2, np.full(x.shape[0], 100.0)]))}   # src:738


def _encode_terms(cones):
    """ctypes arrays describing barrier terms for mgb_amg_create_terms / mgb_map_rows_barrier."""
    kind, nq, iq, isl, is2, pp, coef, off = [], [], [], [], [], [], [], []
    for c in cones:
        if c[0] == "linear":
            _, cidx, ccoef, coff = c
            if not 1 <= len(cidx) <= 3 or len(ccoef) != len(cidx):
                raise ValueError("linear barrier term: 1..3 columns with one coefficient each")
            kind.append(1); nq.append(len(cidx)); iq += (list(cidx) + [0, 0, 0])[:3]; isl.append(0); is2.append(-1)
            pp.append(1.0); coef += (list(map(float, ccoef)) + [0.0, 0.0, 0.0])[:3]; off.append(float(coff))
        else:
            kind.append(0); nq.append(len(c[0]) - 1); iq += (list(c[0][:-1]) + [0, 0, 0])[:3]; isl.append(int(c[0][-1]))
            is2.append(int(c[2]) if len(c) > 2 else -1); pp.append(float(c[1])); coef += [0.0, 0.0, 0.0]; off.append(0.0)
    arr_i = lambda v: (C.c_int * len(v))(*v)
    arr_d = lambda v: (C.c_double * len(v))(*v)
    return (len(cones), arr_i(kind), arr_i(nq), arr_i(iq), arr_i(isl), arr_i(is2), arr_d(pp), arr_d(coef), arr_d(off))


class BarrierFn:
    """One of the three row functions MultiGridBarrier derives from a convex set -- F (which = 0), its gradient F1 (1) or its
    Hessian F2 (2, flattened to K*K columns) -- as an object `map_rows` recognises: `map_rows(fn, x, Dz)` with a device
    matrix Dz then runs the fused HIP kernels (mgb_map_rows_barrier) instead of the host fallback.  This is the closure
    pattern-match of SURVEY.md section 7.2-5: the barrier family has a device form, everything else is evaluated on the host.
    Calling the object on one row (`fn(x_i, dz_i)`, the reference's signature, test/test_apply_d.jl:64,81) works too."""

    def __init__(self, cones, K: int, which: int):
        self.cones, self.K, self.which = list(cones), int(K), int(which)

    def rows(self, Dz: "HPCMatrix"):
        n, K = Dz.shape
        if K != self.K:
            raise ValueError("BarrierFn: Dz has %d columns, the barrier was built for %d" % (K, self.K))
        width = (1, K, K * K)[self.which]
        out = HPCVector(n * width, Dz.backend)
        call("mgb_map_rows_barrier", self.which, K, *_encode_terms(self.cones), n, Dz._v.handle, out.handle)
        if self.which == 0:
            return out
        M_ = HPCMatrix.__new__(HPCMatrix)
        M_.shape, M_.backend, M_._v = (n, width), Dz.backend, out
        return M_

    def __call__(self, x_row, dz_row):
        r = self.rows(HPCMatrix(np.asarray(dz_row, dtype=np.float64).reshape(1, -1))).to_numpy()
        return float(r[0]) if self.which == 0 else r[0]


def barrier_functions(cones, K: int):
    """(F, F1, F2) of the intersection of the given terms (see `AMG` for the term syntax), acting on rows of an n x K Dz."""
    return tuple(BarrierFn(cones, K, w) for w in (0, 1, 2))


class AMG:
    """AMG hierarchy + barrier problem resident in HBM (upstream `amg` + `barrier`)."""

    def __init__(self, geometry: Geometry, state_variables=DEFAULT_STATE, D=None, p: float = 1.0, idx=None,
                 cones=None, select=None):
        """`cones` = the terms of the barrier (an intersection of up to three convex sets, upstream `intersect`):
        (idx, p) | (idx, p, idx_s2) -- the power cone s >= |q|^p on the D rows idx = (q_1..q_d, s) (convex_Euclidian_power);
        ("linear", idx, coef, off)  -- the half space sum_i coef[i] * Dz[:, idx[i]] + off > 0 (convex_linear with one constant
        row: bounds, constant obstacles).  Default: one power cone on the last dim+1 rows of D with exponent p."""
        if geometry._geo is None:
            raise TypeError("AMG needs an MPI geometry (use native_to_mpi / fem*d_mpi)")
        dim = geometry.discretization["dim"]
        D = DEFAULT_D[dim] if D is None else D
        K = len(D)
        if cones is None:
            if idx is None:
                idx = list(range(K - dim - 1, K))       # convex_Euclidian_power(idx=2:dim+2)
            cones = [(list(idx), float(p) if np.isscalar(p) else p)]      # p may be a function p(x) or per-node values
        # x-dependent exponents (upstream convex_Euclidian_power with a function p(x)): a callable or an array of per-node values in
        # a power-cone term is evaluated at the nodes and handed over with mgb_amg_set_exponents after the AMG exists
        self.geometry = geometry
        node_p, cones = {}, list(cones)
        for ti, c in enumerate(cones):
            if c[0] != "linear" and not np.isscalar(c[1]):
                pv = c[1]
                pn = (np.array([float(pv(xi)) for xi in geometry.x.to_numpy()]) if callable(pv) else f64(pv).reshape(-1))
                if pn.size != geometry.x.shape[0] or not np.all(pn >= 1.0):
                    raise ValueError("p(x) must give one value >= 1 per node")
                node_p[ti] = pn
                cones[ti] = (c[0], float(pn[0])) + tuple(c[2:])
        p = float(p) if np.isscalar(p) else (float(node_p[0][0]) if 0 in node_p else 1.0)
        self.p_nodes = node_p.get(0)
        self.state_variables, self.D, self.p, self.cones = tuple(state_variables), tuple(D), float(p), list(cones)
        power = [c for c in cones if c[0] != "linear"]
        self.idx = list(power[0][0]) if power else []
        backend = geometry.x.backend
        h = C.c_void_p()
        call("mgb_amg_create_terms", backend.handle, geometry._geo, len(state_variables), _lib.str_array(state_variables), K,
             _lib.str_array(D), *_encode_terms(cones), C.byref(h))
        self.handle = h
        n, S, K_, L, nY = (C.c_int() for _ in range(5))
        call("mgb_amg_dims", h, C.byref(n), C.byref(S), C.byref(K_), C.byref(L), C.byref(nY))
        self.S, self.K, self.L, self.nY = S.value, K_.value, L.value, nY.value
        ng, r0, nl = C.c_int(), C.c_int(), C.c_int()
        call("mgb_amg_local_rows", h, C.byref(ng), C.byref(r0), C.byref(nl))
        # n = global rows (what set_c / set_z / get_z exchange on every rank); a sharded AMG (backend.set_comm)
        # evaluates apply_D on its own rows [row0, row0 + n_local) only
        self.n, self.row0, self.n_local = ng.value, r0.value, nl.value
        for ti, pn in node_p.items():
            call("mgb_amg_set_exponents", h, int(ti), dptr(pn))
        if select is not None:      # upstream convex_piecewise: term c is active at x iff select(x)[c]
            mask = np.ascontiguousarray([[1 if b else 0 for b in select(xi)] for xi in geometry.x.to_numpy()], dtype=np.uint8)
            if mask.shape != (self.n, len(cones)):
                raise ValueError("select(x) must give one flag per barrier term")
            call("mgb_amg_set_term_mask", h, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))

    def prepare(self, l=-1):
        """Build the level(s) and the factorisation structures now (default: every level the schedule visits), so
        that the next solve() is pure compute."""
        call("mgb_amg_prepare", self.handle, int(l))

    def level_size(self, l):
        N, nz = C.c_int(), C.c_int()
        call("mgb_amg_level_size", self.handle, l, C.byref(N), C.byref(nz))
        return N.value, nz.value

    def chol_info(self, l=None):
        """Device factorisation of level l (default finest): ranks it is split over, doubles exchanged and launches per
        Newton system, whether the Hessian values stay on the rank that computed them (subtrees = row blocks), and the
        device memory of the pre-mapped contribution slabs (MGB_CHOL_PREMAP)."""
        sw, ex, la = C.c_int(), C.c_double(), C.c_int()
        call("mgb_amg_chol_info", self.handle, self.L - 1 if l is None else int(l), C.byref(sw), C.byref(ex), C.byref(la))
        vl = C.c_int()
        call("mgb_amg_chol_values_local", self.handle, self.L - 1 if l is None else int(l), C.byref(vl))
        sb = C.c_double()
        call("mgb_amg_chol_premap", self.handle, self.L - 1 if l is None else int(l), 0, None, None, C.byref(sb))
        return dict(split_world=sw.value, exchange_doubles=ex.value, launches=la.value, values_local=bool(vl.value),
                    slab_bytes=sb.value)

    CHOL_KINDS = ("Leaf", "Single", "SingleNarrow", "SingleDense", "SingleDenseNarrow", "Start", "Step", "Step2", "Panel2",
                  "Update2", "BwdRect", "Bwd256", "Bwd1024", "BwdFused")      # kind codes of mgb_amg_chol_schedule

    def chol_schedule(self, l=None):
        """Launch chain of the device factorisation of level l (default finest) in launch order: kind names and workgroup
        counts, whether the launch reads pre-mapped contribution slabs (premap_consumer) and how many of its fronts store
        their Schur complement into one (premap_producers); per unknown its tree node (postorder) and own column; and per
        tree node its own size, front size, parent and height (leaves 0).  Read-only."""
        l = self.L - 1 if l is None else int(l)
        N = self.level_size(l)[0]
        nl = C.c_int()
        call("mgb_amg_chol_schedule", self.handle, l, 0, C.byref(nl), None, None, None, None)
        kind, wg = np.empty(nl.value, dtype=np.int32), np.empty(nl.value, dtype=np.int32)
        node, col = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
        call("mgb_amg_chol_schedule", self.handle, l, nl.value, C.byref(nl), iptr(kind), iptr(wg), iptr(node), iptr(col))
        cons, prod = np.zeros(nl.value, dtype=np.int32), np.zeros(nl.value, dtype=np.int32)
        call("mgb_amg_chol_premap", self.handle, l, nl.value, iptr(cons), iptr(prod), None)
        nn = C.c_int()
        call("mgb_amg_chol_tree", self.handle, l, 0, C.byref(nn), None, None, None)
        ns, nf, par = (np.empty(nn.value, dtype=np.int32) for _ in range(3))
        call("mgb_amg_chol_tree", self.handle, l, nn.value, C.byref(nn), iptr(ns), iptr(nf), iptr(par))
        height = np.zeros(nn.value, dtype=np.int32)
        for t in range(nn.value):                     # postorder: children first
            if par[t] >= 0:
                height[par[t]] = max(height[par[t]], height[t] + 1)
        return dict(kinds=[self.CHOL_KINDS[k] for k in kind], workgroups=wg, unknown_node=node, unknown_col=col, ns=ns, nf=nf,
                    parent=par, height=height, premap_consumer=cons.astype(bool), premap_producers=prod)

    def hessian_pattern(self, l):
        N, nz = self.level_size(l)
        rp = np.empty(N + 1, dtype=np.int32)
        ci = np.empty(nz, dtype=np.int32)
        call("mgb_amg_hessian_pattern", self.handle, l, iptr(rp), iptr(ci))
        return rp, ci

    def set_c(self, c):
        c = f64(c)
        assert c.shape == (self.n, self.K)
        call("mgb_amg_set_c", self.handle, dptr(c))

    def set_z(self, z):
        z = f64(np.asarray(z).reshape(-1))
        assert z.size == self.n * self.S
        call("mgb_amg_set_z", self.handle, dptr(z))

    def get_z(self):
        z = np.empty(self.n * self.S)
        call("mgb_amg_get_z", self.handle, dptr(z))
        return z

    def get_c(self):
        """The cost as the device holds it, (n_local, K)."""
        c = np.empty((self.n_local, self.K))
        call("mgb_amg_get_c", self.handle, dptr(c))
        return c

    def add_cost_rows(self, load: "NeumannLoad", col: int, k: int = 0, alpha: float = 1.0):
        """c[load.rows, col] += alpha * load.values[k], on the device behind set_c (include/mgb_hip.h: mgb_amg_add_cost_rows)."""
        if load.geometry is not self.geometry:
            raise ValueError("add_cost_rows: the load belongs to another geometry")
        call("mgb_amg_add_cost_rows", self.handle, self.geometry._boundary_dev, load.values._v.handle, int(k), float(alpha), int(col))

    def parabolic_begin(self, bidx):
        """Time loop of parabolic_solve on the device (include/mgb_hip.h): `bidx` = the nodes that carry Dirichlet data."""
        bidx = i32(np.asarray(bidx).reshape(-1))
        call("mgb_amg_parabolic_begin", self.handle, bidx.size, iptr(bidx))

    def parabolic_step(self, h, p, f_nodes: "HPCVector", gb: Optional["HPCVector"] = None, wait=True):
        """Cost from the old u, boundary overwrite, violations and lifts of one time step, enqueued behind each other.
        wait=True returns (lift_1, lift_2); wait=False returns None without waiting for the device (see parabolic_lifts)."""
        out = np.empty(2) if wait else None
        call("mgb_amg_parabolic_step", self.handle, float(h), float(p), f_nodes.handle, None if gb is None else gb.handle, dptr(out))
        return out

    def parabolic_lifts(self):
        out = np.empty(2)
        call("mgb_amg_parabolic_lifts", self.handle, dptr(out))
        return out

    def snapshot(self) -> "HPCMatrix":
        """The current z as an (n, S) HPCMatrix with device storage of its own, written by one kernel."""
        out = HPCMatrix.__new__(HPCMatrix)
        out.shape, out.backend = (self.n, self.S), self.geometry.x.backend
        out._v = HPCVector(self.n * self.S, out.backend)
        call("mgb_amg_snapshot", self.handle, out._v.handle)
        return out

    def apply_D(self, l, s):
        s = f64(s)
        out = np.empty((self.n_local, self.K))
        call("mgb_amg_apply_D", self.handle, l, dptr(s), dptr(out))
        return out

    def apply_D_global(self, l, s):
        """apply_D on all n rows on every rank (a sharded AMG gathers the row blocks by summation)."""
        loc = self.apply_D(l, s)
        backend = self.geometry.x.backend
        if backend.world == 1:
            return loc
        full = np.zeros((self.n, self.K))
        full[self.row0:self.row0 + self.n_local] = loc
        v = HPCVector(full.reshape(-1), backend)
        call("mgb_vec_allreduce_sum", v.handle)
        return v.to_numpy().reshape(self.n, self.K)

    def f0(self, l, s, t, parts=False):
        s = f64(s)
        y = C.c_double()
        pr = np.empty(2)
        call("mgb_amg_f0", self.handle, l, dptr(s), float(t), C.byref(y), dptr(pr))
        return (y.value, pr) if parts else y.value

    def f0_trial(self, l, s_ref, s, t):
        """Line-search trial: f0(s), or +inf if a row lost more than 90 % of its cone distance w.r.t. s_ref."""
        s_ref, s = f64(s_ref), f64(s)
        y = C.c_double()
        call("mgb_amg_f0_trial", self.handle, l, dptr(s_ref), dptr(s), float(t), C.byref(y))
        return y.value

    def f1(self, l, s, t):
        s = f64(s)
        g = np.empty(self.level_size(l)[0])
        call("mgb_amg_f1", self.handle, l, dptr(s), float(t), dptr(g))
        return g

    def f2(self, l, s, t):
        """R'HR as a scipy CSR (full symmetric), assembled on the GPU."""
        s = f64(s)
        N, nz = self.level_size(l)
        vals = np.empty(nz)
        call("mgb_amg_f2", self.handle, l, dptr(s), float(t), dptr(vals))
        rp, ci = self.hessian_pattern(l)
        Lo = sp.csr_matrix((vals, ci, rp), shape=(N, N))
        return Lo + sp.tril(Lo, -1).T, vals

    # Float32 evaluation (csrc/kernels_f32.hip): the same SpMV / barrier kernels instantiated for float
    def f0_f32(self, l, s, t):
        s = np.ascontiguousarray(s, dtype=np.float32)
        y = C.c_double()
        call("mgb_amg_f0_f32", self.handle, l, s.ctypes.data_as(_lib.c_flt_p), float(t), C.byref(y))
        return y.value

    def f1_f32(self, l, s, t):
        s = np.ascontiguousarray(s, dtype=np.float32)
        g = np.empty(self.level_size(l)[0], dtype=np.float32)
        call("mgb_amg_f1_f32", self.handle, l, s.ctypes.data_as(_lib.c_flt_p), float(t), g.ctypes.data_as(_lib.c_flt_p))
        return g

    def f2_f32(self, l, s, t):
        """Lower-triangle values of R'HR in the order of hessian_pattern(l), float32."""
        s = np.ascontiguousarray(s, dtype=np.float32)
        vals = np.empty(self.level_size(l)[1], dtype=np.float32)
        call("mgb_amg_f2_f32", self.handle, l, s.ctypes.data_as(_lib.c_flt_p), float(t), vals.ctypes.data_as(_lib.c_flt_p))
        return vals

    def f1_template_f64(self, l, s, t):
        s = f64(s)
        g = np.empty(self.level_size(l)[0])
        call("mgb_amg_f1_template_f64", self.handle, l, dptr(s), float(t), dptr(g))
        return g

    def f2_template_f64(self, l, s, t):
        s = f64(s)
        vals = np.empty(self.level_size(l)[1])
        call("mgb_amg_f2_template_f64", self.handle, l, dptr(s), float(t), dptr(vals))
        return vals

    TRIAL_MODES = {"set": 0, "separate": 1, "unfused": 2}

    def trial_set(self, l, s, nstep, alphas, phi_ref=None, mode="set"):
        """The line search's objective at the points x_a = s + alphas[a] * nstep (1 to 3 of them; nstep None: x_a = s) on the
        buffers a solve uses (tests).  phi_ref (n x nterms, None: no rule): the fraction-to-the-boundary rule against these cone
        distances.  mode "set": one fused launch for all points; "separate": one fused launch per point; "unfused": x_a,
        apply_D and the objective kernel per point.  Returns a dict: sums_host / sums (na x 2: sum w F, sum w <c, Dz>, as left in
        pinned host memory / copied from the device), s_out (na x N), dz (na x n x K), phi (na x n x nterms)."""
        s, alphas = f64(s), f64(np.asarray(alphas).reshape(-1))
        nstep = None if nstep is None else f64(nstep)
        N, na, nt = self.level_size(l)[0], alphas.size, len(self.cones)
        if s.shape != (N,) or (nstep is not None and nstep.shape != (N,)):
            raise ValueError("trial_set: s and nstep hold one value per unknown of the level")
        if phi_ref is not None:
            phi_ref = f64(phi_ref)
            if phi_ref.shape != (self.n_local, nt):
                raise ValueError("trial_set: phi_ref holds one value per node and barrier term")
        out = dict(sums_host=np.empty((na, 2)), sums=np.empty((na, 2)), s_out=np.empty((na, N)),
                   dz=np.empty((na, self.n_local, self.K)), phi=np.empty((na, self.n_local, nt)))
        call("mgb_amg_trial_set", self.handle, int(l), dptr(s), dptr(nstep), na, dptr(alphas), dptr(phi_ref),
             self.TRIAL_MODES[mode], dptr(out["sums_host"]), dptr(out["sums"]), dptr(out["s_out"]), dptr(out["dz"]),
             dptr(out["phi"]))
        return out

    def f2_hpc(self, l, s, t) -> HPCSparseMatrix:
        """The Newton matrix R'HR of level l as an HPCSparseMatrix (what `f2` returns in the reference and what
        test/test_newton_matrix_compare.jl:33-51 captures); `.local_block(rank, world)` gives the per-rank fields."""
        H, _ = self.f2(l, s, t)
        return HPCSparseMatrix(H, self.geometry.x.backend)

    def solve_linear(self, l, lower_vals, g, solver="gpu"):
        """MultiGridBarrier.solve(A, b) = A \\ b on the level's fixed pattern: device (default) or host
        multifrontal Cholesky."""
        lower_vals, g = f64(lower_vals), f64(g)
        x = np.empty_like(g)
        call("mgb_amg_solve_linear_gpu" if solver == "gpu" else "mgb_amg_solve_linear", self.handle, l,
             dptr(lower_vals), dptr(g), dptr(x))
        return x

    # ---- the owner-local pieces of a sharded Newton step, one call each (include/mgb_hip.h: mgb_amg_f1_owner ...).  Collective:
    # every rank calls them in the same order; sharded contexts whose factorisation keeps its values local only.
    def f1_owner(self, l, s, t):
        """(g, gg, kind): the gradient as the device holds it inside a sharded solve (complete where kind >= 1), |g|^2 as the
        device summed it over the owners, and per unknown 0 = another rank's, 1 = own, 2 = top (separator)."""
        s = f64(s)
        N = self.level_size(l)[0]
        g, gg, kind = np.empty(N), C.c_double(), np.empty(N, dtype=np.int32)
        call("mgb_amg_f1_owner", self.handle, l, dptr(s), float(t), dptr(g), C.byref(gg), iptr(kind))
        return g, gg.value, kind

    def f2_local(self, l, s, t):
        """This rank's contributions to the lower-triangle Hessian values (order of hessian_pattern(l)), before any reduction."""
        s = f64(s)
        vals = np.empty(self.level_size(l)[1])
        call("mgb_amg_f2_local", self.handle, l, dptr(s), float(t), dptr(vals))
        return vals

    def solve_linear_local(self, l, local_vals, g):
        """(x, inc, flag, vals_after) of the owner-local solve on this rank's contributions `local_vals` and a g valid where
        kind >= 1: x is zero where kind = 0, inc = <g, x> over the owners, flag = 1 if a pivot was not positive on some rank
        (returned, never raised), vals_after = the values buffer behind the solve (top entries <- their sums)."""
        local_vals, g = f64(local_vals), f64(g)
        x, inc, flag, after = np.empty_like(g), C.c_double(), C.c_int(), np.empty_like(local_vals)
        call("mgb_amg_solve_linear_local", self.handle, l, dptr(local_vals), dptr(g), dptr(x), C.byref(inc), C.byref(flag),
             dptr(after))
        return x, inc.value, flag.value, after

    SOLVERS = {"gpu": 0, "host": 1, "pcg": 2}

    def set_solver(self, solver="gpu"):
        """Newton linear solver: "gpu" = device multifrontal Cholesky (default), "host" = host Cholesky, "pcg" = conjugate
        gradients preconditioned by a V-cycle over the AMG levels with H applied matrix-free."""
        if solver not in self.SOLVERS:
            raise ValueError("solver must be 'gpu', 'host' or 'pcg'")
        call("mgb_amg_set_solver", self.handle, self.SOLVERS[solver])

    def set_pcg(self, rtol=0.0, maxit=0, degree=0, power_its=0, lo_frac=0.0, hi_frac=0.0, chunk=0, fallback=None,
                assembled_top=None, giveup=-1):
        """Parameters of solver="pcg" (unset ones keep their value): see mgb_amg_set_pcg."""
        flag = lambda v: -1 if v is None else int(bool(v))
        call("mgb_amg_set_pcg", self.handle, float(rtol), int(maxit), int(degree), int(power_its), float(lo_frac),
             float(hi_frac), int(chunk), flag(fallback), flag(assembled_top), int(giveup))

    # ---- multigrid pieces: mgb_hessian_apply / mgb_smooth / mgb_prolong / mgb_restrict
    def hessian_apply(self, l, s, v, matrix_free=True):
        """H(s) v at level l: matrix-free B' (Y o (B v)) on the device, or through the assembled matrix."""
        s, v = f64(s), f64(v)
        out = np.empty_like(v)
        call("mgb_hessian_apply", self.handle, l, dptr(s), dptr(v), dptr(out), int(bool(matrix_free)))
        return out

    def smooth(self, l, s, b, x0=None, degree=2, sweeps=1, lmax=0.0, matrix_free=True):
        """Chebyshev-Jacobi smoothing of H(s) x = b from x0 (zero by default); returns (x, lambda_max used)."""
        s, b = f64(s), f64(b)
        x = np.zeros_like(b) if x0 is None else f64(x0).copy()
        used = C.c_double()
        call("mgb_smooth", self.handle, l, dptr(s), dptr(b), dptr(x), int(degree), int(sweeps), float(lmax),
             int(bool(matrix_free)), C.byref(used))
        return x, used.value

    def prolong(self, l, xc):
        xc = f64(xc)
        xf = np.empty(self.level_size(l + 1)[0])
        call("mgb_prolong", self.handle, l, dptr(xc), dptr(xf))
        return xf

    def restrict(self, l, rf):
        rf = f64(rf)
        rc = np.empty(self.level_size(l)[0])
        call("mgb_restrict", self.handle, l, dptr(rf), dptr(rc))
        return rc

    def prolongation(self, l) -> sp.csr_matrix:
        """P_l (N_{l+1} x N_l) with R_l = R_{l+1} P_l."""
        r, c, nz = C.c_int(), C.c_int(), C.c_int()
        call("mgb_amg_prolongation", self.handle, l, C.byref(r), C.byref(c), C.byref(nz), None, None, None)
        rp, ci, va = np.empty(r.value + 1, dtype=np.int32), np.empty(nz.value, dtype=np.int32), np.empty(nz.value)
        call("mgb_amg_prolongation", self.handle, l, None, None, None, iptr(rp), iptr(ci), dptr(va))
        return sp.csr_matrix((va, ci, rp), shape=(r.value, c.value))

    def pcg_solve_linear(self, l, s, g):
        """x = H(s)^{-1} g by V-cycle-preconditioned CG; returns (x, iterations, relative residual in the M norm, converged)."""
        s, g = f64(s), f64(g)
        x = np.empty_like(g)
        it, ok, rr = C.c_int(), C.c_int(), C.c_double()
        call("mgb_amg_pcg_solve_linear", self.handle, l, dptr(s), dptr(g), dptr(x), C.byref(it), C.byref(rr), C.byref(ok))
        return x, it.value, rr.value, bool(ok.value)

    def pin_lmax(self, l, lmax):
        """Use `lmax` as lambda_max(Dinv H) of level l in every later V-cycle setup instead of the device's estimate; 0 unpins."""
        call("mgb_amg_mg_pin_lmax", self.handle, int(l), float(lmax))

    def vcycle(self, top, s, b):
        """x = V(b), one V-cycle of the preconditioner of solver="pcg" at H(s) of level `top`; returns (x, lambda_max used per
        level: zero on the coarsest level of the cycle and outside it)."""
        s, b = f64(s), f64(b)
        x, used = np.empty_like(b), np.zeros(self.L)
        call("mgb_amg_vcycle", self.handle, int(top), dptr(s), dptr(b), dptr(x), dptr(used))
        return x, used

    MG_KERNEL_NAMES = ("hessian_apply", "chebyshev_step", "hessian_apply_csr", "prolong", "restrict", "hessian_apply_unfused_csr")

    def time_mg_kernels(self, l, reps=50, nrot=1):
        """HIP-event timing of the multigrid kernels at level l (rotating operand copies as time_kernels)."""
        ms, by, alg = np.empty(6), np.empty(6), np.empty(6)
        call("mgb_amg_time_mg_kernels", self.handle, int(l), int(reps), int(nrot), dptr(ms), dptr(by), dptr(alg))
        return {k: dict(ms=float(a), bytes=float(b), algorithmic_bytes=float(c)) for k, a, b, c in zip(self.MG_KERNEL_NAMES, ms, by, alg)}

    def mg_coarsest(self, top=None):
        c0 = C.c_int()
        call("mgb_amg_mg_info", self.handle, self.L - 1 if top is None else int(top), C.byref(c0))
        return c0.value

    ELOP_INFO = ("valid", "tpe", "rows_per_el", "cmax", "nnz_max", "ncls", "nel", "K", "nY", "pipelined", "elasm_valid", "grid",
                 "passes_per_wg")

    def elop_info(self, l):
        """Read-only description of level l's element operator (mgb_amg_elop_info): the kernel instantiation `tpe`, the element
        shape, which load path the apply kernel takes, whether the element-slab assembly is valid, and the launch shape."""
        out = (C.c_int * len(self.ELOP_INFO))()
        call("mgb_amg_elop_info", self.handle, int(l), out)
        d = dict(zip(self.ELOP_INFO, (int(v) for v in out)))
        for k in ("valid", "pipelined", "elasm_valid"):
            d[k] = bool(d[k])
        return d

    def solve(self, tol=None, t=0.1, kappa=10.0, maxit=10000, max_newton=0, verbose=0, schedule="fine",
              solver="gpu", stop_rule="fixed", centering="exact"):
        if schedule not in ("fine", "all"):
            raise ValueError("schedule must be 'fine' or 'all'")
        if stop_rule not in ("fixed", "upstream"):
            raise ValueError("stop_rule must be 'fixed' or 'upstream'")
        if centering not in ("decrement", "exact"):
            raise ValueError("centering must be 'decrement' or 'exact'")
        call("mgb_amg_set_stop_rule", self.handle, 1 if stop_rule == "upstream" else 0)
        call("mgb_amg_set_centering", self.handle, 1 if centering == "exact" else 0)
        call("mgb_amg_set_schedule", self.handle, 1 if schedule == "all" else 0)
        self.set_solver(solver)
        call("mgb_amg_solve", self.handle, float(tol or 0.0), float(t), float(kappa), int(maxit), int(max_newton),
             int(verbose))
        nt, te, tf = C.c_int(), C.c_double(), C.c_double()
        counts = (C.c_longlong * 4)()
        call("mgb_amg_sol_info", self.handle, C.byref(nt), C.byref(te), C.byref(tf), counts)
        its = np.empty(self.L * nt.value, dtype=np.int64)
        ts = np.empty(nt.value)
        cd = np.empty(nt.value)
        call("mgb_amg_sol_get", self.handle, its.ctypes.data_as(_lib.c_ll_p), dptr(ts), dptr(cd))
        nk = len(self.KERNEL_NAMES)
        kms, kby = np.empty(nk), np.empty(nk)
        kl = np.empty(nk, dtype=np.int64)
        call("mgb_amg_sol_kernels", self.handle, dptr(kms), dptr(kby), kl.ctypes.data_as(_lib.c_ll_p))
        kernels = {k: dict(ms=float(m), bytes=float(b), launches=int(c))
                   for k, m, b, c in zip(self.KERNEL_NAMES, kms, kby, kl)}
        pc = (C.c_longlong * 4)()
        tp = C.c_double()
        call("mgb_amg_sol_pcg", self.handle, pc, C.byref(tp))
        return dict(t_elapsed=te.value, ts=ts, its=its.reshape(nt.value, self.L).T.copy(), c_dot_Dz=cd,
                    time_factor=tf.value, n_f0=counts[0], n_f1=counts[1], n_f2=counts[2], n_factor=counts[3],
                    kernels=kernels, pcg=dict(solves=pc[0], iterations=pc[1], fallbacks=pc[2], gave_up_at=pc[3], seconds=tp.value))

    def set_exponents(self, term, p_nodes):
        """Per-node exponents p(x) >= 1 of power-cone term `term` for the later evaluations and solves (mgb_amg_set_exponents)."""
        pn = f64(p_nodes).reshape(-1)
        if pn.size != self.n:
            raise ValueError("p_nodes must give one value per node")
        call("mgb_amg_set_exponents", self.handle, int(term), dptr(pn))

    def set_term_mask(self, mask):
        """mask[q, c] != 0 iff barrier term c is active at node q (mgb_amg_set_term_mask)."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (self.n, len(self.cones)):
            raise ValueError("mask must be n x terms")
        call("mgb_amg_set_term_mask", self.handle, m.ctypes.data_as(C.POINTER(C.c_ubyte)))

    def set_time_kernels(self, on=True):
        """Live kernel timing of the later solves (every 8th Newton step as plain launches); off: every eligible step is a graph."""
        call("mgb_amg_set_time_kernels", self.handle, int(bool(on)))

    TRACE_CENTERING = ("level", "t", "finest", "final", "budget", "k", "converged", "first_step", "steps")
    TRACE_STEP = ("centering", "y", "g", "ymin", "gmin", "inc", "step", "y_next", "g_next", "pivot", "mode", "consumed", "evals",
                  "reason")
    TRACE_MODES = ("graph_replay", "graph_capture", "plain_sampled", "plain_chain", "pcg", "pcg_fallback", "host", "sharded", "plain")
    TRACE_REASONS = ("none", "inc_nonpositive", "decrement", "stagnation", "budget", "pivot", "nonfinite")

    def set_trace(self, max_steps=0, keep_vectors=False):
        """Record the Newton loop of the later solves (mgb_amg_set_trace): 0 turns it off."""
        call("mgb_amg_set_trace", self.handle, int(max_steps), int(bool(keep_vectors)))
        self._trace_vectors = bool(keep_vectors) and max_steps > 0

    def trace(self):
        """The last solve's records: dict(centerings = (nc, 9) array in TRACE_CENTERING order, steps = (ns, 14) array in TRACE_STEP
        order and, with keep_vectors, Dz0 = one (n, K) array per centering and s, nstep, s_next, Dz_next = one array per step).
        After a solve that failed the trace is partial: what was recorded up to the failure."""
        nc, ns, nv = C.c_int(), C.c_int(), C.c_longlong()
        call("mgb_amg_trace_info", self.handle, C.byref(nc), C.byref(ns), C.byref(nv))
        cen = np.empty((nc.value, len(self.TRACE_CENTERING)))
        stp = np.empty((ns.value, len(self.TRACE_STEP)))
        vec = np.empty(nv.value)
        call("mgb_amg_trace_get", self.handle, dptr(cen), dptr(stp), dptr(vec))
        out = dict(centerings=cen, steps=stp)
        if nv.value:
            nK = self.n_local * self.K
            out.update(Dz0=[], s=[], nstep=[], s_next=[], Dz_next=[])
            at = 0
            for c in cen:
                N = self.level_size(int(c[0]))[0]
                out["Dz0"].append(vec[at:at + nK].reshape(self.n_local, self.K))
                at += nK
                for _ in range(int(c[8])):
                    if at + 3 * N + nK > nv.value:
                        break
                    for name in ("s", "nstep", "s_next"):
                        out[name].append(vec[at:at + N])
                        at += N
                    out["Dz_next"].append(vec[at:at + nK].reshape(self.n_local, self.K))
                    at += nK
            if at != nv.value:      # a solve that failed inside a step: keep the complete steps only
                m = min(len(out[k]) for k in ("s", "nstep", "s_next", "Dz_next"))
                for k in ("s", "nstep", "s_next", "Dz_next"):
                    del out[k][m:]
        return out

    KERNEL_NAMES = ("apply_D", "barrier_f2", "hessian_assemble", "barrier_f1", "restrict", "barrier_f0",
                    "chol_front_start", "chol_front_step", "chol_backward_rect", "chol_backward", "chol_front_single")

    def time_kernels(self, l, reps=50, nrot=1):
        """Back-to-back launches of each kernel class; nrot > 1 rotates over that many distinct copies of every operand
        (working set nrot x bytes: beyond 256 MiB the rate is an HBM rate, not an Infinity-Cache rate)."""
        ms = np.empty(8)
        by = np.empty(8)
        call("mgb_amg_time_kernels", self.handle, l, reps, int(nrot), dptr(ms), dptr(by))
        names = ("apply_D", "barrier_f2", "hessian_assemble", "barrier_f1", "restrict", "barrier_f0", "trial_f0")
        out = {k: dict(ms=float(m), bytes=float(b)) for k, m, b in zip(names, ms, by)}
        out["apply_D"]["element_local"] = bool(by[7])
        out["apply_D_csr"] = dict(ms=float(ms[7]), bytes=float(by[0]))
        return out

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.load().mgb_amg_destroy(self.handle)
        except Exception:
            pass


def amg(geometry: Geometry, state_variables=DEFAULT_STATE, D=None, p=1.0, cones=None) -> AMG:
    return AMG(geometry, state_variables, D, p, cones=cones)


@dataclass
class AMGBSOL:
    """src:467-473 field order."""
    z: object
    SOL_feasibility: Optional[dict]
    SOL_main: dict
    log: list
    geometry: Geometry


PHASE1_SLACK_FLOOR = 1.0
PHASE1_PENALTY = 10.0


def _phase1_slack(geometry, M: "AMG", p, z0, c, tol, schedule, solver):
    """General feasibility phase (oracle amgb_phase1_slack; upstream amgb_phase1, SOL_feasibility src:428-455): the original
    problem relaxed by a slack field sigma (:full subspace, one more row `sigma id` of D) -- (q, s + sigma) in the power cone,
    coef . y + off + sigma > 0 for the half space, sigma > -1 -- with the penalty PHASE1_PENALTY max(1, |c|_max) on sigma,
    started strictly inside at sigma0 = 1 + the largest violation and path-followed on the device until sigma < 0 at every
    node (mgb_amg_set_early_stop).  Returns the strictly feasible (n, S) start of the main phase and the SOL fields."""
    n, S = z0.shape
    K = len(M.D)
    cone, extras = M.cones[0], list(M.cones[1:])
    if len(extras) > 1 or cone[0] == "linear":
        raise NotImplementedError("amgb: the feasibility phase covers the power cone intersected with one half space")
    state1 = tuple(M.state_variables) + (("sigma", "full"),)
    D1 = tuple(M.D) + (("sigma", "id"),)
    terms = [(list(cone[0]), cone[1], K)]
    terms += [("linear", list(e[1]) + [K], list(map(float, e[2])) + [1.0], float(e[3])) for e in extras]
    terms.append(("linear", [K], [1.0], PHASE1_SLACK_FLOOR))
    Dz = M.apply_D_global(M.L - 1, np.zeros(M.level_size(M.L - 1)[0]))
    idx = list(cone[0])
    viol = [np.sum(Dz[:, idx[:-1]] ** 2, axis=1) ** (cone[1] / 2.0) - Dz[:, idx[-1]]]
    viol += [-(Dz[:, list(e[1])] @ np.asarray(e[2], dtype=np.float64) + float(e[3])) for e in extras]
    sigma0 = 1.0 + max(0.0, float(np.max(np.concatenate(viol))))
    M1 = AMG(geometry, state1, D1, p, cones=terms)
    c1 = np.column_stack([c, np.full(n, PHASE1_PENALTY * max(1.0, float(np.max(np.abs(c)))))])
    M1.set_c(c1)
    M1.set_z(np.column_stack([z0, np.full(n, sigma0)]).reshape(-1, order="F"))
    call("mgb_amg_set_early_stop", M1.handle, K)
    M1.set_solver(solver)
    M1.prepare()
    SOL = M1.solve(tol=tol, schedule=schedule, solver=solver)
    z1 = M1.get_z().reshape((n, S + 1), order="F")
    if not np.max(z1[:, S]) < 0.0:
        raise MGBError(-3, "amgb: the problem is infeasible (the feasibility phase ended with a non-negative slack)")
    SOL["sigma0"] = sigma0
    return np.ascontiguousarray(z1[:, :S]), SOL


def _amgb_float32(geometry, M: "AMG", z0, tol, t, kappa, maxit, verbose):
    """Float32 main phase (the reference runs T = Float32 on its Metal backend, tolerance 1e-4: test/test_utils.jl:67-88,118-119;
    SURVEY.md section 8 f3).  The Newton loop of oracle amgb_core / newton / line search, driven from the host over the FLOAT
    instantiation of the device kernels -- objective, gradient and Hessian values through mgb_amg_f0_f32 / f1_f32 / f2_f32 -- with
    the Newton system solved by the double device Cholesky on the float-assembled values (there is no Float32 factorisation:
    fp64 runs at the fp32 vector rate on MI355X).  The iterate lives in double between centerings; s, Dz, the barrier terms, the
    gradient and the Hessian values are float.  Host-driven on purpose: the float path is for the small meshes the reference
    runs in Float32, not a hot path."""
    import time as _time
    l = M.L - 1
    R = sp.block_diag([geometry.subspaces[sv[1]][l].host for sv in M.state_variables], format="csr")
    N = R.shape[1]
    z = np.asarray(z0, dtype=np.float64).reshape(-1, order="F").copy()
    kappa0, t_begin = kappa, _time.time()
    t_stop = t
    while t_stop <= 1.0 / tol:
        t_stop *= kappa0
    max_newton, steps = 48, [0]

    def centre(zc, tc):
        M.set_z(zc)
        s = np.zeros(N, dtype=np.float32)
        y = M.f0_f32(l, s, tc)
        if not math.isfinite(y):
            return None
        g = M.f1_f32(l, s, tc).astype(np.float64)
        ymin, gmin = y, float(np.linalg.norm(g))
        for _ in range(max_newton):
            steps[0] += 1
            try:
                n = M.solve_linear(l, M.f2_f32(l, s, tc).astype(np.float64), g)
            except MGBError:
                return None
            inc = float(g @ n)
            if not math.isfinite(inc):
                return None
            if inc <= 0:
                return zc + R @ s.astype(np.float64)
            step, accepted = 1.0, False
            while step >= 1e-8:                               # backtracking: finite (amgb_all_isfinite, src:121) + Armijo
                st = (s.astype(np.float64) - step * n).astype(np.float32)
                yt = M.f0_f32(l, st, tc)
                if math.isfinite(yt) and yt <= y - 0.1 * step * inc:
                    gt = M.f1_f32(l, st, tc).astype(np.float64)
                    if np.all(np.isfinite(gt)):
                        accepted = True
                        break
                step *= 0.5
            if not accepted:
                yt, gt, st = y, g, s
            gn = float(np.linalg.norm(gt))
            done = yt >= ymin and gn >= 0.1 * gmin            # stagnation in float precision (oracle stopping_exact)
            s, y, g = st, yt, gt
            ymin, gmin = min(ymin, y), min(gmin, gn)
            if done:
                return zc + R @ s.astype(np.float64)
        return None

    def c_dot(zc):
        M.set_z(zc)
        return float(M.f0(l, np.zeros(N), 0.0, parts=True)[1][1])

    its, ts, cd = [], [], []
    zz = None
    for _ in range(8):                                        # INITIAL_CENTERING_ATTEMPTS
        zz = centre(z, t)
        if zz is not None:
            break
    if zz is None:
        raise MGBError(-3, "amgb (Float32): initial centering failed")
    z = zz
    its.append(steps[0]); ts.append(t); cd.append(c_dot(z))
    k = 1
    while t < t_stop and kappa > 1 and k < maxit:
        k += 1
        before = steps[0]
        while kappa > 1:
            t1 = min(kappa * t, t_stop)
            b1 = steps[0]
            zz = centre(z, t1)
            if zz is not None:
                if steps[0] - b1 <= max_newton * 0.25:
                    kappa = min(kappa0, kappa * kappa)
                z, t = zz, t1
                break
            kappa = math.sqrt(kappa)
            if kappa < 1 + 1e-3:
                kappa = 1.0
        its.append(steps[0] - before); ts.append(t); cd.append(c_dot(z))
        if verbose:
            print("[mgb f32] t=%.4g kappa=%.3g its=%d" % (t, kappa, its[-1]))
    if t < t_stop:
        raise MGBError(-3, "amgb (Float32): convergence failure (kappa collapsed)")
    itm = np.zeros((M.L, len(its)), dtype=np.int64)
    itm[l] = its
    M.set_z(z)
    return z.astype(np.float32).astype(np.float64), dict(t_elapsed=_time.time() - t_begin, ts=np.array(ts), its=itm,
                                                         c_dot_Dz=np.array(cd), T="float32")


def amgb(geometry: Geometry, p=1.0, state_variables=DEFAULT_STATE, D=None, f=None, g=None, tol=None, t=0.1,
         maxit=10000, kappa=10.0, verbose=False, logfile=None, schedule="fine", solver="gpu", cones=None, stop_rule="fixed",
         centering="exact", T=np.float64, dirichlet=None, neumann=None, **rest) -> AMGBSOL:
    """MultiGridBarrier.amgb on an MPI geometry (called at src:599,666).  kwargs as documented in
    docs/src/guide.md:148-152; unknown kwargs (e.g. `L`, forwarded by fem*d_mpi_solve, src:663-666)
    are ignored like Julia's `kwargs...` fan-out.  `cones` (upstream kwarg `Q`: the convex set) selects the barrier terms,
    see `AMG`; default = the p-Laplace power cone.
    Mixed boundary conditions (single-GPU contexts, T = float64): `dirichlet=where` (a boolean (nf,) array
    over boundary(geometry) or a callable on a facet centre) keeps the variables of the "dirichlet" space fixed at g on the
    selected facets only -- the subspace of dirichlet_on(), built once per geometry and selection; `neumann=h` (see
    neumann_load) adds int h u ds over the facets NOT selected to the cost, in the first row of D that is (that variable, "id").
    h enters as f does: for the default problem the natural condition on the free part is p |grad u|^(p-2) du/dn = -h.  p = 1
    is not coercive with a free boundary: whether the problem is bounded then depends on f and h, at the caller's risk."""
    if neumann is not None and dirichlet is None:
        raise ValueError("amgb: neumann= needs dirichlet= (the load acts on the facets that dirichlet= does not select)")
    if geometry._geo is None:
        raise TypeError("amgb: geometry must come from native_to_mpi / fem*d_mpi")
    dim = geometry.discretization["dim"]
    f = DEFAULT_F[dim] if f is None else f
    g = DEFAULT_G[dim] if g is None else g
    load = None
    if dirichlet is not None:
        if np.dtype(T) != np.float64:
            raise NotImplementedError("amgb: dirichlet= / neumann= are not supported with T = float32")
        state_variables, free, load_var = _mixed_state(geometry, state_variables, dirichlet, "amgb")
        if neumann is not None:
            pairs = [tuple(d) for d in (DEFAULT_D[dim] if D is None else D)]
            if (load_var, "id") not in pairs:
                raise ValueError("amgb: neumann= needs a row (%r, 'id') of D" % (load_var,))
            load = (neumann_load(geometry, neumann, where=free), pairs.index((load_var, "id")))
    M = AMG(geometry, state_variables, D, p, cones=cones, select=rest.get("select"))
    x = geometry.x.to_numpy()
    z0 = _rows(g, x)        # g_grid (n, S)
    c = _rows(f, x)         # f_grid (n, K)
    M.set_c(c)
    if load is not None:
        M.add_cost_rows(load[0], load[1])
        c = M.get_c()       # the cost the feasibility phase scales its penalty by
    M.set_z(z0.reshape(-1, order="F"))
    Nf = M.level_size(M.L - 1)[0]
    y0 = M.f0(M.L - 1, np.zeros(Nf), 0.0)
    SOL_feasibility = None
    if not math.isfinite(y0) and rest.get("select") is not None:
        raise MGBError(-3, "amgb: a piecewise set (select=) needs a strictly feasible start")
    if not math.isfinite(y0):
        # Feasibility phase (SOL_feasibility, src:428-455).  For the power-cone family it has a closed form:
        # the slack row is `id` of a :full state variable (that space contains the constants), so a constant
        # shift sigma = 1 + max(|q|^p - s) of that variable is strictly feasible.  Dz comes from the device.
        idx = M.idx
        if idx and len(M.cones) > 1:
            # general feasibility phase: the set relaxed by a slack field, path-followed until the slack is negative
            z0, SOL_feasibility = _phase1_slack(geometry, M, p, z0, c, tol, schedule, solver)
            M.set_z(z0.reshape(-1, order="F"))
            if not math.isfinite(M.f0(M.L - 1, np.zeros(Nf), 0.0)):
                raise MGBError(-3, "amgb: feasibility phase failed")
        elif not idx:
            raise MGBError(-3, "amgb: infeasible start")
        else:
            var, op = M.D[idx[-1]]
            names = [sv[0] for sv in M.state_variables]
            if op != "id" or dict(M.state_variables)[var] != "full":
                raise NotImplementedError("amgb: feasibility phase needs the cone's slack to be `id` of a :full variable")
            Dz = M.apply_D_global(M.L - 1, np.zeros(Nf))
            q2 = np.sum(Dz[:, idx[:-1]] ** 2, axis=1)
            pv = M.p_nodes if M.p_nodes is not None else p
            sigma = 1.0 + float(np.max(q2 ** (pv / 2.0) - Dz[:, idx[-1]]))
            z0[:, names.index(var)] += sigma
            M.set_z(z0.reshape(-1, order="F"))
            if not math.isfinite(M.f0(M.L - 1, np.zeros(Nf), 0.0)):
                raise MGBError(-3, "amgb: feasibility phase failed")
            SOL_feasibility = dict(shift=sigma, its=np.zeros((M.L, 0), dtype=np.int64), ts=np.zeros(0),
                                   c_dot_Dz=np.zeros(0), t_elapsed=0.0)
    if np.dtype(T) == np.float32:                             # the reference's Float32 configurations (test/test_utils.jl:67-88)
        if SOL_feasibility is not None and "shift" not in SOL_feasibility:
            raise NotImplementedError("amgb: Float32 covers the closed-form feasibility shift only")
        M.prepare()
        tol32 = float(np.sqrt(np.finfo(np.float32).eps)) if tol is None else float(tol)
        z, SOL = _amgb_float32(geometry, M, z0, tol32, t, kappa, maxit, verbose)
        return AMGBSOL(HPCMatrix(z.reshape(z0.shape, order="F"), geometry.x.backend), SOL_feasibility, SOL, [], geometry)
    if np.dtype(T) != np.float64:
        raise ValueError("T must be float64 or float32")
    M.set_solver(solver)
    if rest.get("pcg"):
        M.set_pcg(**rest["pcg"])      # parameters of solver="pcg", see AMG.set_pcg
    M.prepare()       # factorisation structures are setup, not solve time (SOL_main.t_elapsed mirrors the reference's)
    SOL = M.solve(tol=tol, t=t, kappa=kappa, maxit=maxit, verbose=2 if verbose and verbose > 1 else int(bool(verbose)),
                  schedule=schedule, solver=solver, stop_rule=stop_rule, centering=centering)
    z = M.get_z().reshape(z0.shape, order="F")
    return AMGBSOL(HPCMatrix(z, geometry.x.backend), SOL_feasibility, SOL, [], geometry)


def fem1d_mpi_solve(L: int = 4, **kwargs) -> AMGBSOL:
    """src:594-600: kwargs go to both fem1d_mpi and amgb."""
    geo_kw = {k: kwargs[k] for k in ("Ti", "backend") if k in kwargs}
    return amgb(fem1d_mpi(L, **geo_kw), **{k: v for k, v in kwargs.items() if k not in geo_kw})


def fem3d_mpi_solve(L: int = 2, k: int = 3, D=None, f=None, g=None, **kwargs) -> AMGBSOL:
    """src:735-745: 3-D defaults D = [u id; u dx; u dy; u dz; s id], f = (.5,0,0,0,1), g = (|x|^2, 100)."""
    geo_kw = {kk: kwargs[kk] for kk in ("Ti", "backend") if kk in kwargs}
    rest = {kk: v for kk, v in kwargs.items() if kk not in geo_kw}
    return amgb(fem3d_mpi(L, k, **geo_kw), D=D or DEFAULT_D[3], f=f or DEFAULT_F[3], g=g or DEFAULT_G[3], **rest)


def fem2d_mpi_solve(L: int = 2, K=None, **kwargs) -> AMGBSOL:
    """src:661-667."""
    geo_kw = {k: kwargs[k] for k in ("Ti", "backend") if k in kwargs}
    return amgb(fem2d_mpi(L, K, **geo_kw), **{k: v for k, v in kwargs.items() if k not in geo_kw})


@dataclass
class ParabolicSOL:
    """src:512-516 field order: geometry, ts, u (one n x S snapshot per time step); `lift` (this project's, trailing): the
    (nsteps, 2) slack shifts (lift_1, lift_2) applied before each step's barrier solve, None where the loop does not record them."""
    geometry: Geometry
    ts: np.ndarray
    u: list
    lift: Optional[np.ndarray] = None


def _positional_arity(fn, name, who="parabolic_solve"):
    """Number of positional parameters of the closure `fn` (1: fn(x), 2: fn(t, x)); anything else is a TypeError naming `name`."""
    import inspect
    try:
        params = inspect.signature(fn).parameters.values()
    except (TypeError, ValueError):
        raise TypeError("%s: cannot read the signature of %s; pass a function of (x) or of (t, x)" % (who, name))
    k = sum(1 for q in params if q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD))
    if k not in (1, 2) or any(q.kind == q.VAR_POSITIONAL for q in params):
        raise TypeError("%s: %s must take (x) or (t, x), not %d positional parameters" % (who, name, k))
    return k


def _parabolic_times(h, t0, t1, ts):
    """(ts, hs): the time grid and the step of every interval.  `ts=` overrides h, t0, t1 (h_k = ts[k+1] - ts[k]); without it the
    grid is t0 + h * arange(nsteps + 1) and every step is h itself."""
    if ts is None:
        nsteps = int(round((t1 - t0) / h))
        return t0 + h * np.arange(nsteps + 1), np.full(nsteps, float(h))
    ts = np.array(ts, dtype=np.float64)
    if ts.ndim != 1 or ts.size < 2:
        raise ValueError("parabolic_solve: ts must be a 1-D array with at least 2 entries")
    if not np.all(np.isfinite(ts)) or not np.all(np.diff(ts) > 0):
        raise ValueError("parabolic_solve: ts must be finite and strictly increasing")
    return ts, np.diff(ts)


def _parabolic_forcing(f1, x, ts):
    """(time_dependent, row): row(k) = the (n,) forcing of the step that ends at ts[k + 1] (implicit Euler: taken at the new time)."""
    n, nsteps = x.shape[0], len(ts) - 1
    if callable(f1):
        if _positional_arity(f1, "f1") == 1:
            fgrid = np.array([float(f1(xi)) for xi in x])
            return False, lambda k: fgrid
        return True, lambda k: np.array([float(f1(ts[k + 1], xi)) for xi in x])
    fa = f64(np.asarray(f1))
    if fa.shape == (n,):
        return False, lambda k: fa
    if fa.ndim == 2 and fa.shape == (nsteps, n):
        return True, lambda k: fa[k]
    raise ValueError("parabolic_solve: an array f1 must have shape (n,) = (%d,) or (len(ts) - 1, n) = (%d, %d), got %r"
                     % (n, nsteps, n, tuple(fa.shape)))


def _parabolic_host_loop(M, z, n, K, p, hs, fgrid, tol, verbose, schedule, solver, backend):
    """The time loop through the host (sharded contexts): z down, cost built in numpy, cost and snapshot up, every step."""
    u = [HPCMatrix(z.reshape(n, 3, order="F"), backend)]
    M.set_z(z)
    for h in hs:
        c = np.zeros((n, K))
        c[:, 0] = fgrid - z[:n] / h
        c[:, K - 2] = 1.0 / (2.0 * h)
        c[:, K - 1] = 1.0 / p
        M.set_c(c)
        M.solve(tol=tol, verbose=int(bool(verbose)), schedule=schedule, solver=solver)
        z = M.get_z()
        u.append(HPCMatrix(z.reshape(n, 3, order="F"), backend))
    return u


def parabolic_solve(geometry: Geometry, h=0.2, t0=0.0, t1=1.0, p=1.0, f1=None, g=None, tol=None, verbose=False,
                    schedule="fine", solver="gpu", ts=None, dirichlet=None, neumann=None, **rest) -> ParabolicSOL:
    """MultiGridBarrier.parabolic_solve on an MPI geometry (imported at src:22,54; kwargs h, t1, p, verbose as in
    test/test_parabolic.jl:48 and docs/src/guide.md:367,377).  Implicit Euler for
        u_t - div(|grad u|^(p-2) grad u) = -f1 ;
    the step from t_k to t_{k+1} = t_k + h_k minimises int (1/2h_k)(s1 - 2 u u_k) + (1/p) s2 + f1 u subject to s1 >= u^2,
    s2 >= |grad u|^p with the barrier of the two-cone intersection: one GPU barrier solve per step, and between two solves
    the state stays on the device (cost, boundary values, slack lifts and snapshots are kernels).
      f1: f1(x) | f1(t, x) | an (n,) array | a (len(ts) - 1, n) array, row k for the step that ends at ts[k + 1];
      g:  g(x) | g(t, x); its first component is the initial condition at ts[0] and, on the boundary nodes, the Dirichlet
          value at t_{k+1} (g(x): the boundary trace of the initial condition, time independent);
      ts: strictly increasing times (overrides h, t0, t1; h_k = ts[k + 1] - ts[k]).
    Forcing and boundary data are taken at the new time t_{k+1}.  Where new boundary values or a larger gradient push the old
    slacks out of a cone, the slack is shifted by the constant lift = 1 + max violation (0 when nothing violates) before the
    solve; the shifts are returned as `lift` (nsteps, 2).  Sharded contexts (world > 1) run time-independent data only.
      dirichlet, neumann (single-GPU contexts): `dirichlet=where` keeps u at g on the selected boundary
          facets only (dirichlet_on); `neumann=` h(x) | h(t, x), taken at t_{k+1} like f1, adds int h u ds over the other
          facets: the natural condition there is |grad u|^(p-2) du/dn = -h.  The loads of all steps come from one launch and
          are added to the step's forcing vector on the device.  p = 1 with a free boundary is at the caller's risk."""
    if neumann is not None and dirichlet is None:
        raise ValueError("parabolic_solve: neumann= needs dirichlet= (the load acts on the facets that dirichlet= does not select)")
    if geometry._geo is None:
        raise TypeError("parabolic_solve: geometry must come from native_to_mpi / fem*d_mpi")
    dim = geometry.discretization["dim"]
    g = DEFAULT_G[dim] if g is None else g
    f1 = (lambda x: 0.5) if f1 is None else f1
    g_arity = _positional_arity(g, "g")
    explicit_ts = ts is not None
    ts, hs = _parabolic_times(h, t0, t1, ts)
    nsteps = len(hs)
    ops = ("dx", "dy", "dz")[:dim]
    state = (("u", "dirichlet"), ("s1", "full"), ("s2", "full"))
    D = (("u", "id"),) + tuple(("u", o) for o in ops) + (("s1", "id"), ("s2", "id"))
    K = dim + 3
    cones = [([0, K - 2], 2.0), (list(range(1, dim + 1)) + [K - 1], float(p))]
    x = geometry.x.to_numpy()
    n = x.shape[0]
    f_timed, f_row = _parabolic_forcing(f1, x, ts)
    backend = geometry.x.backend
    if backend.world > 1 and (f_timed or g_arity == 2 or explicit_ts):
        raise NotImplementedError("parabolic_solve: sharded contexts (world > 1) are not supported with f1(t, x), g(t, x) or ts=")
    g_at = (lambda t, xi: g(t, xi)) if g_arity == 2 else (lambda t, xi: g(xi))
    space, load, load_timed = "dirichlet", None, False
    if dirichlet is not None:
        state, free, _ = _mixed_state(geometry, state, dirichlet, "parabolic_solve")
        space = state[0][1]
        if neumann is not None:
            if not callable(neumann):
                raise TypeError("parabolic_solve: neumann must be a function h(x) or h(t, x)")
            load_timed = _positional_arity(neumann, "neumann") == 2
            load = neumann_load(geometry, neumann, where=free, ts=ts[1:] if load_timed else None)      # every step: ONE launch
    M = AMG(geometry, state, D, p, cones=cones)
    u0 = np.array([np.asarray(g_at(ts[0], xi), dtype=np.float64).reshape(-1)[0] for xi in x])
    grad2 = sum((geometry.operators[o].host @ u0) ** 2 for o in ops)
    z = np.concatenate([u0, np.full(n, 1.0 + float(np.max(u0 * u0))),
                        np.full(n, 1.0 + float(np.max(grad2 ** (p / 2.0))))])
    if backend.world > 1:
        return ParabolicSOL(geometry, ts, _parabolic_host_loop(M, z, n, K, p, hs, f_row(0), tol, verbose, schedule, solver, backend))
    bidx = np.flatnonzero(np.diff(geometry.subspaces[space][-1].host.indptr) == 0)
    M.set_z(z)
    M.parabolic_begin(bidx)
    u = [M.snapshot()]
    lift = np.zeros((nsteps, 2))
    fv = None
    for k in range(nsteps):
        if fv is None or f_timed or load_timed:
            fv = HPCVector(f_row(k), backend)
            if load is not None:
                load.add_to(fv, k if load_timed else 0)
        gb = None
        if g_arity == 2:
            gb = HPCVector(np.array([np.asarray(g(ts[k + 1], x[b]), dtype=np.float64).reshape(-1)[0] for b in bidx]), backend)
        M.parabolic_step(hs[k], p, fv, gb, wait=False)      # enqueued: the solve starts behind it without a host round trip
        try:
            M.solve(tol=tol, verbose=int(bool(verbose)), schedule=schedule, solver=solver)
        except MGBError:
            M.parabolic_lifts()      # a non-finite state is the cause if there is one: report that instead
            raise
        lift[k] = M.parabolic_lifts()
        u.append(M.snapshot())
    return ParabolicSOL(geometry, ts, u, lift)


# --------------------------------------------------------------------------- evaluation at arbitrary points


def _locator_of(geometry: Geometry):
    if geometry._geo is None:
        raise TypeError("interpolate: geometry must come from native_to_mpi / fem*d_mpi")
    backend = geometry.x.backend
    if backend.world > 1:
        raise NotImplementedError("interpolate: sharded contexts (world > 1) are not supported")
    if geometry._locator is None:
        h = C.c_void_p()
        call("mgb_locator_create", backend.handle, geometry._geo, C.byref(h))
        geometry._locator = h
    return geometry._locator, backend


def _nodal_values(geometry: Geometry, z, backend, who):
    """z as a device vector of n x S row-major nodal values of `geometry`, and S."""
    if z is None:
        raise ValueError("%s: z= is required with a Geometry" % who)
    n = len(geometry.w)
    if isinstance(z, HPCMatrix) and z.backend is backend:
        zv, zshape = z._v, z.shape
    elif isinstance(z, HPCVector) and z.backend is backend:
        zv, zshape = z, (len(z), 1)
    else:
        za = f64(np.asarray(_to_cpu_array(z)))
        za = za.reshape(za.shape[0], -1) if za.ndim else za.reshape(1, 1)
        zv, zshape = HPCVector(za, backend), za.shape
    if zshape[0] != n or zshape[1] < 1:
        raise ValueError("%s: z must have one row per node of the geometry (%d), got shape %r" % (who, n, tuple(zshape)))
    return zv, int(zshape[1])


def interpolate(obj, points, z=None, grad=False, return_element=False):
    """Evaluate nodal values at arbitrary points on the device (csrc/interp.hip; contract in include/mgb_hip.h and DESIGN.md
    section 4d).  `obj`: an AMGBSOL (its z and geometry), a ParabolicSOL (all snapshots stacked column-wise, ONE launch,
    result (T, m, S)) or a device Geometry with `z=` an (n,) / (n, S) array, HPCVector or HPCMatrix.  `points`: (m, dim), or
    (m,) in 1-D.  Returns vals (m, S) [, grads (m, S, dim) if grad] [, elem (m,) int32 if return_element].  A point outside
    the mesh (or with a non-finite coordinate) gives NaN in every column and element -1."""
    T = None
    if isinstance(obj, AMGBSOL):
        geometry, z = obj.geometry, (obj.z if z is None else z)
    elif isinstance(obj, ParabolicSOL):
        geometry = obj.geometry
        if z is None:
            T = len(obj.u)
            z = np.hstack([np.asarray(_to_cpu_array(uk)).reshape(len(geometry.w), -1) for uk in obj.u])
    elif isinstance(obj, Geometry):
        geometry = obj
    else:
        raise TypeError("interpolate: expected an AMGBSOL, a ParabolicSOL or a Geometry")
    loc, backend = _locator_of(geometry)
    dim = geometry.discretization["dim"]
    zv, S = _nodal_values(geometry, z, backend, "interpolate")
    pts = f64(np.asarray(points))
    if pts.ndim == 1 and dim == 1:
        pts = pts.reshape(-1, 1)
    if pts.ndim != 2 or pts.shape[1] != dim:
        raise ValueError("interpolate: points must have shape (m, %d)" % dim)
    m = pts.shape[0]
    pv = HPCVector(pts, backend)
    vals = HPCVector(m * S, backend)
    grads = HPCVector(m * S * dim, backend) if grad else None
    elem = np.empty(m, dtype=np.int32) if return_element else None
    call("mgb_interpolate", loc, m, pv.handle, S, zv.handle, vals.handle, grads.handle if grad else None, iptr(elem))
    out = [vals.to_numpy().reshape(m, S)]
    if grad:
        out.append(grads.to_numpy().reshape(m, S, dim))
    if T is not None:      # columns are (snapshot, state variable)
        out[0] = out[0].reshape(m, T, S // T).transpose(1, 0, 2)
        if grad:
            out[1] = out[1].reshape(m, T, S // T, dim).transpose(1, 0, 2, 3)
    if return_element:
        out.append(elem)
    return out[0] if len(out) == 1 else tuple(out)


def sample_grid(obj, shape, bounds=None, z=None):
    """Sample on a regular grid (what a plot needs): `shape` = points per axis, slowest axis first -- (ny, nx) in 2-D --,
    `bounds` = (lower corner, upper corner), default the bounding box of the nodes.  Returns X (*shape, dim) and the values
    (*shape, S) -- (T, *shape, S) for a ParabolicSOL --, NaN outside the mesh."""
    geometry = obj if isinstance(obj, Geometry) else obj.geometry
    dim = geometry.discretization["dim"]
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
    if len(shape) != dim or min(shape) < 1:
        raise ValueError("sample_grid: shape must give one positive point count per axis (%d)" % dim)
    if bounds is None:
        x = np.asarray(_to_cpu_array(geometry.x)).reshape(-1, dim)
        lo, hi = x.min(axis=0), x.max(axis=0)
    else:
        lo, hi = (f64(np.asarray(b)).reshape(dim) for b in bounds)
    axes = [np.linspace(lo[a], hi[a], shape[dim - 1 - a]) for a in range(dim)]
    mesh = np.meshgrid(*axes[::-1], indexing="ij")                      # slowest axis first
    X = np.stack(mesh[::-1], axis=-1)
    vals = interpolate(obj, X.reshape(-1, dim), z=z)
    if vals.ndim == 3:
        return X, vals.reshape((vals.shape[0],) + shape + (vals.shape[-1],))
    return X, vals.reshape(shape + (vals.shape[-1],))


# --------------------------------------------------------------------------- norms and errors of solutions


@dataclass
class FieldNorms:
    """Result of norms() / error(): (S,) arrays by the nodal quadrature rule -- `integral` = sum w d (signed), `lq` =
    (sum w |d|^q)^(1/q), `w1q` = (sum w |grad d|_2^q)^(1/q), `max` = max |d|, `gradmax` = max |grad d|_2 -- the raw `sums`
    (S x 5, the columns of mgb_field_norms), `q`, and `outside`: nodes that lie in no element of the other mesh."""
    integral: np.ndarray
    lq: np.ndarray
    w1q: np.ndarray
    max: np.ndarray
    gradmax: np.ndarray
    sums: np.ndarray
    q: float
    outside: int = 0


def _field_norms(geometry, zv, S, q, ref_vals=None, ref_grads=None, other=None, z_other=None, sign=1.0) -> FieldNorms:
    loc, _ = _locator_of(geometry)
    q = float(q)
    if not (math.isfinite(q) and q >= 1.0):
        raise ValueError("norms: q must be a finite real >= 1, got %r" % (q,))
    sums = np.empty((S, 5))
    outside = C.c_longlong(0)
    call("mgb_field_norms", loc, S, zv.handle, q, ref_vals.handle if ref_vals is not None else None,
         ref_grads.handle if ref_grads is not None else None, other, z_other.handle if z_other is not None else None,
         dptr(sums), C.byref(outside))
    sums[:, 0] *= sign
    return FieldNorms(sums[:, 0].copy(), sums[:, 1] ** (1.0 / q), sums[:, 2] ** (1.0 / q), sums[:, 3].copy(), sums[:, 4].copy(),
                      sums, q, int(outside.value))


def _field_of(obj, who, z=None):
    """(geometry, z) of an AMGBSOL, a (Geometry, z) pair or a Geometry with z=."""
    if isinstance(obj, AMGBSOL):
        return obj.geometry, (obj.z if z is None else z)
    if isinstance(obj, Geometry):
        return obj, z
    if isinstance(obj, tuple) and len(obj) == 2 and isinstance(obj[0], Geometry):
        return obj
    raise TypeError("%s: expected an AMGBSOL or a (Geometry, z) pair" % who)


def norms(obj, z=None, q=2.0) -> FieldNorms:
    """L^q norm, W^{1,q} seminorm, integral and maxima of nodal values by the nodal quadrature rule, on the device
    (csrc/norms.hip; contract in include/mgb_hip.h and DESIGN.md section 4e).  `obj`, `z`: as for interpolate -- an AMGBSOL,
    or a device Geometry with `z=` an (n,) / (n, S) array, HPCVector or HPCMatrix.  One entry per column."""
    geometry, z = _field_of(obj, "norms", z)
    _, backend = _locator_of(geometry)
    zv, S = _nodal_values(geometry, z, backend, "norms")
    return _field_norms(geometry, zv, S, q)


def error(a, b, q=2.0, grad=None, on=None, allow_outside=False) -> FieldNorms:
    """Norms of the difference a - b (csrc/norms.hip).  `a`: an AMGBSOL or a (Geometry, z) pair.  `b`: a callable
    x_row -> S values evaluated on the host at the nodes (like `f` and `g` of amgb), with `grad=` a callable x_row -> (S, dim)
    for the exact gradient; or an (n, S) array of nodal values (`grad=` an (n, S, dim) array); or another AMGBSOL /
    (Geometry, z) pair on a different mesh of the same dimension.  Without `grad=` the gradient of the reference is the element
    gradient of its nodal values.  For two meshes the quadrature runs on the one with more nodes (`on="a"` / `on="b"`
    overrides) and the other field is evaluated there by its own polynomials; the signed integral is always that of a - b;
    nodes outside the other mesh are counted in `outside` and raise ValueError unless allow_outside."""
    ga, za = _field_of(a, "error")
    _, backend = _locator_of(ga)
    zv, S = _nodal_values(ga, za, backend, "error")
    n, dim = len(ga.w), ga.discretization["dim"]
    if on not in (None, "a", "b"):
        raise ValueError("error: on must be None, 'a' or 'b'")
    if isinstance(b, AMGBSOL) or (isinstance(b, tuple) and len(b) == 2 and isinstance(b[0], Geometry)):
        if grad is not None:
            raise ValueError("error: grad= goes with a callable or an array, not with a second mesh")
        gb, zb = _field_of(b, "error")
        _, backend_b = _locator_of(gb)
        if backend_b is not backend:
            raise ValueError("error: the two fields live on different backends")
        if gb.discretization["dim"] != dim:
            raise ValueError("error: the two meshes have different dimensions (%d and %d)" % (dim, gb.discretization["dim"]))
        if gb.discretization.get("k") != ga.discretization.get("k"):
            raise ValueError("error: the two meshes have elements of different degrees")
        zbv, Sb = _nodal_values(gb, zb, backend, "error")
        if Sb != S:
            raise ValueError("error: a has %d columns, b has %d" % (S, Sb))
        on_a = len(gb.w) <= n if on is None else on == "a"
        if on_a:
            res = _field_norms(ga, zv, S, q, other=_locator_of(gb)[0], z_other=zbv)
        else:
            res = _field_norms(gb, zbv, S, q, other=_locator_of(ga)[0], z_other=zv, sign=-1.0)
    else:
        if on == "b":
            raise ValueError("error: on='b' needs a second mesh")
        x = np.asarray(_to_cpu_array(ga.x)).reshape(n, dim)
        rows = lambda f, shape: np.array([np.asarray(f(xi), dtype=np.float64).reshape(shape) for xi in x])
        rv = rows(b, (-1,)) if callable(b) else f64(np.asarray(_to_cpu_array(b)))
        rv = rv.reshape(rv.shape[0], -1) if rv.ndim else rv.reshape(1, 1)
        if rv.shape != (n, S):
            raise ValueError("error: b must give %d values per node on %d nodes, got shape %r" % (S, n, rv.shape))
        rg = None
        if grad is not None:
            rg = rows(grad, (-1, dim)) if callable(grad) else f64(np.asarray(_to_cpu_array(grad)))
            if rg.size != n * S * dim or (rg.ndim == 3 and rg.shape != (n, S, dim)):
                raise ValueError("error: grad must give (%d, %d) values per node on %d nodes" % (S, dim, n))
            rg = HPCVector(f64(rg).reshape(-1), backend)
        res = _field_norms(ga, zv, S, q, ref_vals=HPCVector(f64(rv).reshape(-1), backend), ref_grads=rg)
    if res.outside > 0 and not allow_outside:
        raise ValueError("error: %d quadrature nodes lie outside the other mesh (allow_outside=True skips them)" % res.outside)
    return res


@dataclass
class Convergence:
    """Result of convergence(): `errors` (one FieldNorms per level), the stacked `lq`, `w1q`, `max`, `gradmax` (levels x S) and
    the observed orders log2(e_l / e_{l+1}) of each ((levels - 1) x S)."""
    errors: list
    lq: np.ndarray
    w1q: np.ndarray
    max: np.ndarray
    gradmax: np.ndarray
    order_lq: np.ndarray
    order_w1q: np.ndarray
    order_max: np.ndarray
    order_gradmax: np.ndarray


def convergence(sols, exact=None, grad=None, q=2.0) -> Convergence:
    """Errors of the solutions `sols` (coarse to fine, each mesh the refinement of the one before) against `exact` (and its
    gradient `grad`: callables as for error), or against the finest solution when `exact` is None, and the observed orders
    log2(e_l / e_{l+1}).  Host glue around error()."""
    sols = list(sols)
    if exact is None:
        if len(sols) < 2:
            raise ValueError("convergence: at least two solutions are needed without an exact one")
        errs = [error(s, sols[-1], q=q) for s in sols[:-1]]
    else:
        errs = [error(s, exact, q=q, grad=grad) for s in sols]
    stack = lambda name: np.array([getattr(e, name) for e in errs]).reshape(len(errs), -1)
    cols = {name: stack(name) for name in ("lq", "w1q", "max", "gradmax")}
    with np.errstate(divide="ignore", invalid="ignore"):
        orders = {name: np.log2(v[:-1] / v[1:]) for name, v in cols.items()}
    return Convergence(errs, cols["lq"], cols["w1q"], cols["max"], cols["gradmax"], orders["lq"], orders["w1q"], orders["max"],
                       orders["gradmax"])


# --------------------------------------------------------------------------- energy, flux and cone margin of solutions


@dataclass
class Energy:
    """Result of energy(), by the nodal quadrature rule: `gradient` = int (1/p) |grad u|^p, `load` = int f u, `total` =
    gradient + load, `slack_gap` = int (s - |grad u|^p) / p, `margin` = -max (|grad u|^p - s) (negative: a node lies outside its
    cone), `flux_max` = max |grad u|^(p-1).  Floats for one field; arrays of len(ts) for a ParabolicSOL, whose `ts` is carried."""
    gradient: object
    load: object
    total: object
    slack_gap: object
    margin: object
    flux_max: object
    ts: Optional[np.ndarray] = None


def _energy_exponent(p, x, who):
    """(scalar p, per-node exponents or None) of a scalar, a callable p(x) or an (n,) array: the forms amgb takes."""
    n = x.shape[0]
    if callable(p):
        pn = np.array([float(p(xi)) for xi in x])
    elif np.isscalar(p):
        if isinstance(p, (str, bytes)):
            raise TypeError("%s: p must be a scalar, a callable p(x) or an (n,) array, got %r" % (who, p))
        p = float(p)
        if not (math.isfinite(p) and p >= 1.0):
            raise ValueError("%s: p must be a finite real >= 1, got %r" % (who, p))
        return p, None
    else:
        try:
            pn = f64(np.asarray(_to_cpu_array(p)))
        except (TypeError, ValueError):
            raise TypeError("%s: p must be a scalar, a callable p(x) or an (n,) array" % who)
        if pn.shape != (n,):
            raise ValueError("%s: an array p must have shape (n,) = (%d,), got %r" % (who, n, tuple(pn.shape)))
    if not (np.all(np.isfinite(pn)) and np.all(pn >= 1.0)):
        raise ValueError("%s: p must give one finite value >= 1 per node" % who)
    return float(pn[0]), pn


def _energy_forcing(f, x, ts, B, who):
    """None or the (rows, n) forcing, rows 1 or B, of a scalar, f(x), an (n,) array or -- with ts -- f(t, x) / (len(ts), n).
    A callable is f(x) or f(t, x) by the number of its positional parameters WITHOUT a default."""
    n = x.shape[0]
    if f is None:
        return None
    if callable(f):
        import inspect
        try:
            params = inspect.signature(f).parameters.values()
            k = sum(1 for q in params if q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD) and q.default is q.empty)
        except (TypeError, ValueError):
            k = 1
        if k == 2:
            if ts is None:
                raise TypeError("%s: f(t, x) goes with a ParabolicSOL; pass f(x) here" % who)
            return np.array([[float(f(t, xi)) for xi in x] for t in ts])
        if k != 1:
            raise TypeError("%s: f must take (x) or (t, x), not %d positional parameters without a default" % (who, k))
        return np.array([float(f(xi)) for xi in x]).reshape(1, n)
    if np.isscalar(f):
        return np.full((1, n), float(f))
    fa = f64(np.asarray(_to_cpu_array(f)))
    if fa.shape == (n,):
        return fa.reshape(1, n)
    if ts is not None and fa.shape == (B, n):
        return fa
    if ts is not None:
        raise ValueError("%s: an array f must have shape (n,) = (%d,) or (len(ts), n) = (%d, %d), got %r"
                         % (who, n, B, n, tuple(fa.shape)))
    raise ValueError("%s: an array f must have shape (n,) = (%d,), got %r" % (who, n, tuple(fa.shape)))


def _energy_column(v, S, name, who):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s: %s must be a column index (an int), got %r" % (who, name, v))
    c = int(v) + S if v < 0 else int(v)
    if not 0 <= c < S:
        raise ValueError("%s: column %s = %d is outside the %d columns of z" % (who, name, v, S))
    return c


def energy(obj, p, f=None, u=0, s=-1, z=None) -> Energy:
    """Energy J(u) = int (1/p) |grad u|^p + f u, slack gap, cone margin and largest flux of a solution, reduced on the device
    (csrc/energy.hip; contract in include/mgb_hip.h and DESIGN.md section 4g).  `obj`: an AMGBSOL, a device Geometry with `z=`
    an (n, S) array or HPCMatrix, or a ParabolicSOL, whose len(ts) snapshots are reduced by ONE pair of launches.  `p`: a
    scalar, a callable p(x) or an (n,) array; `f`: None (no load), a scalar, f(x), an (n,) array, and for a ParabolicSOL also
    f(t, x) or a (len(ts), n) array, row k going with snapshot k; `u`, `s`: the columns of the solution and of its slack
    (negative: from the end)."""
    ts = None
    if isinstance(obj, ParabolicSOL):
        if z is not None:
            raise ValueError("energy: z= does not go with a ParabolicSOL (its snapshots are the fields)")
        geometry, fields, ts = obj.geometry, list(obj.u), np.asarray(obj.ts)
        if len(fields) != len(ts) or not fields:
            raise ValueError("energy: the ParabolicSOL has %d snapshots for %d times" % (len(fields), len(ts)))
    elif isinstance(obj, (AMGBSOL, Geometry)):
        geometry, z = _field_of(obj, "energy", z)
        fields = [z]
    else:
        raise TypeError("energy: expected an AMGBSOL, a ParabolicSOL or a Geometry")
    if geometry._geo is None:
        raise TypeError("energy: geometry must come from native_to_mpi / fem*d_mpi")
    if geometry.x.backend.world > 1:
        raise NotImplementedError("energy: sharded contexts (world > 1) are not supported")
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "energy") for zk in fields]
    B, S = len(vecs), vecs[0][1]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("energy: the snapshots have different numbers of columns")
    if S < 2:
        raise ValueError("energy: z must have a solution column and a slack column, got %d column" % S)
    u, s = _energy_column(u, S, "u", "energy"), _energy_column(s, S, "s", "energy")
    if u == s:
        raise ValueError("energy: u and s are the same column (%d)" % u)
    x = np.asarray(_to_cpu_array(geometry.x)).reshape(len(geometry.w), -1)
    p0, pn = _energy_exponent(p, x, "energy")
    fa = _energy_forcing(f, x, ts, B, "energy")
    pv = HPCVector(pn, backend) if pn is not None else None
    fv = HPCVector(fa, backend) if fa is not None else None
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    out = np.empty((B, 5))
    call("mgb_geo_field_energy", loc, B, table, S, u, s, p0, pv.handle if pv is not None else None,
         fv.handle if fv is not None else None, fa.shape[0] if fa is not None else 1, dptr(out))
    cols = [out[:, 0].copy(), out[:, 1].copy(), out[:, 0] + out[:, 1], out[:, 2].copy(), -out[:, 4], out[:, 3].copy()]
    if ts is None:
        return Energy(*[float(c[0]) for c in cols])
    return Energy(*cols, ts=ts)


def flux(obj, p, u=0, z=None, k=-1) -> HPCMatrix:
    """The flux sigma = |grad u|^(p-2) grad u at the nodes, each in its own element: an (n, dim) HPCMatrix that stays on the
    device (csrc/energy.hip).  `obj`, `p`, `u`: as for energy; `k` selects the snapshot of a ParabolicSOL.  It is the gradient
    itself at p = 2 and exactly 0 where the gradient vanishes."""
    if isinstance(obj, ParabolicSOL):
        if z is not None:
            raise ValueError("flux: z= does not go with a ParabolicSOL (k= selects a snapshot)")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not -len(obj.u) <= k < len(obj.u):
            raise ValueError("flux: k = %r is not one of the %d snapshots" % (k, len(obj.u)))
        geometry, z = obj.geometry, obj.u[int(k)]
    elif isinstance(obj, (AMGBSOL, Geometry)):
        geometry, z = _field_of(obj, "flux", z)
    else:
        raise TypeError("flux: expected an AMGBSOL, a ParabolicSOL or a Geometry")
    if geometry._geo is None:
        raise TypeError("flux: geometry must come from native_to_mpi / fem*d_mpi")
    if geometry.x.backend.world > 1:
        raise NotImplementedError("flux: sharded contexts (world > 1) are not supported")
    loc, backend = _locator_of(geometry)
    zv, S = _nodal_values(geometry, z, backend, "flux")
    u = _energy_column(u, S, "u", "flux")
    n, dim = len(geometry.w), geometry.discretization["dim"]
    p0, pn = _energy_exponent(p, np.asarray(_to_cpu_array(geometry.x)).reshape(n, -1), "flux")
    pv = HPCVector(pn, backend) if pn is not None else None
    out = HPCMatrix.__new__(HPCMatrix)
    out.shape, out.backend = (n, dim), backend
    out._v = HPCVector(n * dim, backend)
    call("mgb_geo_field_flux", loc, zv.handle, S, u, p0, pv.handle if pv is not None else None, out._v.handle)
    out._inputs = (zv, pv)      # the launch is not waited for: what it reads lives as long as what it writes
    return out


# --------------------------------------------------------------------------- level sets of solutions


class LevelSets:
    """Result of level_sets(): per field and level `above` = measure of {u > c}, `length` = measure of {u = c} (2-D: the length
    of the contour; 1-D: the number of crossings), `excess` = int_{u > c} (u - c), `count` = the number of segments (1-D:
    crossings), `reached` = the level lies strictly inside the range of the lattice values.  Floats for one field and a scalar
    level; an axis of len(ts) in front for a ParabolicSOL (whose `ts` is carried), an axis of len(levels) behind for an array of
    levels.  `rows` is the (B, nl, 5) table of the C ABI.  `segments(level, step)` gives the (m, 2, 2) contour segments
    [[x0, y0], [x1, y1]] of levels[level] in snapshot `step`, the above side on their left, in ascending item order, and
    `elements(level, step)` the element of each; in 1-D `points(level, step)` and `directions(level, step)` take their place."""

    def __init__(self, levels, rows, counts, ts, squeeze, dim, refine, offsets=None, seg=None, item=None):
        self.levels, self.rows, self.ts, self.dim, self.refine = levels, rows, ts, dim, refine
        self._counts, self._offsets, self._seg, self._item = counts, offsets, seg, item

        def shape(a):
            a = a[:, 0] if squeeze[1] else a
            a = a[0] if squeeze[0] else a
            return a if np.ndim(a) else a.item()

        self.above, self.length, self.excess = (shape(rows[:, :, k].copy()) for k in range(3))
        self.count = shape(counts.copy())
        self.reached = shape((rows[:, :, 3] > 0.0) & (rows[:, :, 4] > 0.0))

    def _row(self, level, step, who):
        B, nl = self._counts.shape
        if self._offsets is None:
            raise ValueError("LevelSets.%s: level_sets was called with segments=False" % who)
        for v, m, name in ((level, nl, "level"), (step, B, "step")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -m <= v < m:
                raise IndexError("LevelSets.%s: %s = %r is not one of %d" % (who, name, v, m))
        r = (int(step) % B) * nl + int(level) % nl
        return int(self._offsets[r]), int(self._offsets[r + 1])

    def _need_dim(self, dim, who, other):
        if self.dim != dim:
            raise ValueError("LevelSets.%s: a %d-D result has %s" % (who, self.dim, other))

    def segments(self, level=0, step=0) -> np.ndarray:
        self._need_dim(2, "segments", "points() and directions()")
        a, b = self._row(level, step, "segments")
        return self._seg[a:b].reshape(-1, 2, 2).copy()

    def elements(self, level=0, step=0) -> np.ndarray:
        a, b = self._row(level, step, "elements")
        return self._item[a:b] // (6 * 4 ** self.refine if self.dim == 2 else 1)

    def points(self, level=0, step=0) -> np.ndarray:
        self._need_dim(1, "points", "segments()")
        a, b = self._row(level, step, "points")
        return self._seg[a:b, 0].copy()

    def directions(self, level=0, step=0) -> np.ndarray:
        self._need_dim(1, "directions", "segments()")
        a, b = self._row(level, step, "directions")
        return self._seg[a:b, 1].astype(np.int64)

    def __repr__(self):
        return "LevelSets(levels=%r, above=%r, length=%r, count=%r)" % (self.levels, self.above, self.length, self.count)


def _level_fields(who, obj, z):
    """(geometry, fields, ts) of level_sets() and isosurfaces(): the snapshots of a ParabolicSOL with its times, or the one
    field of an AMGBSOL or of a Geometry with z=; on one rank."""
    ts = None
    if isinstance(obj, ParabolicSOL):
        if z is not None:
            raise ValueError("%s: z= does not go with a ParabolicSOL (its snapshots are the fields)" % who)
        geometry, fields, ts = obj.geometry, list(obj.u), np.asarray(obj.ts)
        if len(fields) != len(ts) or not fields:
            raise ValueError("%s: the ParabolicSOL has %d snapshots for %d times" % (who, len(fields), len(ts)))
    elif isinstance(obj, (AMGBSOL, Geometry)):
        geometry, z = _field_of(obj, who, z)
        fields = [z]
    else:
        raise TypeError("%s: expected an AMGBSOL, a ParabolicSOL or a Geometry" % who)
    if geometry._geo is None:
        raise TypeError("%s: geometry must come from native_to_mpi / fem*d_mpi" % who)
    if geometry.x.backend.world > 1:
        raise NotImplementedError("%s: sharded contexts (world > 1) are not supported" % who)
    return geometry, fields, ts


def _level_values(who, levels):
    """(levels as a contiguous 1-D float64 array, whether a scalar was given)"""
    try:
        lv = np.asarray(levels.to_numpy() if hasattr(levels, "to_numpy") else levels, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s: levels must be a scalar or a 1-D array of them" % who)
    scalar = lv.ndim == 0      # before f64(): ascontiguousarray gives a 0-d array one axis
    lv = f64(lv.reshape(-1) if scalar else lv)
    if lv.ndim != 1 or lv.size < 1:
        raise ValueError("%s: levels must be a scalar or a non-empty 1-D array, got shape %r" % (who, tuple(lv.shape)))
    if not np.all(np.isfinite(lv)):
        raise ValueError("%s: every level must be finite" % who)
    return lv, scalar


def level_sets(obj, levels, u=0, z=None, refine=0, segments=True) -> LevelSets:
    """Where a solution takes given values: the contour {u = c} of the finite-element function, its length, the area of
    {u > c} and int_{u > c} (u - c), measured on the device (csrc/levelset.hip; the rule is in include/mgb_hip.h and DESIGN.md
    section 4n).  `obj`: an AMGBSOL, a device Geometry with `z=` an (n,) / (n, S) array or HPCMatrix, or a ParabolicSOL, all of
    whose snapshots are measured by ONE set of launches.  `levels`: a finite scalar or a 1-D array of them; `u`: the column
    (negative: from the end).  `refine` = 0..3 (2-D): every element is cut into 6 * 4^refine triangles on which u is taken as
    linear; 0 uses the nodal values alone and gives a watertight contour, each further step divides the error of a smooth
    contour by about 4.  `segments=False` leaves out the segments -- one launch and one copy less -- for front histories.
    1-D geometries give crossing points; 3-D ones raise NotImplementedError here: isosurfaces() is their entry point."""
    geometry, fields, ts = _level_fields("level_sets", obj, z)
    dim = geometry.discretization["dim"]
    if dim == 3:
        raise NotImplementedError("level_sets: isosurfaces of 3-D fields are not covered")
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= refine <= (3 if dim == 2 else 0):
        raise ValueError("level_sets: refine must be %s, got %r" % ("0, 1, 2 or 3" if dim == 2 else "0 in 1-D", refine))
    lv, scalar = _level_values("level_sets", levels)
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "level_sets") for zk in fields]
    B, S, nl = len(vecs), vecs[0][1], lv.size
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("level_sets: the snapshots have different numbers of columns")
    u = _energy_column(u, S, "u", "level_sets")
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows, counts = np.empty((B, nl, 5)), np.empty((B, nl), dtype=np.int64)
    h = C.c_void_p()
    call("mgb_geo_level_sets", loc, B, table, S, u, nl, dptr(lv), int(refine), dptr(rows),
         counts.ctypes.data_as(_lib.c_ll_p), C.byref(h) if segments else None)
    offsets = seg = item = None
    if segments:
        try:
            total = int(counts.sum())
            offsets, seg, item = np.empty(B * nl + 1, dtype=np.int64), np.empty((total, 4 if dim == 2 else 2)), np.empty(total, dtype=np.int32)
            call("mgb_levelset_get", h, offsets.ctypes.data_as(_lib.c_ll_p), dptr(seg), iptr(item))
        finally:
            call("mgb_levelset_destroy", h)
    return LevelSets(lv[0].item() if scalar else lv, rows, counts, ts, (ts is None, scalar), dim, int(refine), offsets, seg, item)


# --------------------------------------------------------------------------- time statistics of parabolic runs


class TimeStats:
    """Result of time_stats(): what every node saw over the window `ts` of a run.  `node` (n, 8) and `level` (nl * n, 5;
    None without levels) are the HPCMatrix tables of the C ABI and stay on the device; the array attributes copy a table on
    first use and cache it.  Per node, shape (n,): `integral`, `mean` (= integral / (ts[-1] - ts[0])), `max`, `tmax`, `min`,
    `tmin`, `variation`, `rate`, `change`.  Per node and level, (n,) for a scalar level and (n, nl) for an array: `arrival`,
    `left` (the value `never` where there is none), `exposure`, `excess`, `entries` (int64), `reached` (= entries > 0).
    Totals, floats: `total`, `total_variation`, `total_change`, `peak`, `trough`; per level (a float for a scalar level):
    `reached_measure`, `exposure_total`, `excess_total`, `last_arrival` (-inf where nothing was reached), `longest_exposure`.
    `rows` is the raw (1 + nl, 5) table.  A node with a non-finite value in the window holds NaN everywhere (`entries` then
    reads as the smallest int64 and `reached` as False)."""

    _NODE = {"integral": 0, "max": 1, "tmax": 2, "min": 3, "tmin": 4, "variation": 5, "rate": 6, "change": 7}
    _LEVEL = {"arrival": 0, "left": 1, "exposure": 2, "excess": 3}
    _ROW0 = {"total": 0, "total_variation": 1, "total_change": 2, "peak": 3}
    _ROWL = {"reached_measure": 0, "exposure_total": 1, "excess_total": 2, "last_arrival": 3, "longest_exposure": 4}

    def __init__(self, node, level, rows, ts, levels, scalar):
        self.node, self.level, self.rows, self.ts, self.levels = node, level, rows, ts, levels
        self._scalar, self._node_host, self._level_host = scalar, None, None

    def _node_table(self):
        if self._node_host is None:
            self._node_host = self.node.to_numpy()
        return self._node_host

    def _level_table(self, name):
        if self.level is None:
            raise ValueError("TimeStats.%s: time_stats was called without levels" % name)
        if self._level_host is None:
            n = self.node.shape[0]
            self._level_host = self.level.to_numpy().reshape(-1, n, 5)
        return self._level_host

    def _per_level(self, a):
        return a[0].copy() if self._scalar else a.T.copy()

    def __getattr__(self, name):
        if name in TimeStats._NODE:
            return self._node_table()[:, TimeStats._NODE[name]].copy()
        if name in TimeStats._LEVEL:
            return self._per_level(self._level_table(name)[:, :, TimeStats._LEVEL[name]])
        if name in TimeStats._ROW0:
            return float(self.rows[0, TimeStats._ROW0[name]])
        if name in TimeStats._ROWL:
            if self.level is None:
                raise ValueError("TimeStats.%s: time_stats was called without levels" % name)
            col = self.rows[1:, TimeStats._ROWL[name]]
            return float(col[0]) if self._scalar else col.copy()
        raise AttributeError(name)

    @property
    def mean(self) -> np.ndarray:
        return self.integral / (self.ts[-1] - self.ts[0])

    @property
    def trough(self) -> float:
        return -float(self.rows[0, 4])

    @property
    def entries(self) -> np.ndarray:
        with np.errstate(invalid="ignore"):
            return self._per_level(self._level_table("entries")[:, :, 4]).astype(np.int64)

    @property
    def reached(self) -> np.ndarray:
        return self._per_level(self._level_table("reached")[:, :, 4]) > 0.0

    def __repr__(self):
        return "TimeStats(ts=[%g .. %g], levels=%r, total=%r, peak=%r, trough=%r)" % (
            self.ts[0], self.ts[-1], self.levels, self.total, self.peak, self.trough)


def _snapshot_index(v, T, name, who):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s: %s must be a snapshot index (an int), got %r" % (who, name, v))
    if not -T <= v < T:
        raise ValueError("%s: %s = %d is not one of the %d snapshots" % (who, name, v, T))
    return int(v) % T


def time_stats(par, levels=None, u=0, start=0, stop=None, never=float("nan")) -> TimeStats:
    """What every node of a ParabolicSOL saw over time, reduced along the time axis on the device (csrc/timestat.hip; the rule
    is in include/mgb_hip.h and DESIGN.md section 4u): the trapezoid integral (the dose), peak and trough with their times,
    total variation, the largest rate of change, and per level c the arrival time (first rise above c, interpolated linearly
    between snapshots), the last time the value fell back, the time spent above c and the integral of the excess over c.
    `u`: the column (negative: from the end); `start`, `stop`: the first and the last snapshot of the window (negative: from
    the end; stop=None: the last), at least 2 snapshots; `levels`: None, a finite scalar or a 1-D array; `never`: the value of
    `arrival` / `left` where there is none -- NaN, or any float, e.g. ts[-1] + 1 to draw isochrones with
    level_sets(geometry, c, z=st.arrival).  One statistics launch and one finish launch whatever len(ts) and len(levels) are
    (every 4 levels read the run once more: 1 + ceil(len(levels) / 4) passes); the per-node tables stay on the device (TimeStats.node, TimeStats.level)."""
    who = "time_stats"
    if not isinstance(par, ParabolicSOL):
        raise TypeError("time_stats: expected a ParabolicSOL")
    geometry, fields, ts = _level_fields(who, par, None)
    T = len(fields)
    a = _snapshot_index(start, T, "start", who)
    b = T - 1 if stop is None else _snapshot_index(stop, T, "stop", who)
    if b - a + 1 < 2:
        raise ValueError("time_stats: the window start..stop = %d..%d holds fewer than 2 snapshots" % (a, b))
    if isinstance(never, bool) or not isinstance(never, (int, float, np.integer, np.floating)):
        raise TypeError("time_stats: never must be a float, got %r" % (never,))
    tw = f64(np.asarray(ts, dtype=np.float64)[a:b + 1])
    if tw.ndim != 1 or not np.all(np.isfinite(tw)) or not np.all(np.diff(tw) > 0):
        raise ValueError("time_stats: the times of the window must be finite and strictly increasing")
    lv, scalar = (None, False) if levels is None else _level_values(who, levels)
    nl = 0 if lv is None else lv.size
    if nl > 4096:
        raise ValueError("time_stats: at most 4096 levels per call, got %d" % nl)
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, who) for zk in fields[a:b + 1]]
    B, S, n = len(vecs), vecs[0][1], len(geometry.w)
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("time_stats: the snapshots have different numbers of columns")
    u = _energy_column(u, S, "u", who)

    def table_of(rows, cols):
        out = HPCMatrix.__new__(HPCMatrix)
        out.shape, out.backend = (rows, cols), backend
        out._v = HPCVector(rows * cols, backend)
        return out

    node, level = table_of(n, 8), (table_of(nl * n, 5) if nl else None)
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows = np.empty((1 + nl, 5))
    call("mgb_geo_time_stats", loc, B, table, dptr(tw), S, u, nl, dptr(lv) if nl else None, float(never), node._v.handle,
         level._v.handle if nl else None, dptr(rows))
    return TimeStats(node, level, rows, tw, None if lv is None else (lv[0].item() if scalar else lv), scalar)


# --------------------------------------------------------------------------- isosurfaces of 3-D solutions


class Isosurfaces:
    """Result of isosurfaces(): per field and level `above` = volume of {u > c}, `area` = area of {u = c}, `excess` =
    int_{u > c} (u - c), `count` = the number of triangles, `reached` = the level lies strictly inside the range of the lattice
    values.  Shapes as in LevelSets: floats for one field and a scalar level, an axis of len(ts) in front for a ParabolicSOL
    (whose `ts` is carried), an axis of len(levels) behind for an array of levels.  `rows` is the (B, nl, 5) table of the C ABI.
    `triangles(level, field)` gives the (m, 3, 3) vertices [P0, P1, P2] of the triangles of levels[level] in snapshot `field`,
    (P1 - P0) x (P2 - P0) pointing to the below side, in ascending item order; `items(level, field)` the item of each (an item
    with two triangles occurs twice) and `elements(level, field)` its element."""

    def __init__(self, levels, rows, counts, ts, squeeze, k, refine, offsets=None, tri=None, item=None):
        self.levels, self.rows, self.ts, self.k, self.refine = levels, rows, ts, k, refine
        self._counts, self._offsets, self._tri, self._item = counts, offsets, tri, item

        def shape(a):
            a = a[:, 0] if squeeze[1] else a
            a = a[0] if squeeze[0] else a
            return a if np.ndim(a) else a.item()

        self.above, self.area, self.excess = (shape(rows[:, :, j].copy()) for j in range(3))
        self.count = shape(counts.copy())
        self.reached = shape((rows[:, :, 3] > 0.0) & (rows[:, :, 4] > 0.0))

    def _row(self, level, field, who):
        B, nl = self._counts.shape
        if self._offsets is None:
            raise ValueError("Isosurfaces.%s: isosurfaces was called with triangles=False" % who)
        for v, m, name in ((level, nl, "level"), (field, B, "field")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -m <= v < m:
                raise IndexError("Isosurfaces.%s: %s = %r is not one of %d" % (who, name, v, m))
        r = (int(field) % B) * nl + int(level) % nl
        return int(self._offsets[r]), int(self._offsets[r + 1])

    def triangles(self, level=0, field=0) -> np.ndarray:
        a, b = self._row(level, field, "triangles")
        return self._tri[a:b].reshape(-1, 3, 3).copy()

    def items(self, level=0, field=0) -> np.ndarray:
        a, b = self._row(level, field, "items")
        return self._item[a:b].copy()

    def elements(self, level=0, field=0) -> np.ndarray:
        a, b = self._row(level, field, "elements")
        return self._item[a:b] // (6 * (self.k * 2 ** self.refine) ** 3)

    def __repr__(self):
        return "Isosurfaces(levels=%r, above=%r, area=%r, count=%r)" % (self.levels, self.above, self.area, self.count)


def isosurfaces(obj, levels, u=0, z=None, refine=0, triangles=True) -> Isosurfaces:
    """Where a 3-D solution takes given values: the surface {u = c} of the finite-element function as oriented triangles, its
    area, the volume of {u > c} and int_{u > c} (u - c), measured on the device (csrc/isosurface.hip; the rule is in
    include/mgb_hip.h and DESIGN.md section 4o).  `obj`, `levels`, `u` and `z` as in level_sets(); all snapshots of a
    ParabolicSOL are measured by ONE set of launches.  `refine` = 0, 1 or 2: every element of degree k is cut into
    6 (k 2^refine)^3 tetrahedra on which u is taken as linear; 0 uses the nodal values alone and gives a watertight surface,
    each further step divides the error of a smooth surface by about 4.  `triangles=False` leaves out the triangles -- one
    launch and one copy less -- for front histories.  1-D and 2-D geometries raise ValueError: level_sets() covers them."""
    geometry, fields, ts = _level_fields("isosurfaces", obj, z)
    dim = geometry.discretization["dim"]
    if dim != 3:
        raise ValueError("isosurfaces: a 3-D geometry is needed, got %d-D; level_sets() covers 1-D and 2-D" % dim)
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= refine <= 2:
        raise ValueError("isosurfaces: refine must be 0, 1 or 2, got %r" % (refine,))
    lv, scalar = _level_values("isosurfaces", levels)
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "isosurfaces") for zk in fields]
    B, S, nl = len(vecs), vecs[0][1], lv.size
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("isosurfaces: the snapshots have different numbers of columns")
    u = _energy_column(u, S, "u", "isosurfaces")
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows, counts = np.empty((B, nl, 5)), np.empty((B, nl), dtype=np.int64)
    h = C.c_void_p()
    call("mgb_geo_isosurfaces", loc, B, table, S, u, nl, dptr(lv), int(refine), dptr(rows),
         counts.ctypes.data_as(_lib.c_ll_p), C.byref(h) if triangles else None)
    offsets = tri = item = None
    if triangles:
        try:
            total = int(counts.sum())
            offsets, tri, item = np.empty(B * nl + 1, dtype=np.int64), np.empty((total, 9)), np.empty(total, dtype=np.int32)
            call("mgb_levelset_get", h, offsets.ctypes.data_as(_lib.c_ll_p), dptr(tri), iptr(item))
        finally:
            call("mgb_levelset_destroy", h)
    k = round(geometry.discretization["block"] ** (1.0 / 3.0)) - 1
    return Isosurfaces(lv[0].item() if scalar else lv, rows, counts, ts, (ts is None, scalar), k, int(refine), offsets, tri, item)


# --------------------------------------------------------------------------- flow lines of solutions


class FlowLines:
    """Result of flow_lines(): per seed `status` (one of EXIT, STALLED, MAXSTEPS, OUTSIDE, NONFINITE), `count` = the points
    recorded (the seed included), `length` = the arc length, `time` = int ds / |sigma| along the line, `start_value` and
    `end_value` = u at the seed and at the end point, `end` (dim) the end point and `end_element` its element.  Shapes (m,) and
    (m, dim) for one field; an axis of len(ts) in front for a ParabolicSOL (whose `ts` is carried).  `rows` is the (B, m, 4) table
    of the C ABI, `ds` the step that was taken.  `path(i, b)` gives the (count, dim) points of seed i in field b and
    `elements(i, b)` the element of each."""

    EXIT, STALLED, MAXSTEPS, OUTSIDE, NONFINITE = 0, 1, 2, 3, 4

    def __init__(self, rows, end, status, count, end_element, ts, ds, offsets=None, pts=None, elem=None):
        self.rows, self.ts, self.ds = rows, ts, ds
        self._offsets, self._pts, self._elem = offsets, pts, elem
        self._shape = status.shape      # (B, m)
        shape = (lambda a: a[0]) if ts is None else (lambda a: a)
        self.status, self.count, self.end_element, self.end = shape(status), shape(count), shape(end_element), shape(end)
        self.length, self.time, self.start_value, self.end_value = (shape(rows[:, :, k].copy()) for k in range(4))

    def _row(self, i, b, who):
        B, m = self._shape
        if self._offsets is None:
            raise ValueError("FlowLines.%s: flow_lines was called with paths=False" % who)
        for v, n, name in ((i, m, "seed"), (b, B, "field")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -n <= v < n:
                raise IndexError("FlowLines.%s: %s = %r is not one of %d" % (who, name, v, n))
        r = (int(b) % B) * m + int(i) % m
        return int(self._offsets[r]), int(self._offsets[r + 1])

    def path(self, i, b=0) -> np.ndarray:
        a, e = self._row(i, b, "path")
        return self._pts[a:e].copy()

    def elements(self, i, b=0) -> np.ndarray:
        a, e = self._row(i, b, "elements")
        return self._elem[a:e].copy()

    def __repr__(self):
        return "FlowLines(m=%d, ds=%r, status=%r, length=%r)" % (self._shape[1], self.ds, self.status, self.length)


def flow_lines(obj, seeds, p=2.0, u=0, z=None, direction=+1, ds=None, max_steps=1024, gmin=1e-12, paths=True,
               workgroup=None) -> FlowLines:
    """The curves that the flux sigma = |grad u|^(p-2) grad u of a solution follows, traced on the device from `seeds` (m, dim)
    by the midpoint rule in arc length (csrc/flowline.hip; the rule is in include/mgb_hip.h and DESIGN.md section 4q): where a
    particle released at a seed leaves the domain, what it passes through, the length of its path and its travel time
    int ds / |sigma|.  `obj`, `u` and `z` as in level_sets(); all snapshots of a ParabolicSOL are traced by ONE launch.  `p`: a
    finite scalar >= 1, it enters the time only.  `direction`: +1 up the gradient, -1 down.  `ds`: the step (None: a quarter of
    the smallest element extent); a line stops after `max_steps` steps, where |grad u| <= gmin, at a non-finite value, or where
    it leaves the mesh (the exit point is found by bisection).  `paths=False` leaves out the points -- no path buffer, one launch
    and one copy less.  `workgroup`: 64, 128 or 256 threads (None: the measured default); the result does not depend on it.
    2-D and 3-D geometries; a 1-D one raises ValueError."""
    geometry, fields, ts = _level_fields("flow_lines", obj, z)
    dim = geometry.discretization["dim"]
    if dim == 1:
        raise ValueError("flow_lines: a 2-D or 3-D geometry is needed, got 1-D")
    if callable(p):
        raise TypeError("flow_lines: p must be a scalar (a variable exponent is not covered)")
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise TypeError("flow_lines: p must be a scalar, got %r" % (p,))
    if not (math.isfinite(p) and p >= 1.0):
        raise ValueError("flow_lines: p must be finite and >= 1, got %r" % (p,))
    if isinstance(direction, bool) or direction not in (1, -1):
        raise ValueError("flow_lines: direction must be +1 or -1, got %r" % (direction,))
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 1:
        raise ValueError("flow_lines: max_steps must be an int >= 1, got %r" % (max_steps,))
    gmin = float(gmin)
    if not (math.isfinite(gmin) and gmin >= 0.0):
        raise ValueError("flow_lines: gmin must be finite and >= 0, got %r" % (gmin,))
    if ds is not None:
        ds = float(ds)
        if not (math.isfinite(ds) and ds > 0.0):
            raise ValueError("flow_lines: ds must be finite and > 0, got %r" % (ds,))
    if workgroup not in (None, 64, 128, 256):
        raise ValueError("flow_lines: workgroup must be 64, 128 or 256, got %r" % (workgroup,))
    pts = f64(np.asarray(_to_cpu_array(seeds)))
    if pts.ndim != 2 or pts.shape[1] != dim:
        raise ValueError("flow_lines: seeds must have shape (m, %d), got %r" % (dim, tuple(pts.shape)))
    m = pts.shape[0]
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "flow_lines") for zk in fields]
    B, S = len(vecs), vecs[0][1]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("flow_lines: the snapshots have different numbers of columns")
    if B > 65535:
        raise ValueError("flow_lines: at most 65535 fields per call")
    u = _energy_column(u, S, "u", "flow_lines")
    if B * m > 2 ** 31 - 1 or (paths and B * m * (int(max_steps) + 2) * dim > 2 ** 31 - 1):
        raise ValueError("flow_lines: the path buffer of B m (max_steps + 2) dim doubles has more than 2^31 - 1 entries")
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows, end = np.empty((B, m, 4)), np.empty((B, m, dim))
    status, count, end_element = (np.empty((B, m), dtype=np.int32) for _ in range(3))
    ds_in, ds_used = (None if ds is None else C.c_double(ds)), C.c_double(0.0)
    h = C.c_void_p()
    call("mgb_geo_flow_lines", loc, B, table, S, u, m, dptr(pts), p, int(direction),
         None if ds_in is None else C.cast(C.byref(ds_in), _lib.c_dbl_p), int(max_steps), gmin, int(workgroup or 0), dptr(rows),
         dptr(end), iptr(status), iptr(count), iptr(end_element), C.cast(C.byref(ds_used), _lib.c_dbl_p),
         C.byref(h) if paths else None)
    offsets = ppts = pelem = None
    if paths:
        try:
            total = int(count.sum())
            offsets, ppts, pelem = np.empty(B * m + 1, dtype=np.int64), np.empty((total, dim)), np.empty(total, dtype=np.int32)
            call("mgb_flowpath_get", h, offsets.ctypes.data_as(_lib.c_ll_p), dptr(ppts), iptr(pelem))
        finally:
            call("mgb_flowpath_destroy", h)
    return FlowLines(rows, end, status, count, end_element, ts, ds_used.value, offsets, ppts, pelem)


# --------------------------------------------------------------------------- path lines through parabolic runs


class PathLines:
    """Result of path_lines(): per seed `status` (one of DONE, EXIT, OUTSIDE, NONFINITE), `count` = the points recorded (the seed
    included), `rested` = the accepted steps on which the particle did not move, `end` (dim) the end point, `end_element` its
    element, `length` = the length of the path, `time` = the time at which it ended (ts[stop] for DONE), `start_value` and
    `end_value` = u at the seed at its release time and at the end, `max_step` = the longest accepted step.  `rows` is the (m, 5)
    table of the C ABI; `ts`, `release` (m,), `stop` and `substeps` are those of the call.  `path(i)` gives the (count, dim)
    points of seed i, `elements(i)` the element of each, `times(i)` the time of each (the last one `time` on EXIT) and
    `positions(j)` the (m, dim) positions of all particles at the snapshot time ts[j], NaN where a particle is not yet released or
    no longer alive: the tracer cloud, and with one seed repeated and release=arange the streakline."""

    DONE, EXIT, OUTSIDE, NONFINITE = 0, 1, 2, 3

    def __init__(self, rows, end, status, count, end_element, rested, ts, release, stop, substeps, offsets=None, pts=None,
                 elem=None):
        self.rows, self.end, self.status, self.count, self.end_element, self.rested = rows, end, status, count, end_element, rested
        self.ts, self.release, self.stop, self.substeps = ts, release, stop, substeps
        self._offsets, self._pts, self._elem = offsets, pts, elem
        self.length, self.time, self.start_value, self.end_value, self.max_step = (rows[:, k].copy() for k in range(5))

    def _row(self, i, who):
        m = len(self.status)
        if self._offsets is None:
            raise ValueError("PathLines.%s: path_lines was called with paths=False" % who)
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not -m <= i < m:
            raise IndexError("PathLines.%s: seed = %r is not one of %d" % (who, i, m))
        r = int(i) % m
        return r, int(self._offsets[r]), int(self._offsets[r + 1])

    def path(self, i) -> np.ndarray:
        _, a, e = self._row(i, "path")
        return self._pts[a:e].copy()

    def elements(self, i) -> np.ndarray:
        _, a, e = self._row(i, "elements")
        return self._elem[a:e].copy()

    def _step_time(self, rel, k):
        """the time after k accepted steps of a particle released at ts[rel]: ts[j] + i dt with k = (j - rel) substeps + i and dt
        formed as the rule forms it; ts[stop] at the end of the last slab"""
        n, ts = self.substeps, self.ts
        k = np.asarray(k, dtype=np.int64)
        j = np.minimum(rel + k // n, self.stop - 1)
        t = ts[j] + (k - (j - rel) * n) * ((ts[j + 1] - ts[j]) / n)
        return np.where(k >= (self.stop - rel) * n, ts[self.stop], t)

    def _accepted(self):
        """(m,) the accepted steps of every row (-1 for OUTSIDE): the recorded points but the seed and, on EXIT, the exit point,
        which is recorded unless the bisection ended at lo = 0; then `time` is the time of the last accepted step itself"""
        rel = self.release.astype(np.int64)
        c = self.count.astype(np.int64) - 1
        at = self._step_time(rel, np.maximum(c, 0))
        own = (self.status == self.EXIT) & ~(self.time == at)
        return np.where(own, c - 1, c)

    def times(self, i) -> np.ndarray:
        r, a, e = self._row(i, "times")
        t = self._step_time(int(self.release[r]), np.arange(e - a))
        if e - a == int(self._accepted()[r]) + 2:      # the last point is the exit point
            t[-1] = self.time[r]
        return t

    def positions(self, j) -> np.ndarray:
        B = len(self.ts)
        if self._offsets is None:
            raise ValueError("PathLines.positions: path_lines was called with paths=False")
        if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or not -B <= j < B:
            raise IndexError("PathLines.positions: snapshot = %r is not one of %d" % (j, B))
        j = int(j) % B
        m, dim = self.end.shape
        out = np.full((m, dim), np.nan)
        if j > self.stop:
            return out
        k = (j - self.release.astype(np.int64)) * self.substeps      # the accepted steps a particle needs to be there
        ok = (k >= 0) & (k <= self._accepted())
        out[ok] = self._pts[self._offsets[:-1][ok] + k[ok]]
        return out

    def __repr__(self):
        return "PathLines(m=%d, stop=%d, substeps=%d, status=%r, time=%r)" % (len(self.status), self.stop, self.substeps,
                                                                             self.status, self.time)


def path_lines(par, seeds, p=2.0, u=0, direction=-1, speed=1.0, substeps=4, release=0, stop=None, gmin=1e-12, paths=True,
               workgroup=None) -> PathLines:
    """Where particles released into a time-dependent solution go: each seed (m, dim) is released at the snapshot time
    ts[release] and carried to ts[stop] by w = speed direction |grad u|^(p-2) grad u of the field blended linearly in time
    between the snapshots of the ParabolicSOL `par`, by the midpoint rule with `substeps` steps per snapshot interval
    (csrc/pathline.hip; the rule is in include/mgb_hip.h and DESIGN.md section 4s).  The whole trajectory of every particle is
    ONE launch.  `direction=-1` (the default) follows the flux of the parabolic equation, -sigma.  `release`: an int or an (m,)
    int array in [0, stop); `stop=None` is the last snapshot.  Where |grad u| <= gmin a particle rests and goes on when the
    field moves again; it stops where it leaves the mesh (the exit point and time are found by bisection) or at a non-finite
    value.  `paths=False` leaves out the points -- no path buffer, one launch and one copy less.  `workgroup`: 64, 128 or 256
    threads (None: the measured default); the result does not depend on it.  2-D and 3-D geometries."""
    who = "path_lines"
    if not isinstance(par, ParabolicSOL):
        raise TypeError("path_lines: expected a ParabolicSOL (its snapshots are the field in time); flow_lines() follows ONE field")
    geometry, fields, ts = _level_fields(who, par, None)
    dim = geometry.discretization["dim"]
    if dim == 1:
        raise ValueError("path_lines: a 2-D or 3-D geometry is needed, got 1-D")
    if callable(p):
        raise TypeError("path_lines: p must be a scalar (a variable exponent is not covered)")
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise TypeError("path_lines: p must be a scalar, got %r" % (p,))
    if not (math.isfinite(p) and p >= 1.0):
        raise ValueError("path_lines: p must be finite and >= 1, got %r" % (p,))
    if isinstance(direction, bool) or direction not in (1, -1):
        raise ValueError("path_lines: direction must be +1 or -1, got %r" % (direction,))
    speed, gmin = float(speed), float(gmin)
    if not (math.isfinite(speed) and speed > 0.0):
        raise ValueError("path_lines: speed must be finite and > 0, got %r" % (speed,))
    if not (math.isfinite(gmin) and gmin >= 0.0):
        raise ValueError("path_lines: gmin must be finite and >= 0, got %r" % (gmin,))
    if isinstance(substeps, bool) or not isinstance(substeps, (int, np.integer)) or substeps < 1:
        raise ValueError("path_lines: substeps must be an int >= 1, got %r" % (substeps,))
    if workgroup not in (None, 64, 128, 256):
        raise ValueError("path_lines: workgroup must be 64, 128 or 256, got %r" % (workgroup,))
    ts = f64(ts)
    B = len(fields)
    if B < 2 or B > 65535:
        raise ValueError("path_lines: the ParabolicSOL must have 2..65535 snapshots, got %d" % B)
    if not np.all(np.isfinite(ts)) or not np.all(np.diff(ts) > 0):
        raise ValueError("path_lines: ts must be finite and strictly increasing")
    if stop is None:
        stop = B - 1
    if isinstance(stop, bool) or not isinstance(stop, (int, np.integer)) or not 1 <= stop <= B - 1:
        raise ValueError("path_lines: stop must be an int in [1, %d], got %r" % (B - 1, stop))
    stop = int(stop)
    pts = f64(np.asarray(_to_cpu_array(seeds)))
    if pts.ndim != 2 or pts.shape[1] != dim:
        raise ValueError("path_lines: seeds must have shape (m, %d), got %r" % (dim, tuple(pts.shape)))
    m = pts.shape[0]
    rel = np.asarray(release)
    if rel.dtype == np.bool_ or not np.issubdtype(rel.dtype, np.integer) or rel.shape not in ((), (m,)):
        raise ValueError("path_lines: release must be an int or an (m,) = (%d,) int array, got %r" % (m, release))
    rel = np.ascontiguousarray(np.broadcast_to(rel, (m,)), dtype=np.int64)
    if m and (rel.min() < 0 or rel.max() >= stop):
        raise ValueError("path_lines: every release index must lie in [0, stop) = [0, %d)" % stop)
    rel = np.ascontiguousarray(rel, dtype=np.int32)
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, who) for zk in fields]
    S = vecs[0][1]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("path_lines: the snapshots have different numbers of columns")
    u = _energy_column(u, S, "u", who)
    slots = (stop - (int(rel.min()) if m else 0)) * int(substeps) + 2
    if paths and m * slots * dim > 2 ** 31 - 1:
        raise ValueError("path_lines: the path buffer of m ((stop - min release) substeps + 2) dim doubles has more than "
                         "2^31 - 1 entries")
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows, end = np.empty((m, 5)), np.empty((m, dim))
    status, count, end_element, rested = (np.empty(m, dtype=np.int32) for _ in range(4))
    h = C.c_void_p()
    call("mgb_geo_path_lines", loc, B, table, dptr(ts), S, u, m, dptr(pts), iptr(rel), stop, int(substeps), p, int(direction), speed,
         gmin, int(workgroup or 0), dptr(rows), dptr(end), iptr(status), iptr(count), iptr(end_element), iptr(rested),
         C.byref(h) if paths else None)
    offsets = ppts = pelem = None
    if paths:
        try:
            total = int(count.sum())
            offsets, ppts, pelem = np.empty(m + 1, dtype=np.int64), np.empty((total, dim)), np.empty(total, dtype=np.int32)
            call("mgb_flowpath_get", h, offsets.ctypes.data_as(_lib.c_ll_p), dptr(ppts), iptr(pelem))
        finally:
            call("mgb_flowpath_destroy", h)
    return PathLines(rows, end, status, count, end_element, rested, ts, rel, stop, int(substeps), offsets, ppts, pelem)


# --------------------------------------------------------------------------- plane sections of solutions


class Sections:
    """Result of sections(): per field and plane `measure` = the length (2-D) or area (3-D) of the cut, `integral` = int u over
    it, `mean` = integral / measure (NaN for an empty cut), `flux` = int sigma . nu, the flow rate in the direction of n, `max`
    and `min` = the extrema of u over the quadrature points (-inf and +inf for an empty cut), `count` = the number of pieces,
    `hit` = the plane cuts something (true also where every cut item holds a non-finite value: the row is NaN, `count` 0).  Floats for one field and one plane; an axis of len(ts) in front for a ParabolicSOL
    (whose `ts` is carried), an axis of len(planes) behind for an array of planes.  `rows` is the (B, nc, 5) table of the C ABI.
    `pieces(plane, field)` gives the (m, 2, 2) segments (the side n points to on their left) or the (m, 3, 3) triangles
    ((P1 - P0) x (P2 - P0) pointing against n) of planes[plane] in snapshot `field`, in ascending item order, `values(plane,
    field)` the (m, 2) or (m, 3) values of u at their vertices, `items(plane, field)` the item of each piece (an item with two
    triangles occurs twice) and `elements(plane, field)` its element."""

    def __init__(self, planes, rows, counts, ts, squeeze, dim, offsets=None, piece=None, item=None):
        self.planes, self.rows, self.ts, self.dim = planes, rows, ts, dim
        self._counts, self._offsets, self._piece, self._item = counts, offsets, piece, item

        def shape(a):
            a = a[:, 0] if squeeze[1] else a
            a = a[0] if squeeze[0] else a
            return a if np.ndim(a) else a.item()

        self.measure, self.integral, self.flux, self.max = (shape(rows[:, :, j].copy()) for j in range(4))
        self.min = shape(-rows[:, :, 4])
        with np.errstate(invalid="ignore", divide="ignore"):
            self.mean = shape(np.where(counts > 0, rows[:, :, 1] / rows[:, :, 0], np.nan))
        self.count = shape(counts.copy())
        self.hit = shape((counts > 0) | np.isnan(rows[:, :, 0]))      # a row poisoned by a non-finite node was cut, whatever it emitted

    def _row(self, plane, field, who):
        B, nc = self._counts.shape
        if self._offsets is None:
            raise ValueError("Sections.%s: sections was called with pieces=False" % who)
        for v, m, name in ((plane, nc, "plane"), (field, B, "field")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -m <= v < m:
                raise IndexError("Sections.%s: %s = %r is not one of %d" % (who, name, v, m))
        r = (int(field) % B) * nc + int(plane) % nc
        return int(self._offsets[r]), int(self._offsets[r + 1])

    def pieces(self, plane=0, field=0) -> np.ndarray:
        a, b = self._row(plane, field, "pieces")
        d = self.dim
        return self._piece[a:b, :d * d].reshape(-1, d, d).copy()

    def values(self, plane=0, field=0) -> np.ndarray:
        a, b = self._row(plane, field, "values")
        return self._piece[a:b, self.dim * self.dim:].copy()

    def items(self, plane=0, field=0) -> np.ndarray:
        a, b = self._row(plane, field, "items")
        return self._item[a:b].copy()

    def elements(self, plane=0, field=0) -> np.ndarray:
        a, b = self._row(plane, field, "elements")
        return self._item[a:b] // (6 if self.dim == 3 else 1)

    def __repr__(self):
        return "Sections(measure=%r, integral=%r, flux=%r, count=%r)" % (self.measure, self.integral, self.flux, self.count)


def sections(obj, planes, p=2.0, u=0, z=None, pieces=True) -> Sections:
    """What a solution looks like on the cut of the domain by a plane n . x = c (a line in 2-D) and how much flows through it:
    the exact cut of every element, its measure, int u, the mean, the flow rate int sigma . nu with sigma = |grad u|^(p-2)
    grad u and nu = n / |n|, and the extrema of u, by a fixed Gauss rule that integrates the element polynomials exactly,
    on the device (csrc/section.hip; the rule is in include/mgb_hip.h and DESIGN.md section 4r).  `obj`, `u` and `z` as in
    level_sets(); all snapshots of a ParabolicSOL are cut by ONE set of launches.  `planes`: one row (n_0 .. n_{dim-1}, c) or
    an (nc, dim + 1) array of them, n finite and not zero.  `p`: ONE finite scalar >= 1 (a callable or nodal p(x) is refused).
    `pieces=False` leaves out the pieces -- one launch and one copy less -- for flow-rate histories.  A 1-D geometry raises
    ValueError: interpolate() gives the value at a point."""
    geometry, fields, ts = _level_fields("sections", obj, z)
    dim = geometry.discretization["dim"]
    if dim == 1:
        raise ValueError("sections: a 2-D or 3-D geometry is needed, got 1-D; interpolate() gives the value at a point")
    if callable(p) or isinstance(p, (HPCVector, HPCMatrix)) or np.ndim(p) != 0:
        raise TypeError("sections: p must be one scalar per call (a callable or nodal exponent p(x) is not supported)")
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise TypeError("sections: p must be one scalar per call, got %r" % (p,))
    if not (np.isfinite(p) and p >= 1.0):
        raise ValueError("sections: p must be finite and >= 1, got %r" % (p,))
    try:
        pl = np.asarray(planes.to_numpy() if hasattr(planes, "to_numpy") else planes, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("sections: planes must be one row (n, c) or an (nc, %d) array of them" % (dim + 1))
    single = pl.ndim == 1
    pl = f64(pl.reshape(1, -1) if single else pl)
    if pl.ndim != 2 or pl.shape[0] < 1 or pl.shape[1] != dim + 1:
        raise ValueError("sections: planes must be one row (n, c) or an (nc, %d) array of them, got shape %r" % (dim + 1, tuple(pl.shape)))
    if not np.all(np.isfinite(pl)) or not np.all(np.any(pl[:, :dim] != 0.0, axis=1)):
        raise ValueError("sections: every plane needs a finite normal that is not zero and a finite c")
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "sections") for zk in fields]
    B, S, nc = len(vecs), vecs[0][1], pl.shape[0]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("sections: the snapshots have different numbers of columns")
    if B > 65535 or nc > 65535:
        raise ValueError("sections: at most 65535 fields and 65535 planes per call")
    u = _energy_column(u, S, "u", "sections")
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows, counts = np.empty((B, nc, 5)), np.empty((B, nc), dtype=np.int64)
    h = C.c_void_p()
    call("mgb_geo_sections", loc, B, table, S, u, nc, dptr(pl), p, dptr(rows), counts.ctypes.data_as(_lib.c_ll_p),
         C.byref(h) if pieces else None)
    offsets = piece = item = None
    if pieces:
        try:
            total = int(counts.sum())
            offsets, piece, item = np.empty(B * nc + 1, dtype=np.int64), np.empty((total, 6 if dim == 2 else 12)), np.empty(total, dtype=np.int32)
            call("mgb_levelset_get", h, offsets.ctypes.data_as(_lib.c_ll_p), dptr(piece), iptr(item))
        finally:
            call("mgb_levelset_destroy", h)
    return Sections(pl[0].copy() if single else pl, rows, counts, ts, (ts is None, single), dim, offsets, piece, item)


# --------------------------------------------------------------------------- line integrals of solutions


class LineIntegrals:
    """Result of line_integrals(): per segment `length` = the length of the part inside the mesh, `integral` = int u ds over
    it, `mean` = integral / length (NaN where length == 0), `along` = int sigma . tdir ds, `across` = int sigma . nu ds with nu
    the left normal of the segment (the flow rate through a gate; None in 3-D), `max` and `min` = the extrema of u over the
    quadrature points and the ends of the pieces (-inf and +inf without pieces), `enter` and `leave` = the parameters t in
    [0, 1] at which the segment first enters and last leaves the mesh (NaN without pieces), `count` = the number of pieces.
    Shapes (m,) for one field; an axis of len(ts) in front for a ParabolicSOL (whose `ts` is carried).  `rows` is the (B, m, 8)
    table of the C ABI.  `pieces(i, b)` gives (elements, t0, t1, integral) of the pieces of segment i in field b, in walk
    order."""

    def __init__(self, rows, count, ts, dim, offsets=None, piece=None, elem=None):
        self.rows, self.ts, self.dim = rows, ts, dim
        self._count, self._offsets, self._piece, self._elem = count, offsets, piece, elem
        self._shape = count.shape      # (B, m)
        self._view = (lambda a: a[0]) if ts is None else (lambda a: a)
        self._set(self._shape[1:])

    def _set(self, shape):
        B = self._shape[0]
        col = lambda j: self._view(self.rows[:, :, j].reshape((B,) + tuple(shape)).copy())
        self.length, self.integral, self.along, self.across, self.max, self.min, self.enter, self.leave = (col(j) for j in range(8))
        if self.dim == 3:
            self.across = None
        with np.errstate(invalid="ignore", divide="ignore"):
            self.mean = np.where(self.length > 0, self.integral / self.length, np.nan)
        self.count = self._view(self._count.reshape((B,) + tuple(shape)).copy())

    def _row(self, i, b, who):
        B, m = self._shape
        if self._offsets is None:
            raise ValueError("LineIntegrals.%s: line_integrals was called with pieces=False" % who)
        for v, n, name in ((i, m, "segment"), (b, B, "field")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -n <= v < n:
                raise IndexError("LineIntegrals.%s: %s = %r is not one of %d" % (who, name, v, n))
        r = (int(b) % B) * m + int(i) % m
        return int(self._offsets[r]), int(self._offsets[r + 1])

    def pieces(self, i, b=0):
        a, e = self._row(i, b, "pieces")
        return self._elem[a:e].copy(), self._piece[a:e, 0].copy(), self._piece[a:e, 1].copy(), self._piece[a:e, 2].copy()

    def __repr__(self):
        return "LineIntegrals(m=%d, length=%r, integral=%r, count=%r)" % (self._shape[1], self.length, self.integral, self.count)


def line_integrals(obj, a, b, p=2.0, u=0, z=None, pieces=False, workgroup=None) -> LineIntegrals:
    """Integrals of a solution along straight segments a[i] -> b[i], (m, dim) each, on the device (csrc/ray.hip; the rule is in
    include/mgb_hip.h and DESIGN.md section 4t): the length inside the mesh, int u ds, the mean, the flow int sigma . tdir ds
    along and -- in 2-D -- int sigma . nu ds across the segment (the flow rate through a gate, nu its left normal), sigma =
    |grad u|^(p-2) grad u, the extrema of u and where the segment enters and leaves the mesh.  One lane walks one segment
    through the bin grid; every element polynomial is integrated exactly by a fixed Gauss rule.  `obj`, `u` and `z` as in
    sections(); all snapshots of a ParabolicSOL are integrated by ONE set of launches.  `p`: ONE finite scalar >= 1.
    `pieces=True` also returns the pieces per element.  `workgroup`: 64, 128 or 256 lanes (None: the default); the result does
    not depend on it.  A segment outside the mesh, with a == b or with a non-finite end gives an empty row, not an error.
    A 1-D geometry raises ValueError."""
    geometry, fields, ts = _level_fields("line_integrals", obj, z)
    dim = geometry.discretization["dim"]
    if dim == 1:
        raise ValueError("line_integrals: a 2-D or 3-D geometry is needed, got 1-D; interpolate() gives the value at a point")
    if callable(p) or isinstance(p, (HPCVector, HPCMatrix)) or np.ndim(p) != 0:
        raise TypeError("line_integrals: p must be one scalar per call (a callable or nodal exponent p(x) is not supported)")
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise TypeError("line_integrals: p must be one scalar per call, got %r" % (p,))
    if not (np.isfinite(p) and p >= 1.0):
        raise ValueError("line_integrals: p must be finite and >= 1, got %r" % (p,))
    if workgroup not in (None, 64, 128, 256):
        raise ValueError("line_integrals: workgroup must be 64, 128 or 256, got %r" % (workgroup,))
    try:
        pa, pb = (f64(np.asarray(v.to_numpy() if hasattr(v, "to_numpy") else v, dtype=np.float64)) for v in (a, b))
    except (TypeError, ValueError):
        raise TypeError("line_integrals: a and b must be (m, %d) arrays" % dim)
    if pa.ndim == 1 and pb.ndim == 1 and pa.shape == (dim,):
        pa, pb = pa.reshape(1, dim), pb.reshape(1, dim)
    if pa.ndim != 2 or pa.shape[1] != dim or pb.shape != pa.shape:
        raise ValueError("line_integrals: a and b must both have shape (m, %d), got %r and %r" % (dim, tuple(pa.shape), tuple(pb.shape)))
    m = pa.shape[0]
    loc, backend = _locator_of(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "line_integrals") for zk in fields]
    B, S = len(vecs), vecs[0][1]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("line_integrals: the snapshots have different numbers of columns")
    if B > 65535:
        raise ValueError("line_integrals: at most 65535 fields per call")
    if B * m > 2 ** 31 - 1:
        raise ValueError("line_integrals: more than 2^31 - 1 rows (fields x segments) per call")
    u = _energy_column(u, S, "u", "line_integrals")
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    rows, count = np.empty((B, m, 8)), np.empty((B, m), dtype=np.int32)
    h = C.c_void_p()
    call("mgb_geo_line_integrals", loc, B, table, S, u, m, dptr(pa), dptr(pb), p, int(workgroup or 0), dptr(rows), iptr(count),
         C.byref(h) if pieces else None)
    offsets = piece = elem = None
    if pieces:
        try:
            total = int(count.sum())
            offsets, piece, elem = np.empty(B * m + 1, dtype=np.int64), np.empty((total, 3)), np.empty(total, dtype=np.int32)
            call("mgb_levelset_get", h, offsets.ctypes.data_as(_lib.c_ll_p), dptr(piece), iptr(elem))
        finally:
            call("mgb_levelset_destroy", h)
    return LineIntegrals(rows, count, ts, dim, offsets, piece, elem)


def project(obj, axis=-1, shape=(256, 256), bounds=None, **kw):
    """A projection of a solution along a coordinate axis: parallel segments along `axis` across the bounding box (or
    `bounds` = (lower corner, upper corner)), one from every pixel centre of a grid of `shape` pixels over the other axes,
    slowest axis first as in sample_grid() -- (ny, nx) for a 3-D solution projected along z, (n,) for the marginal profiles of a
    2-D one.  Returns X (*shape, dim - 1), the pixel centres in the coordinates of the other axes, and the LineIntegrals of
    line_integrals(obj, a, b, **kw) with every result array reshaped to `shape` ((len(ts), *shape) for a ParabolicSOL): `mean`
    and `max` are the two usual projections."""
    geometry = obj if isinstance(obj, Geometry) else getattr(obj, "geometry", None)
    if not isinstance(geometry, Geometry):
        raise TypeError("project: expected an AMGBSOL, a ParabolicSOL or a Geometry")
    dim = geometry.discretization["dim"]
    if dim == 1:
        raise ValueError("project: a 2-D or 3-D geometry is needed, got 1-D")
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not -dim <= axis < dim:
        raise ValueError("project: axis must be one of the %d axes, got %r" % (dim, axis))
    axis = int(axis) % dim
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
    if len(shape) != dim - 1 or min(shape) < 1:
        raise ValueError("project: shape must give one positive pixel count per remaining axis (%d)" % (dim - 1))
    if bounds is None:
        x = np.asarray(_to_cpu_array(geometry.x)).reshape(-1, dim)
        lo, hi = x.min(axis=0), x.max(axis=0)
    else:
        lo, hi = (f64(np.asarray(v)).reshape(dim) for v in bounds)
    others = [d for d in range(dim) if d != axis]
    # pixel centres: others[0] is the fastest axis of the image, as x is in sample_grid
    centres = [lo[d] + (np.arange(shape[len(others) - 1 - j]) + 0.5) * ((hi[d] - lo[d]) / shape[len(others) - 1 - j])
               for j, d in enumerate(others)]
    mesh = np.meshgrid(*centres[::-1], indexing="ij")
    X = np.stack(mesh[::-1], axis=-1)
    flat = X.reshape(-1, dim - 1)
    a, b = np.empty((len(flat), dim)), np.empty((len(flat), dim))
    a[:, others], b[:, others] = flat, flat
    a[:, axis], b[:, axis] = lo[axis], hi[axis]
    res = line_integrals(obj, a, b, **kw)
    res._set(shape)
    return X, res


# --------------------------------------------------------------------------- boundary facets and boundary integrals


@dataclass
class Boundary:
    """The boundary facets of a geometry, in ascending (element, local facet) order (contract in include/mgb_hip.h, DESIGN.md
    section 4h): `element` (nf,) the own element of a facet, `nodes` (nf, q) its rows of x, `weights` (nf, q) the facet
    quadrature weights at those rows, `normal` (nf, dim) the outward unit normal, `measure` (nf,), `centre` (nf, dim)."""
    element: np.ndarray
    nodes: np.ndarray
    weights: np.ndarray
    normal: np.ndarray
    measure: np.ndarray
    centre: np.ndarray

    def __len__(self):
        return len(self.element)


@dataclass
class BoundaryFlux:
    """Result of boundary_flux(), by the nodal rule on the selected boundary facets: `flux` = int sigma . n ds with sigma =
    |grad u|^(p-2) grad u, `trace` = int u ds (trace / measure is the mean of the trace), `measure` = int ds, `normal_max` =
    max |sigma . n|, `tangential_max` = max |sigma - (sigma . n) n|.  Floats for one field; arrays of len(ts) for a ParabolicSOL,
    whose `ts` is carried.  `facets` (per_facet=True): int_facet sigma . n of every facet, (nf,) or (len(ts), nf)."""
    flux: object
    trace: object
    measure: object
    normal_max: object
    tangential_max: object
    ts: Optional[np.ndarray] = None
    facets: Optional[np.ndarray] = None


def boundary(geometry: Geometry) -> Boundary:
    """The boundary facets of a native or a device geometry, found on the host from subspaces["full"] at the finest level
    (csrc/boundary.hpp) and kept on the geometry."""
    if not isinstance(geometry, Geometry):
        raise TypeError("boundary: expected a Geometry")
    if geometry._boundary is not None:
        return geometry._boundary
    h, own = geometry._geo, False
    if h is None:                                                        # a native geometry: x, w and the finest full subspace
        x = f64(np.asarray(geometry.x))
        x = x.reshape(x.shape[0], -1)
        w, L = f64(geometry.w), len(geometry.refine)
        h = C.c_void_p()
        call("mgb_geo_create", x.shape[0], x.shape[1], L, int(geometry.discretization.get("block", 1)), dptr(x), dptr(w), C.byref(h))
        own = True
    try:
        if own and "full" in geometry.subspaces:
            S = sp.csr_matrix(geometry.subspaces["full"][L - 1], dtype=np.float64)
            S.sort_indices()
            S.sum_duplicates()
            rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
            call("mgb_geo_set_matrix", h, ("sub:full:%d" % (L - 1)).encode(), S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va))
        nf, q, dim = C.c_int(), C.c_int(), C.c_int()
        call("mgb_geo_boundary_dims", h, C.byref(nf), C.byref(q), C.byref(dim))
        nf, q, dim = nf.value, q.value, dim.value
        b = Boundary(np.empty(nf, dtype=np.int32), np.empty((nf, q), dtype=np.int32), np.empty((nf, q)), np.empty((nf, dim)),
                     np.empty(nf), np.empty((nf, dim)))
        call("mgb_geo_boundary_get", h, iptr(b.element), iptr(b.nodes), dptr(b.weights), dptr(b.normal), dptr(b.measure), dptr(b.centre))
    finally:
        if own:
            call("mgb_geo_destroy", h)
    geometry._boundary = b
    return b


def _boundary_selection(where, b: Boundary, who):
    """None or the (nf,) uint8 mask of `where`: a boolean (nf,) array or a callable on a facet centre."""
    if where is None:
        return None
    if callable(where):
        return np.array([1 if where(c) else 0 for c in b.centre], dtype=np.uint8).reshape(len(b))
    m = np.asarray(where)
    if m.dtype != np.bool_ or m.shape != (len(b),):
        raise ValueError("%s: where must be None, a boolean array of shape (nf,) = (%d,) or a callable on a facet centre, got %s %r"
                         % (who, len(b), m.dtype, tuple(m.shape)))
    return np.ascontiguousarray(m, dtype=np.uint8)


def boundary_flux(obj, p, u=0, z=None, where=None, per_facet=False) -> BoundaryFlux:
    """Flow rate int sigma . n ds, int u ds, measure and the largest normal and tangential flux of a solution on its boundary
    facets, sigma = |grad u|^(p-2) grad u, reduced on the device (csrc/boundary.hip; contract in include/mgb_hip.h and
    DESIGN.md section 4h).  `obj`, `p`, `u`, `z`: as for energy -- an AMGBSOL, a device Geometry with `z=`, or a ParabolicSOL,
    whose len(ts) snapshots are reduced by ONE pair of launches.  `where` selects facets: None (all of them), a boolean (nf,)
    array in the order of boundary(geometry), or a callable on a facet centre.  `per_facet=True` also returns every facet's own
    integral."""
    ts = None
    if isinstance(obj, ParabolicSOL):
        if z is not None:
            raise ValueError("boundary_flux: z= does not go with a ParabolicSOL (its snapshots are the fields)")
        geometry, fields, ts = obj.geometry, list(obj.u), np.asarray(obj.ts)
        if len(fields) != len(ts) or not fields:
            raise ValueError("boundary_flux: the ParabolicSOL has %d snapshots for %d times" % (len(fields), len(ts)))
    elif isinstance(obj, (AMGBSOL, Geometry)):
        geometry, z = _field_of(obj, "boundary_flux", z)
        fields = [z]
    else:
        raise TypeError("boundary_flux: expected an AMGBSOL, a ParabolicSOL or a Geometry")
    if geometry._geo is None:
        raise TypeError("boundary_flux: geometry must come from native_to_mpi / fem*d_mpi")
    if geometry.x.backend.world > 1:
        raise NotImplementedError("boundary_flux: sharded contexts (world > 1) are not supported")
    loc, backend = _locator_of(geometry)
    b = boundary(geometry)
    if geometry._boundary_dev is None:
        h = C.c_void_p()
        call("mgb_boundary_create", loc, geometry._geo, C.byref(h))
        geometry._boundary_dev = h
    vecs = [_nodal_values(geometry, zk, backend, "boundary_flux") for zk in fields]
    B, S = len(vecs), vecs[0][1]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("boundary_flux: the snapshots have different numbers of columns")
    u = _energy_column(u, S, "u", "boundary_flux")
    x = np.asarray(_to_cpu_array(geometry.x)).reshape(len(geometry.w), -1)
    p0, pn = _energy_exponent(p, x, "boundary_flux")
    mask = _boundary_selection(where, b, "boundary_flux")
    pv = HPCVector(pn, backend) if pn is not None else None
    table = (C.c_void_p * B)(*[v.handle.value for v, _ in vecs])
    out = np.empty((B, 5))
    facets = np.empty((B, len(b))) if per_facet else None
    call("mgb_boundary_flux", geometry._boundary_dev, B, table, S, u, p0, pv.handle if pv is not None else None, u8ptr(mask),
         dptr(facets), dptr(out))
    cols = [out[:, k].copy() for k in range(5)]
    if ts is None:
        return BoundaryFlux(*[float(c[0]) for c in cols], facets=facets[0] if per_facet else None)
    return BoundaryFlux(*cols, ts=ts, facets=facets)


# --------------------------------------------------------------------------- residual error indicators, adaptive coarse meshes


@dataclass
class InteriorFacets:
    """The interior facets of a geometry (contract in include/mgb_hip.h), in ascending (element, local
    facet) order of their first side: `elements` (nif, 2); `nodes` (nif, 2, q) the rows of the first side and those of the second
    side, node j of both on the same continuous dof; `weights` (nif, q), `normal` (nif, dim) out of the first side, `measure`
    (nif,), `centre` (nif, dim); `element_facets` (nel, nlf): the interior facet of a local facet, or -1 - f for boundary facet f."""
    elements: np.ndarray
    nodes: np.ndarray
    weights: np.ndarray
    normal: np.ndarray
    measure: np.ndarray
    centre: np.ndarray
    element_facets: np.ndarray

    def __len__(self):
        return len(self.elements)


def interior(geometry: Geometry) -> InteriorFacets:
    """The interior facets of a native or a device geometry, found on the host by the key sort of boundary() (csrc/boundary.hpp)
    and kept on the geometry."""
    if not isinstance(geometry, Geometry):
        raise TypeError("interior: expected a Geometry")
    if geometry._interior is not None:
        return geometry._interior
    h, own = geometry._geo, False
    if h is None:
        x = f64(np.asarray(geometry.x))
        x = x.reshape(x.shape[0], -1)
        w, L = f64(geometry.w), len(geometry.refine)
        h = C.c_void_p()
        call("mgb_geo_create", x.shape[0], x.shape[1], L, int(geometry.discretization.get("block", 1)), dptr(x), dptr(w), C.byref(h))
        own = True
    try:
        if own and "full" in geometry.subspaces:
            S = sp.csr_matrix(geometry.subspaces["full"][L - 1], dtype=np.float64)
            S.sort_indices()
            S.sum_duplicates()
            rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
            call("mgb_geo_set_matrix", h, ("sub:full:%d" % (L - 1)).encode(), S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va))
        nif, q, dim, nel, nlf = (C.c_int() for _ in range(5))
        call("mgb_geo_interior_dims", h, C.byref(nif), C.byref(q), C.byref(dim), C.byref(nel), C.byref(nlf))
        nif, q, dim, nel, nlf = nif.value, q.value, dim.value, nel.value, nlf.value
        I = InteriorFacets(np.empty((nif, 2), dtype=np.int32), np.empty((nif, 2, q), dtype=np.int32), np.empty((nif, q)),
                           np.empty((nif, dim)), np.empty(nif), np.empty((nif, dim)), np.empty((nel, nlf), dtype=np.int32))
        call("mgb_geo_interior_get", h, iptr(I.elements), iptr(I.nodes), dptr(I.weights), dptr(I.normal), dptr(I.measure),
             dptr(I.centre), iptr(I.element_facets))
    finally:
        if own:
            call("mgb_geo_destroy", h)
    geometry._interior = I
    return I


class ErrorIndicators:
    """Result of estimate().  `parts` (nel, 3): vol_e, jump_e, neu_e, the three numbers whose sum is
    eta_e^r; `eta` (nel,) = eta_e, its r-th root.  Both stay on the device until first used.  `volume`, `jump`, `neumann`: the sums
    of the three columns; `total` = (volume + jump + neumann)^(1/r); `eta_max` = max_e eta_e; `jump_max` = max |J_Fj| over the
    interior facet nodes; `r` the power; `columns` the five totals as the C ABI returns them (sum vol, sum jump, sum neu, max
    eta_e^r, max |J_Fj|).  A non-finite input shows as NaN in the elements it feeds and in the totals."""

    def __init__(self, geometry, parts_dev, cols, r):
        self.geometry, self.r = geometry, float(r)
        self._dev, self._parts = parts_dev, None
        self.columns = np.array(cols, dtype=np.float64)
        self.volume, self.jump, self.neumann = float(cols[0]), float(cols[1]), float(cols[2])
        self.total = float((cols[0] + cols[1] + cols[2]) ** (1.0 / self.r))
        self.eta_max = float(cols[3] ** (1.0 / self.r))
        self.jump_max = float(cols[4])

    @property
    def parts(self) -> np.ndarray:
        if self._parts is None:
            self._parts = self._dev.to_numpy().reshape(-1, 3)
            self._dev = None
        return self._parts

    @property
    def eta(self) -> np.ndarray:
        P = self.parts
        return ((P[:, 0] + P[:, 1]) + P[:, 2]) ** (1.0 / self.r)

    def coarse(self, L: Optional[int] = None) -> np.ndarray:
        """eta^r summed over the 2^(L-1) / 4^(L-1) / 8^(L-1) consecutive elements of each element of the coarse mesh (element
        c e + k is child k of e at every refinement); L defaults to the geometry's number of levels."""
        L = len(self.geometry.refine) if L is None else int(L)
        P = self.parts
        group = (2 ** self.geometry.discretization["dim"]) ** (L - 1)
        if L < 1 or len(P) % group:
            raise ValueError("ErrorIndicators.coarse: %d elements are not groups of %d" % (len(P), group))
        return ((P[:, 0] + P[:, 1]) + P[:, 2]).reshape(-1, group).sum(axis=1)

    def __repr__(self):
        return "ErrorIndicators(total=%r, volume=%r, jump=%r, neumann=%r, eta_max=%r, jump_max=%r, r=%r)" % (
            self.total, self.volume, self.jump, self.neumann, self.eta_max, self.jump_max, self.r)


def _estimate_forcing(f, x, who):
    """None or the (n,) nodal forcing of u: a scalar, an (n,) array, or what amgb takes -- a callable f(x) or an (n, K) array whose
    first entry is the cost of (u, id)."""
    n = x.shape[0]
    if f is None:
        return None
    if callable(f):
        fa = _rows(f, x)
    elif np.isscalar(f):
        return np.full(n, float(f))
    else:
        fa = f64(np.asarray(_to_cpu_array(f)))
    if fa.ndim == 2 and fa.shape[0] == n and fa.shape[1] >= 1:
        fa = fa[:, 0]
    if fa.shape != (n,):
        raise ValueError("%s: f must give one value (or one row) per node, (%d,) or (%d, K), got %r" % (who, n, n, tuple(fa.shape)))
    return np.ascontiguousarray(fa)


def estimate(obj, p, f=None, u=0, z=None, r=2.0, scale=None, dirichlet=None, neumann=None) -> ErrorIndicators:
    """Residual error indicators of a solution, per element and in total, computed on the device (csrc/estimate.hip; contract in
    include/mgb_hip.h and DESIGN.md section 4j): the element residual f - lambda div sigma of the interpolated nodal flux sigma =
    |grad u|^(p-2) grad u, the jumps of lambda sigma . n over the interior facets and the Neumann residual lambda sigma . n + h.
    `obj`: an AMGBSOL, or a device Geometry with `z=`; `p`, `u`: as for energy; `f`: None (0), a scalar, an (n,) array, or amgb's
    f(x) / (n, K) array, whose first entry is taken; `r` >= 1 the power; `scale`: lambda, None meaning lambda_i = p_i -- amgb's
    problem min int f u + s, s >= |grad u|^p -- and 1 the convention of energy().  `dirichlet`, `neumann`: as in amgb -- the
    Neumann data h act on the boundary facets NOT selected by `dirichlet` (h = 0 when only `dirichlet` is given); with neither,
    the boundary contributes nothing."""
    if isinstance(obj, ParabolicSOL):
        raise TypeError("estimate: a ParabolicSOL is not supported (the residual of a time step has a term this function does not know)")
    if not isinstance(obj, (AMGBSOL, Geometry)):
        raise TypeError("estimate: expected an AMGBSOL or a Geometry")
    if neumann is not None and dirichlet is None:
        raise ValueError("estimate: neumann= needs dirichlet= (the data act on the facets that dirichlet= does not select)")
    geometry, z = _field_of(obj, "estimate", z)
    if geometry._geo is None:
        raise TypeError("estimate: geometry must come from native_to_mpi / fem*d_mpi")
    if geometry.x.backend.world > 1:
        raise NotImplementedError("estimate: sharded contexts (world > 1) are not supported")
    if isinstance(r, (str, bytes)) or not np.isscalar(r) or not (math.isfinite(float(r)) and float(r) >= 1.0):
        raise ValueError("estimate: r must be a finite real >= 1, got %r" % (r,))
    if scale is not None and (isinstance(scale, (str, bytes)) or not np.isscalar(scale) or not math.isfinite(float(scale))):
        raise ValueError("estimate: scale must be None or a finite real, got %r" % (scale,))
    loc, backend = _locator_of(geometry)
    b = boundary(geometry)
    zv, S = _nodal_values(geometry, z, backend, "estimate")
    u = _energy_column(u, S, "u", "estimate")
    x = np.asarray(_to_cpu_array(geometry.x)).reshape(len(geometry.w), -1)
    p0, pn = _energy_exponent(p, x, "estimate")
    fa = _estimate_forcing(f, x, "estimate")
    hv = mask = None
    if dirichlet is not None:
        sel = _boundary_selection(dirichlet, b, "estimate")
        if sel is None:
            raise ValueError("estimate: dirichlet=None selects nothing")
        hv, mask, _ = _neumann_data(geometry, 0.0 if neumann is None else neumann, sel == 0, None, "estimate")
        hv = hv[0]
    if geometry._boundary_dev is None:
        hd = C.c_void_p()
        call("mgb_boundary_create", loc, geometry._geo, C.byref(hd))
        geometry._boundary_dev = hd
    nel = len(geometry.w) // geometry.discretization["block"]
    pv = HPCVector(pn, backend) if pn is not None else None
    fv = HPCVector(fa, backend) if fa is not None else None
    parts = HPCVector(3 * nel, backend)
    out = np.empty(5)
    call("mgb_estimate", geometry._boundary_dev, zv.handle, S, u, p0, pv.handle if pv is not None else None,
         fv.handle if fv is not None else None, float(r), 0 if scale is None else 1, 1.0 if scale is None else float(scale),
         dptr(hv), u8ptr(mask), parts.handle, dptr(out))
    return ErrorIndicators(geometry, parts, out, r)


def mark(values, theta=0.5) -> np.ndarray:
    """Doerfler marking on the host: the indices of the shortest prefix of `values`, in stable descending order (ties to the
    lower index), whose np.cumsum reaches theta times the total.  `theta` in (0, 1]; values must be finite and >= 0; an
    all-zero array marks nothing."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    theta = float(theta)
    if not (0.0 < theta <= 1.0):
        raise ValueError("mark: theta must lie in (0, 1], got %r" % (theta,))
    if not np.isfinite(v).all():
        raise ValueError("mark: the values must be finite")
    if (v < 0.0).any():
        raise ValueError("mark: the values must be >= 0")
    if v.size == 0:
        return np.zeros(0, dtype=np.int64)
    order = np.argsort(-v, kind="stable")
    cs = np.cumsum(v[order])
    if not cs[-1] > 0.0:
        return np.zeros(0, dtype=np.int64)
    k = int(np.argmax(cs >= theta * cs[-1]))
    return order[:k + 1].astype(np.int64)


_DEFAULT_K = np.array([[-1, -1], [1, -1], [-1, 1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64)      # fem2d's default square


def refine_triangles(K, marked) -> np.ndarray:
    """Rivara longest-edge bisection with closure of a conforming 2-D triangle list K (3m x 2, as fem2d takes it), on the host: no
    triangle of `marked` (indices into the m triangles) survives and the result is conforming.  To bisect t, look across its
    longest edge: bisect both sides when the neighbour's longest edge is that edge (or there is no neighbour), else bisect the
    neighbour first.  Equal lengths break to the lexicographically smallest sorted pair of end points, so both sides agree.
    Midpoints are (a + b) / 2, fem2d's expression; the children (a, m, c), (m, b, c) keep the parent's orientation and take its
    place; every other triangle keeps its bits and its relative order.  An empty `marked` returns K bitwise."""
    K = np.array(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[1] != 2 or K.shape[0] % 3 or K.shape[0] < 3:
        raise ValueError("refine_triangles: K must be a (3m, 2) array, got %r" % (tuple(K.shape),))
    if not np.isfinite(K).all():
        raise ValueError("refine_triangles: K must be finite")
    m = K.shape[0] // 3
    marked = np.asarray(marked).reshape(-1)
    if marked.size and not np.issubdtype(marked.dtype, np.integer):
        raise TypeError("refine_triangles: marked must hold triangle indices")
    marked = [int(t) for t in marked]
    if any(not 0 <= t < m for t in marked):
        raise ValueError("refine_triangles: marked holds an index outside [0, %d)" % m)
    if not marked:
        return K
    verts = [tuple((float(K[3 * t + i, 0]), float(K[3 * t + i, 1])) for i in range(3)) for t in range(m)]
    children = [None] * m          # per node of the refinement forest: None (a leaf) or its two children
    edges = {}                     # sorted end points -> the leaves that have this edge

    def edge_keys(v):
        return [tuple(sorted((v[i], v[(i + 1) % 3]))) for i in range(3)]

    def attach(t):
        for key in edge_keys(verts[t]):
            edges.setdefault(key, []).append(t)

    def detach(t):
        for key in edge_keys(verts[t]):
            edges[key].remove(t)

    def longest(t):
        v, best = verts[t], None
        for i, key in enumerate(edge_keys(verts[t])):
            (ax, ay), (bx, by) = key
            rank = (-((bx - ax) * (bx - ax) + (by - ay) * (by - ay)), key)
            if best is None or rank < best[0]:
                best = (rank, i, key)
        return best[1], best[2]

    def split(t, i):
        v = verts[t]
        a, b, c = v[i], v[(i + 1) % 3], v[(i + 2) % 3]
        mid = ((a[0] + b[0]) / 2, (a[1] + b[1]) / 2)
        detach(t)
        kids = []
        for tri in ((a, mid, c), (mid, b, c)):
            verts.append(tri)
            children.append(None)
            kids.append(len(verts) - 1)
            attach(kids[-1])
        children[t] = kids

    for t in range(m):
        attach(t)
    for t0 in marked:
        if children[t0] is not None:
            continue
        stack = [t0]
        while stack:
            t = stack[-1]
            if children[t] is not None:
                stack.pop()
                continue
            i, key = longest(t)
            others = [o for o in edges[key] if o != t]
            if len(others) > 1:
                raise ValueError("refine_triangles: an edge is shared by more than two triangles")
            if not others:
                split(t, i)
            else:
                o = others[0]
                io, keyo = longest(o)
                if keyo == key:
                    split(t, i)
                    split(o, io)
                else:
                    stack.append(o)
    out = []
    todo = list(range(m - 1, -1, -1))
    while todo:
        t = todo.pop()
        if children[t] is None:
            out.append(verts[t])
        else:
            todo.extend(reversed(children[t]))
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def adapt(K, L, p, steps, theta=0.5, **amgb_kwargs) -> list:
    """Solve, estimate, mark, refine the coarse mesh, solve again: `steps` refinements of the 2-D coarse mesh K (None: fem2d's
    default square), every mesh solved by amgb on fem2d_mpi(L, K) with `amgb_kwargs`.  The indicators of a solve, summed per
    coarse triangle (ErrorIndicators.coarse), feed mark(., theta), and refine_triangles gives the next K.  Returns the steps + 1
    triples (K, sol, ErrorIndicators), the last one on the finest mesh.  f, dirichlet and neumann of `amgb_kwargs` also go to
    estimate (f defaults to amgb's)."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("adapt: steps must be >= 0")
    K = _DEFAULT_K.copy() if K is None else np.array(K, dtype=np.float64)
    geo_kw = {k: amgb_kwargs[k] for k in ("Ti", "backend") if k in amgb_kwargs}
    solve_kw = {k: v for k, v in amgb_kwargs.items() if k not in geo_kw}
    est_kw = dict(f=solve_kw.get("f", DEFAULT_F[2]), dirichlet=solve_kw.get("dirichlet"), neumann=solve_kw.get("neumann"))
    out = []
    for step in range(steps + 1):
        sol = amgb(fem2d_mpi(int(L), K, **geo_kw), p=p, **solve_kw)
        ind = estimate(sol, p, **est_kw)
        out.append((K, sol, ind))
        if step < steps:
            K = refine_triangles(K, mark(ind.coarse(int(L)), theta))
    return out


# --------------------------------------------------------------------------- error indicators of parabolic runs


class StepIndicators:
    """Result of estimate_steps(), B = len(ts) - 1 steps.  `ts`, `hs` (B,) the times and the steps, `r`
    the power.  `parts` (B, nel, 4): vol_e, jump_e, neu_e -- their sum is eta_e^r of the step problem -- and tim_e; it stays on
    the device until first used.  Arrays of length B: `volume`, `jump`, `neumann`, `space` (their sum), `time` (sum of tim_e),
    `rate` (the L^r norm of the difference quotient d = (u_k - u_(k-1)) / h_k), `rate_max` (max |d_i|), `eta_max` (max_e eta_e),
    `jump_max` (max |J_Fj|), `time_max` (max_e tim_e).  `columns` (B, 2, 5): the totals as the C ABI returns them.  `sigma`: the
    (B + 1, n * dim) device HPCMatrix of the fluxes of all snapshots.  `total_space` = (sum_k h_k space_k)^(1/r), `total_time` =
    (sum_k h_k time_k)^(1/r), `total` = (sum_k h_k (space_k + time_k))^(1/r).  A non-finite input shows as NaN in the steps it
    feeds."""

    def __init__(self, geometry, ts, parts_dev, cols, sigma, r):
        self.geometry, self.r = geometry, float(r)
        self.ts = np.array(ts, dtype=np.float64)
        self.hs = np.diff(self.ts)
        self._dev, self._parts = parts_dev, None
        self.columns = np.array(cols, dtype=np.float64).reshape(len(self.hs), 2, 5)
        self.sigma = sigma
        c, q = self.columns, 1.0 / self.r
        self.volume, self.jump, self.neumann = c[:, 0, 0].copy(), c[:, 0, 1].copy(), c[:, 0, 2].copy()
        self.space = (c[:, 0, 0] + c[:, 0, 1]) + c[:, 0, 2]
        self.time = c[:, 1, 0].copy()
        self.rate, self.rate_max = c[:, 1, 1] ** q, c[:, 1, 4].copy()
        self.eta_max, self.jump_max, self.time_max = c[:, 0, 3] ** q, c[:, 0, 4].copy(), c[:, 1, 3].copy()
        self.total_space = float(np.sum(self.hs * self.space) ** q)
        self.total_time = float(np.sum(self.hs * self.time) ** q)
        self.total = float(np.sum(self.hs * (self.space + self.time)) ** q)

    @property
    def parts(self) -> np.ndarray:
        if self._parts is None:
            self._parts = self._dev.to_numpy().reshape(len(self.hs), -1, 4)
            self._dev = None
        return self._parts

    def elements(self) -> np.ndarray:
        """sum_k h_k eta_{e,k}^r, (nel,): where in space the run is inaccurate; feeds mark() and refine_triangles()."""
        P = self.parts
        return np.tensordot(self.hs, (P[:, :, 0] + P[:, :, 1]) + P[:, :, 2], axes=1)

    def coarse(self, L: Optional[int] = None) -> np.ndarray:
        """elements() summed over the consecutive elements of each element of the coarse mesh, as ErrorIndicators.coarse."""
        L = len(self.geometry.refine) if L is None else int(L)
        E = self.elements()
        group = (2 ** self.geometry.discretization["dim"]) ** (L - 1)
        if L < 1 or len(E) % group:
            raise ValueError("StepIndicators.coarse: %d elements are not groups of %d" % (len(E), group))
        return E.reshape(-1, group).sum(axis=1)

    def __repr__(self):
        return "StepIndicators(steps=%d, total=%r, total_space=%r, total_time=%r, r=%r)" % (
            len(self.hs), self.total, self.total_space, self.total_time, self.r)


def estimate_steps(par, p, f1=None, u=0, r=2.0, scale=1.0, dirichlet=None, neumann=None) -> StepIndicators:
    """Error indicators of every step of a parabolic run, from one set of launches whatever the number of steps
    (csrc/estimate.hip; contract in include/mgb_hip.h and DESIGN.md section 4m).  Step k solved an implicit-Euler problem whose
    strong form is (u_k - u_(k-1)) / h_k + f_k - div sigma_k = 0: per step the space indicator of that problem (estimate()'s
    residual with lambda = `scale` plus the difference quotient), the time indicator sum_e sum_i w_i |sigma_k - sigma_(k-1)|^r
    and the norm of the difference quotient.  `par`: a ParabolicSOL (snapshots as HPCMatrix or numpy arrays); `p`, `u`: as for
    energy; `f1`, `dirichlet`, `neumann`: as parabolic_solve takes them (f1 None is its default 0.5, pass 0.0 for no forcing;
    h(t, x) is taken at ts[1:]; values at the facet nodes, (nf, q) or (B, nf, q), are taken too), so estimate_steps(parabolic_solve(g, **kw), **kw) describes that run; `r` >= 1 the power."""
    if not isinstance(par, ParabolicSOL):
        raise TypeError("estimate_steps: par must be a ParabolicSOL")
    if neumann is not None and dirichlet is None:
        raise ValueError("estimate_steps: neumann= needs dirichlet= (the data act on the facets that dirichlet= does not select)")
    geometry, fields = par.geometry, list(par.u)
    ts = np.array(par.ts, dtype=np.float64).reshape(-1)
    if len(ts) < 2:
        raise ValueError("estimate_steps: par must hold at least two snapshots, got %d times" % len(ts))
    if len(fields) != len(ts):
        raise ValueError("estimate_steps: par.u has %d snapshots for %d times" % (len(fields), len(ts)))
    if not np.all(np.isfinite(ts)) or not np.all(np.diff(ts) > 0):
        raise ValueError("estimate_steps: par.ts must be finite and strictly increasing")
    if not isinstance(geometry, Geometry) or geometry._geo is None:
        raise TypeError("estimate_steps: the geometry of par must come from native_to_mpi / fem*d_mpi")
    if geometry.x.backend.world > 1:
        raise NotImplementedError("estimate_steps: sharded contexts (world > 1) are not supported")
    if isinstance(r, (str, bytes)) or not np.isscalar(r) or not (math.isfinite(float(r)) and float(r) >= 1.0):
        raise ValueError("estimate_steps: r must be a finite real >= 1, got %r" % (r,))
    if isinstance(scale, (str, bytes)) or not np.isscalar(scale) or not math.isfinite(float(scale)):
        raise ValueError("estimate_steps: scale must be a finite real, got %r" % (scale,))
    B = len(ts) - 1
    if B + 1 > 65535:
        raise ValueError("estimate_steps: at most 65535 snapshots per call, got %d" % (B + 1))
    loc, backend = _locator_of(geometry)
    b = boundary(geometry)
    vecs = [_nodal_values(geometry, zk, backend, "estimate_steps") for zk in fields]
    S = vecs[0][1]
    if any(Sk != S for _, Sk in vecs):
        raise ValueError("estimate_steps: the snapshots of par.u have different numbers of columns")
    u = _energy_column(u, S, "u", "estimate_steps")
    n, dim = len(geometry.w), geometry.discretization["dim"]
    x = np.asarray(_to_cpu_array(geometry.x)).reshape(n, -1)
    p0, pn = _energy_exponent(p, x, "estimate_steps")
    f1 = 0.5 if f1 is None else f1      # parabolic_solve's default, lambda x: 0.5, without a Python call per node
    if not callable(f1) and np.isscalar(f1) and not isinstance(f1, (str, bytes)):
        f1 = np.full(n, float(f1))
    try:
        f_timed, f_row = _parabolic_forcing(f1, x, ts)
    except (TypeError, ValueError) as e:
        raise type(e)(str(e).replace("parabolic_solve:", "estimate_steps: f1:", 1))
    fa = np.ascontiguousarray(np.stack([f_row(k) for k in range(B)]) if f_timed else f_row(0).reshape(1, n), dtype=np.float64)
    hv = mask = None
    if dirichlet is not None:
        sel = _boundary_selection(dirichlet, b, "estimate_steps")
        if sel is None:
            raise ValueError("estimate_steps: dirichlet=None selects nothing")
        hv, mask, _ = _neumann_data(geometry, 0.0 if neumann is None else neumann, sel == 0, ts[1:], "estimate_steps")
        if hv.shape[0] not in (1, B):
            raise ValueError("estimate_steps: neumann gives %d fields for %d steps" % (hv.shape[0], B))
    if geometry._boundary_dev is None:
        hd = C.c_void_p()
        call("mgb_boundary_create", loc, geometry._geo, C.byref(hd))
        geometry._boundary_dev = hd
    nel = n // geometry.discretization["block"]
    pv = HPCVector(pn, backend) if pn is not None else None
    fv = HPCVector(fa, backend)
    parts = HPCVector(B * nel * 4, backend)
    sigma = HPCMatrix.__new__(HPCMatrix)
    sigma.shape, sigma.backend, sigma._v = (B + 1, n * dim), backend, HPCVector((B + 1) * n * dim, backend)
    table = (C.c_void_p * (B + 1))(*[v.handle.value for v, _ in vecs])
    out = np.empty((B, 2, 5))
    call("mgb_estimate_steps", geometry._boundary_dev, B, table, dptr(ts), S, u, p0, pv.handle if pv is not None else None, fv.handle,
         fa.shape[0], float(r), float(scale), dptr(hv), 1 if hv is None else hv.shape[0], u8ptr(mask), sigma._v.handle, parts.handle,
         dptr(out))
    return StepIndicators(geometry, ts, parts, out, sigma, r)


def refine_times(ts, marked) -> np.ndarray:
    """The time twin of refine_triangles, on the host: the midpoint (ts[k] + ts[k + 1]) / 2 is inserted into every interval k of
    `marked` (indices into the len(ts) - 1 intervals); every other time keeps its bits and its order.  An empty `marked` returns
    a bitwise copy.  An index out of range, a duplicate, or a midpoint that does not fall strictly between its neighbours is a
    ValueError."""
    ts = np.array(ts, dtype=np.float64)
    if ts.ndim != 1 or ts.size < 2:
        raise ValueError("refine_times: ts must be a 1-D array with at least 2 entries")
    if not np.all(np.isfinite(ts)) or not np.all(np.diff(ts) > 0):
        raise ValueError("refine_times: ts must be finite and strictly increasing")
    marked = np.asarray(marked).reshape(-1)
    if marked.size and not np.issubdtype(marked.dtype, np.integer):
        raise TypeError("refine_times: marked must hold interval indices")
    marked = [int(k) for k in marked]
    if any(not 0 <= k < ts.size - 1 for k in marked):
        raise ValueError("refine_times: marked holds an index outside [0, %d)" % (ts.size - 1))
    if len(set(marked)) != len(marked):
        raise ValueError("refine_times: marked holds an interval twice")
    chosen, out = set(marked), []
    for k in range(ts.size - 1):
        out.append(ts[k])
        if k in chosen:
            mid = (ts[k] + ts[k + 1]) / 2
            if not ts[k] < mid < ts[k + 1]:
                raise ValueError("refine_times: the midpoint of interval %d does not fall strictly between its end points" % k)
            out.append(mid)
    out.append(ts[-1])
    return np.array(out, dtype=np.float64)


def adapt_time(geometry, ts, p, steps, theta=0.5, **kw) -> list:
    """Solve, estimate, mark, refine the times, solve again: the time twin of adapt.  Every round runs parabolic_solve(geometry,
    ts=ts, p=p, **kw) and estimate_steps on it; the time indicators h_k time_k feed mark(., theta) and refine_times gives the next
    ts.  Returns the steps + 1 triples (ts, par, StepIndicators), the last one on the finest grid.  f1, dirichlet and neumann of
    `kw` also go to estimate_steps."""
    steps = int(steps)
    if steps < 0:
        raise ValueError("adapt_time: steps must be >= 0")
    ts = np.array(ts, dtype=np.float64)
    est_kw = {k: kw[k] for k in ("f1", "dirichlet", "neumann") if k in kw}
    out = []
    for step in range(steps + 1):
        par = parabolic_solve(geometry, p=p, ts=ts, **kw)
        ind = estimate_steps(par, p, **est_kw)
        out.append((ts, par, ind))
        if step < steps:
            ts = refine_times(ts, mark(ind.hs * ind.time, theta))
    return out


# --------------------------------------------------------------------------- mixed boundary conditions


_TAKEN_SUBSPACES = ("full", "dirichlet", "fixed")


def _host_geo_with_full(geometry: Geometry):
    """A temporary host mgb_geo of a native geometry: x, w and every level of subspaces["full"] (the caller destroys it)."""
    x = f64(np.asarray(geometry.x))
    x = x.reshape(x.shape[0], -1)
    w, L = f64(geometry.w), len(geometry.refine)
    h = C.c_void_p()
    call("mgb_geo_create", x.shape[0], x.shape[1], L, int(geometry.discretization.get("block", 1)), dptr(x), dptr(w), C.byref(h))
    try:
        for l, S in enumerate(geometry.subspaces.get("full", [])[:L]):
            S = sp.csr_matrix(S, dtype=np.float64)
            S.sort_indices()
            rp, ci, va = i32(S.indptr), i32(S.indices), f64(S.data)
            call("mgb_geo_set_matrix", h, ("sub:full:%d" % l).encode(), S.shape[0], S.shape[1], iptr(rp), iptr(ci), dptr(va))
    except Exception:
        call("mgb_geo_destroy", h)
        raise
    return h


def dirichlet_on(geometry: Geometry, where, name: str = "mixed") -> str:
    """Dirichlet conditions on part of the boundary: adds geometry.subspaces[name], one matrix per level, and returns `name` for
    use in `state_variables` (amgb(dirichlet=where) does both).  A variable in that space is fixed on the rows of the selected
    boundary facets, end points included, and free everywhere else.  `where`: a boolean (nf,) array in the order of
    boundary(geometry) or a callable on a facet centre; None is refused (it would be "dirichlet"); a selection with no facet
    gives "full".  Rule (csrc/mixed.hpp): per level, the columns of subspaces["full"] without those that
    are non-zero in a selected row of the finest mesh.  Native (scipy) and device geometries."""
    if not isinstance(geometry, Geometry):
        raise TypeError("dirichlet_on: expected a Geometry")
    if where is None:
        raise ValueError('dirichlet_on: where=None would select every facet: that is the subspace "dirichlet"')
    name = str(name)
    if name in _TAKEN_SUBSPACES or name in geometry.subspaces or not name or ":" in name:
        raise ValueError("dirichlet_on: the subspace name %r is taken or not usable" % name)
    if geometry._geo is not None and geometry.x.backend.world > 1:
        raise NotImplementedError("dirichlet_on: sharded contexts (world > 1) are not supported")
    mask = _boundary_selection(where, boundary(geometry), "dirichlet_on")
    L = len(geometry.refine)
    if geometry._geo is None:
        h = _host_geo_with_full(geometry)
        try:
            call("mgb_geo_dirichlet_on", h, name.encode(), u8ptr(mask))
            mats = [_geo_matrix(h, "sub:%s:%d" % (name, l)) for l in range(L)]
        finally:
            call("mgb_geo_destroy", h)
    else:
        call("mgb_geo_dirichlet_on", geometry._geo, name.encode(), u8ptr(mask))
        backend = geometry.x.backend
        if geometry._geo_ref is not None:
            mats = [_GeoMatrix(geometry._geo_ref, "sub:%s:%d" % (name, l), backend) for l in range(L)]
        else:
            mats = [HPCSparseMatrix(_geo_matrix(geometry._geo, "sub:%s:%d" % (name, l)), backend) for l in range(L)]
    geometry.subspaces[name] = mats
    if geometry._mixed is None:
        geometry._mixed = {}
    geometry._mixed.setdefault(mask.tobytes(), name)
    return name


def _mixed_state(geometry: Geometry, state_variables, where, who):
    """(state_variables with "dirichlet" replaced by the subspace of the selection `where`, the boolean mask of the facets NOT
    selected, the first replaced variable).  The subspace is built once per geometry and selection."""
    if geometry.x.backend.world > 1:
        raise NotImplementedError("%s: dirichlet= / neumann= are not supported on sharded contexts (world > 1)" % who)
    if where is None:
        raise ValueError("%s: dirichlet=None selects nothing to replace" % who)
    mask = _boundary_selection(where, boundary(geometry), who)
    name = (geometry._mixed or {}).get(mask.tobytes())
    if name is None:
        k = 0
        while "mixed%d" % k in geometry.subspaces:
            k += 1
        name = dirichlet_on(geometry, mask.astype(np.bool_), "mixed%d" % k)
    state = tuple((v, name if sub == "dirichlet" else sub) for v, sub in state_variables)
    moved = [v for v, sub in state_variables if sub == "dirichlet"]
    if not moved:
        raise ValueError('%s: dirichlet= needs a state variable in the "dirichlet" space' % who)
    return state, mask == 0, moved[0]


@dataclass
class NeumannLoad:
    """Result of neumann_load(): `rows` (nb,) the distinct rows of the boundary facet nodes, ascending; `values` the loads on
    the device, (B, nb); `ts` the times of the B fields of an h(t, x)."""
    geometry: Geometry
    rows: np.ndarray
    values: "HPCMatrix"
    ts: Optional[np.ndarray] = None
    _host: object = field(default=None, repr=False)      # the host data the copy on the context stream reads

    def add_to(self, y: "HPCVector", k: int = 0, alpha: float = 1.0, stride: int = 1, offset: int = 0):
        """y[rows * stride + offset] += alpha * values[k], on the device."""
        call("mgb_boundary_load_add", self.geometry._boundary_dev, self.values._v.handle, int(k), float(alpha), y.handle,
             int(stride), int(offset))
        return y

    def dense(self, k: int = 0) -> "HPCVector":
        """Field k as a vector of n nodal values, zero off the boundary rows."""
        return self.add_to(HPCVector(len(self.geometry.w), self.values.backend), k)


def _neumann_data(geometry: Geometry, h, where, ts, who="neumann_load"):
    """((B, nf, q) values of h at the facet nodes, the uint8 facet mask or None, the times or None); host only."""
    b = boundary(geometry)
    nf, q = b.nodes.shape
    mask = _boundary_selection(where, b, who)
    times = None
    if callable(h):
        x = np.asarray(_to_cpu_array(geometry.x), dtype=np.float64).reshape(len(geometry.w), -1)[b.nodes]      # (nf, q, dim)
        if _positional_arity(h, "h", who) == 1:
            hv = np.array([[float(h(xi)) for xi in xf] for xf in x]).reshape(1, nf, q)
        else:
            if ts is None:
                raise ValueError("%s: h(t, x) needs ts=" % who)
            times = np.array(ts, dtype=np.float64).reshape(-1)
            if times.size < 1:
                raise ValueError("%s: ts is empty" % who)
            hv = np.array([[[float(h(t, xi)) for xi in xf] for xf in x] for t in times]).reshape(len(times), nf, q)
    elif np.isscalar(h):
        hv = np.full((1, nf, q), float(h))
    else:
        hv = f64(np.asarray(h))
        if hv.shape == (nf, q):
            hv = hv.reshape(1, nf, q)
        if hv.ndim != 3 or hv.shape[1:] != (nf, q) or hv.shape[0] < 1:
            raise ValueError("%s: an array h must have shape (nf, q) = (%d, %d) or (B, nf, q), got %r" % (who, nf, q, tuple(np.shape(h))))
    sel = np.ones(nf, dtype=bool) if mask is None else mask.astype(bool)
    if not np.isfinite(hv[:, sel]).all():
        raise ValueError("%s: h is not finite on a selected facet" % who)
    return np.ascontiguousarray(hv), mask, times


def neumann_load(geometry: Geometry, h, where=None, ts=None) -> NeumannLoad:
    """The load of Neumann data on the boundary facets of a device geometry, computed on the device (csrc/boundary.hip; contract
    in include/mgb_hip.h and DESIGN.md section 4i): l_i = (sum of omega h over the facet nodes at row i) / w_i, the addition to
    the (u, id) column of the cost that stands for int h u ds.  `h`: a scalar, a callable h(x), a callable h(t, x) with `ts=`
    (one field per time), an (nf, q) array of values at the facet nodes, or a (B, nf, q) array.  `where` selects facets as in
    boundary_flux.  All B fields come from one launch.  A non-finite h on a selected facet raises ValueError."""
    if not isinstance(geometry, Geometry):
        raise TypeError("neumann_load: expected a Geometry")
    hv, mask, times = _neumann_data(geometry, h, where, ts)
    if geometry._geo is None:
        raise TypeError("neumann_load: geometry must come from native_to_mpi / fem*d_mpi")
    if geometry.x.backend.world > 1:
        raise NotImplementedError("neumann_load: sharded contexts (world > 1) are not supported")
    loc, backend = _locator_of(geometry)
    if geometry._boundary_dev is None:
        hd = C.c_void_p()
        call("mgb_boundary_create", loc, geometry._geo, C.byref(hd))
        geometry._boundary_dev = hd
    if geometry._boundary_rows is None:
        nb = C.c_int()
        call("mgb_boundary_incidence", geometry._boundary_dev, C.byref(nb), None, None, None, None)
        rows = np.empty(nb.value, dtype=np.int32)
        call("mgb_boundary_incidence", geometry._boundary_dev, None, None, iptr(rows), None, None)
        geometry._boundary_rows = rows
    rows = geometry._boundary_rows
    B = hv.shape[0]
    vals = HPCMatrix.__new__(HPCMatrix)
    vals.shape, vals.backend, vals._v = (B, len(rows)), backend, HPCVector(B * len(rows), backend)
    call("mgb_boundary_load", geometry._boundary_dev, B, dptr(hv), u8ptr(mask), vals._v.handle)
    return NeumannLoad(geometry, rows, vals, times, (hv, mask))


def mpi_to_native(obj):
    """src:355-517: gather device objects back to native numpy/scipy types."""
    if isinstance(obj, ParabolicSOL):                                   # src:495-517
        return ParabolicSOL(mpi_to_native(obj.geometry), obj.ts, [_to_cpu_array(uk) for uk in obj.u], obj.lift)
    if isinstance(obj, Geometry):
        conv = lambda m: m.to_scipy() if isinstance(m, HPCSparseMatrix) else m
        return Geometry(dict(obj.discretization), _to_cpu_array(obj.x), _to_cpu_array(obj.w),
                        {k: [conv(m) for m in v] for k, v in obj.subspaces.items()},
                        {k: conv(m) for k, m in obj.operators.items()},
                        [conv(m) for m in obj.refine], [conv(m) for m in obj.coarsen])
    if isinstance(obj, AMGBSOL):
        return AMGBSOL(_to_cpu_array(obj.z), obj.SOL_feasibility, obj.SOL_main, obj.log, mpi_to_native(obj.geometry))
    if isinstance(obj, (HPCVector, HPCMatrix)):
        return obj.to_numpy()
    if isinstance(obj, HPCSparseMatrix):
        return obj.to_scipy()
    return obj
