"""The coarse 2-D meshes K (3m x 2, as fem2d(L, K) takes them) that the Cholesky, V-cycle and whole-solve tests share beyond
the default square.  A helper module, not a test module; everything here runs on the host and is deterministic.

  lshape       the L shape [-1, 1]^2 without (0, 1]^2, 6 triangles (interp_reference.LSHAPE)
  graded4 / 7  the L shape after 4 / 7 rounds of refine_triangles, each round marking every triangle with a vertex at (0, 0), the
               re-entrant corner: 30 / 48 triangles, what adapt() produces there.  The geometric nested dissection cuts between
               distinct coordinate values, so these give elimination trees quite unlike the square's
  two_squares  [-2, -1] x [0, 1] and [1, 2] x [0, 1], two triangles each: a disconnected domain, whose tree has a root with an
               empty separator and two children"""
import numpy as np

# interp_reference.LSHAPE, restated so that the child processes of the GPU tests can import this module without the oracle on
# their path (test_mesh_cases.py holds the two to one another)
LSHAPE = np.array([[-1, -1], [0, -1], [-1, 0], [0, -1], [0, 0], [-1, 0],
                   [0, -1], [1, -1], [0, 0], [1, -1], [1, 0], [0, 0],
                   [-1, 0], [0, 0], [-1, 1], [0, 0], [0, 1], [-1, 1]], dtype=np.float64)


def corner_triangles(K):
    """indices of the triangles of K with a vertex at (0, 0)"""
    T = np.asarray(K, dtype=np.float64).reshape(-1, 3, 2)
    return np.flatnonzero((np.abs(T).sum(axis=2) == 0.0).any(axis=1))


def graded(rounds):
    import mgb_amd as M
    K = LSHAPE.copy()
    for _ in range(rounds):
        K = M.refine_triangles(K, corner_triangles(K))
    return K


def _square(x0):
    return [[x0, 0], [x0 + 1, 0], [x0, 1], [x0 + 1, 0], [x0 + 1, 1], [x0, 1]]


_BUILD = {"square": lambda: None, "lshape": lambda: LSHAPE.copy(), "graded4": lambda: graded(4), "graded7": lambda: graded(7),
          "two_squares": lambda: np.array(_square(-2) + _square(1), dtype=np.float64)}


class _Meshes(dict):
    """name -> K, built on first use (the graded meshes need the library, which a helper does not import at collection) and
    kept, read-only"""

    def __missing__(self, name):
        self[name] = K = _BUILD[name]()
        if K is not None:
            K.setflags(write=False)
        return K


NAMES = tuple(_BUILD)
MESHES = _Meshes()
TRIANGLES = {"lshape": 6, "graded4": 30, "graded7": 48, "two_squares": 4}
# sizes of the levels 0 .. L - 1 of the default problem (u on the Dirichlet subspace, s on the full one) on fem2d(L, K)
LEVEL_SIZES = {("graded4", 3): [182, 722, 2882], ("graded7", 2): [290, 1154], ("lshape", 3): [38, 146, 578]}


def mesh(name):
    """K of a mesh name; None (and "square") give None, fem2d's default square"""
    return None if name is None else MESHES[name]
