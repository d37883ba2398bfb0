"""Host-only checks of tests/mesh_cases.py, the coarse meshes shared by the Cholesky, V-cycle and whole-solve tests: the triangle
counts, conformity and orientation of each mesh, the sizes of the levels the cases were chosen for, and that the library and the
oracle build the same nodes on them (the oracle is the reference of every solve on these meshes)."""
import numpy as np
import pytest

import estimate_reference as XR
import interp_reference as IR
import mesh_cases as MC
import mgb_oracle as O

NAMES = [n for n in MC.NAMES if n != "square"]


def test_the_table_names_the_meshes():
    assert MC.NAMES == ("square", "lshape", "graded4", "graded7", "two_squares") and set(MC.TRIANGLES) == set(NAMES)
    assert MC.LSHAPE.tobytes() == IR.LSHAPE.tobytes() and MC.MESHES["lshape"].tobytes() == IR.LSHAPE.tobytes()
    assert MC.MESHES["square"] is None and MC.mesh(None) is None and MC.mesh("lshape") is MC.MESHES["lshape"]
    K = MC.MESHES["graded4"]
    assert K is MC.MESHES["graded4"] and not K.flags.writeable      # built once, shared, left unchanged
    assert K.tobytes() == MC.graded(4).tobytes()                    # deterministic


@pytest.mark.parametrize("name", NAMES)
def test_triangles_conformity_orientation(name):
    K = MC.MESHES[name]
    assert K.dtype == np.float64 and K.shape == (3 * MC.TRIANGLES[name], 2)
    XR.check_conforming(K)
    twice = XR.orientation(K)
    assert (twice > 0).all()
    assert abs(0.5 * twice.sum() - (2.0 if name == "two_squares" else 3.0)) <= 1e-12      # the area of the domain
    if name.startswith("graded"):      # graded towards the re-entrant corner: a smallest triangle touches (0, 0)
        area = np.abs(twice)
        smallest = XR.triangles(K)[area <= area.min() * (1 + 1e-12)]
        assert any((np.abs(t).sum(axis=1) == 0.0).any() for t in smallest)
        assert area.min() < area.max()
    if name == "two_squares":          # two components: no vertex is shared between the squares
        T = XR.triangles(K)
        assert (T[:2, :, 0] <= -1).all() and (T[2:, :, 0] >= 1).all()


@pytest.mark.parametrize("name,L", sorted(MC.LEVEL_SIZES))
def test_level_sizes_of_the_oracle(name, L):
    Mo = O.amg(O.fem2d(L, MC.MESHES[name]))
    assert [R.shape[1] for R in Mo.R] == MC.LEVEL_SIZES[(name, L)]


@pytest.mark.parametrize("name,L", [("lshape", 3), ("graded4", 2), ("graded7", 2), ("two_squares", 3)])
def test_library_and_oracle_build_the_same_nodes(name, L):
    import mgb_amd as M
    K = MC.MESHES[name]
    g, go = M.fem2d(L, K), O.fem2d(L, K)
    x = np.asarray(g.x).reshape(np.asarray(g.x).shape[0], -1)
    assert x.shape == go.x.shape == (7 * MC.TRIANGLES[name] * 4 ** (L - 1), 2)
    assert np.array_equal(x, go.x)
    assert np.allclose(np.asarray(g.w), go.w, rtol=1e-14, atol=0)
