"""CPU checks of tests/interp_reference.py itself (the yardstick of the interpolation tests): it reproduces functions of the
element space and their gradients, it agrees with the project's own prolongation `refine` on every fine node, it finds the
parent element of a fine centroid exactly, and the notch of the L-shape is outside."""
import numpy as np
import pytest

import interp_reference as IR
import mgb_oracle as O


def _geo(kind, L, extra=None):
    if kind == "fem1d":
        return O.fem1d(L)
    if kind == "fem2d":
        return O.fem2d(L, extra)
    return O.fem3d(L, extra)


def _interior(g, block, m, rng):
    x = g.x.reshape(g.x.shape[0], -1)
    dim = x.shape[1]
    e = rng.integers(0, x.shape[0] // block, size=m)
    r = IR._ref_points(dim, m, rng, margin=1e-3)
    pts = np.empty((m, dim))
    for q in range(m):
        x0, J = IR._element_map(dim, block, x[e[q] * block:(e[q] + 1) * block])
        pts[q] = x0 + J @ r[q]
    return pts, e, r


def test_reproduces_quadratic_plus_bubble_2d():
    g = O.fem2d(2, IR.LSHAPE)
    rng = np.random.default_rng(1)
    nel = g.x.shape[0] // 7
    c = rng.standard_normal(nel)                               # bubble coefficient per element
    A = rng.standard_normal((2, 2)); A = A + A.T; b = rng.standard_normal(2)
    quad = lambda p: 0.3 + p @ b + 0.5 * np.einsum("pi,ij,pj->p", p, A, p)
    z = quad(g.x)
    z[6::7] += c / 27.0                                        # lambda1 lambda2 lambda3 = 1/27 at the centroid, 0 at the other nodes
    pts, e, r = _interior(g, 7, 200, rng)
    vals, grads, elem = IR.interpolate(g.x, 7, z, pts)
    lam = np.stack([1 - r[:, 0] - r[:, 1], r[:, 0], r[:, 1]], axis=1)
    want = quad(pts) + c[e] * lam.prod(axis=1)
    gl = np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]])      # reference gradients of the barycentrics
    gb_ref = sum(gl[i] * (lam[:, (i + 1) % 3] * lam[:, (i + 2) % 3])[:, None] for i in range(3))
    gwant = b + pts @ A
    for q in range(pts.shape[0]):
        _, J = IR._element_map(2, 7, g.x[e[q] * 7:(e[q] + 1) * 7])
        gwant[q] += c[e[q]] * np.linalg.solve(J.T, gb_ref[q])
    assert np.array_equal(elem, e)
    vtol, gtol = IR.tolerances(g.x, 7, z)
    assert np.abs(vals[:, 0] - want).max() < vtol
    assert np.abs(grads[:, 0] - gwant).max() < gtol


@pytest.mark.parametrize("k", [1, 2, 3])
def test_reproduces_tensor_monomial_3d(k):
    g = O.fem3d(2, k)
    rng = np.random.default_rng(2)
    f = lambda p: p[:, 0] ** k * p[:, 1] ** (k - 1) * p[:, 2]
    pts, e, _ = _interior(g, (k + 1) ** 3, 100, rng)
    vals, grads, elem = IR.interpolate(g.x, (k + 1) ** 3, f(g.x), pts)
    x, y, zc = pts.T
    gwant = np.stack([k * x ** (k - 1) * y ** (k - 1) * zc,
                      (k - 1) * x ** k * y ** max(k - 2, 0) * zc, x ** k * y ** (k - 1)], axis=1)
    assert np.array_equal(elem, e)
    vtol, gtol = IR.tolerances(g.x, (k + 1) ** 3, f(g.x))
    assert np.abs(vals[:, 0] - f(pts)).max() < vtol
    assert np.abs(grads[:, 0] - gwant).max() < gtol


def test_reproduces_affine_1d():
    g = O.fem1d(3)
    rng = np.random.default_rng(3)
    pts, e, _ = _interior(g, 2, 50, rng)
    vals, grads, elem = IR.interpolate(g.x, 2, 2.0 - 3.0 * g.x[:, 0], pts)
    assert np.array_equal(elem, e)
    vtol, gtol = IR.tolerances(g.x, 2, 2.0 - 3.0 * g.x[:, 0])
    assert np.abs(vals[:, 0] - (2.0 - 3.0 * pts[:, 0])).max() < vtol and np.abs(grads[:, 0, 0] + 3.0).max() < gtol


@pytest.mark.parametrize("kind,L,extra,block", [("fem2d", 3, None, 7), ("fem2d", 3, IR.LSHAPE, 7), ("fem1d", 4, None, 2),
                                                ("fem3d", 2, 2, 27)])
def test_agrees_with_refine_on_every_fine_node(kind, L, extra, block):
    """z in the continuous coarse space: interpolate(g_{L-1}, z, g_L.x) == g_L.refine[L-2] @ z on every row (coincident fine
    nodes of neighbouring coarse elements see the same value, so ties do not matter)."""
    gc, gf = _geo(kind, L - 1, extra), _geo(kind, L, extra)
    rng = np.random.default_rng(4)
    R = gc.subspaces["full"][-1]
    z = R @ rng.standard_normal((R.shape[1], 2))
    vals, _, elem = IR.interpolate(gc.x, block, z, gf.x)
    want = gf.refine[L - 2] @ z
    assert (elem >= 0).all()
    assert np.abs(vals - want).max() < IR.tolerances(gc.x, block, z)[0]


@pytest.mark.parametrize("extra", [None, IR.LSHAPE])
def test_broken_field_at_fine_centroids(extra):
    """A broken (discontinuous) z: fine centroids (rows 7e + 6) are strictly inside their parent e // 4."""
    L = 3
    gc, gf = O.fem2d(L - 1, extra), O.fem2d(L, extra)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((gc.x.shape[0], 3))
    rows = np.arange(6, gf.x.shape[0], 7)
    vals, _, elem = IR.interpolate(gc.x, 7, z, gf.x[rows])
    want = (gf.refine[L - 2] @ z)[rows]
    assert np.array_equal(elem, (rows // 7) // 4)
    assert np.abs(vals - want).max() < IR.tolerances(gc.x, 7, z)[0]


def test_notch_of_the_lshape_is_outside():
    g = O.fem2d(3, IR.LSHAPE)
    assert g.x.shape[0] == 96 * 7
    vals, grads, elem = IR.interpolate(g.x, 7, np.ones((g.x.shape[0], 2)), np.array([[0.5, 0.5], [-0.5, 0.5], [np.nan, 0.0]]))
    assert elem.tolist()[0] == -1 and elem[1] >= 0 and elem[2] == -1
    assert np.isnan(vals[0]).all() and np.isnan(grads[0]).all() and np.isnan(vals[2]).all()
    assert np.abs(vals[1] - 1.0).max() < 1e-14
