"""The float64 reference of TSDF fusion and marching tetrahedra (tests/tsdf_reference.py) held to ground truth: analytic fields whose
surface is known.  CPU only; nothing of the product is imported."""
import numpy as np
import pytest

from tests import tsdf_reference as R

CENTRE, RADIUS = np.array([6.1, 5.9, 6.2]), 3.7


@pytest.fixture(scope="module")
def sphere_mesh():
    t, w = R.analytic_sphere_grid(12, CENTRE, RADIUS)
    return R.extract(t, w, None, (0.0, 0.0, 0.0), 1.0)


def test_sphere_mesh_is_closed_and_outward(sphere_mesh):
    m = sphere_mesh
    V, E, F = R.assert_closed(m["faces"])
    assert (V, E, F) == (780, 2334, 1556), "the figures of a prototype of the same specification"
    assert V == m["vertices"].shape[0], "everything valid: no vertex without a triangle"
    n, c = R.triangle_normals(m["vertices"], m["faces"])
    assert (np.einsum("ij,ij->i", n, c - CENTRE) > 0).all(), "every triangle normal points outward"
    dist = np.abs(np.linalg.norm(m["vertices"] - CENTRE, axis=1) - RADIUS)
    assert dist.max() <= 0.15, dist.max()
    ratio = R.enclosed_volume(m["vertices"], m["faces"]) / (4.0 / 3.0 * np.pi * RADIUS ** 3)
    assert abs(ratio - 1.0) <= 0.05, ratio
    # the vertex normals are the field's gradient: radial on a distance field
    radial = (m["vertices"] - CENTRE) / np.linalg.norm(m["vertices"] - CENTRE, axis=1)[:, None]
    assert np.einsum("ij,ij->i", m["normals"], radial).min() > 0.99
    # vertices come ordered by (owner, type)
    key = m["owner"] * 7 + m["type"]
    assert (np.diff(key) > 0).all()


def test_sphere_with_an_invalid_corner_block_opens_a_boundary():
    t, w = R.analytic_sphere_grid(12, CENTRE, RADIUS)
    w[:4, :4, :4] = 0.0
    m = R.extract(t, w, None, (0.0, 0.0, 0.0), 1.0)
    _, cu = R.edge_stats(m["faces"])
    assert (cu == 1).any(), "boundary edges appear"
    assert cu.max() <= 2, "no edge is used more than twice"
    used = np.unique(m["faces"])
    assert used.size <= m["vertices"].shape[0]
    # nothing stands inside the invalid block: a vertex needs two valid ends
    k, j, i = np.unravel_index(m["owner"], t.shape)
    assert not ((k < 4) & (j < 4) & (i < 4)).any()


def test_exact_zeros_count_as_outside_and_give_vertices_at_the_corner():
    t = np.ones((3, 3, 3))
    t[1, 1, 1] = -1.0
    t[1, 1, 2] = 0.0   # (i = 2, j = 1, k = 1): a zero next to the inside voxel
    m = R.extract(t, np.ones_like(t), None, (0.0, 0.0, 0.0), 1.0)
    R.assert_closed(m["faces"])
    on = np.isclose(m["vertices"], [2.5, 1.5, 1.5]).all(1)
    assert on.sum() == 1, "the edge from the inside voxel to the zero ends exactly on the zero's centre"


def test_integrated_sphere_lies_on_the_sphere():
    sc = R.sphere_scene()
    T, W, _, unstable = R.reference_of(sc)
    assert unstable.mean() <= 0.05, unstable.mean()
    m = R.extract(T, W, None, sc["origin"], np.float32(sc["voxel"]))
    assert m["faces"].shape[0] > 0
    err = np.abs(np.linalg.norm(m["vertices"] - np.array(sc["centre"]), axis=1) - sc["radius"]) / sc["voxel"]
    print(f"radial error of {err.size} vertices: median {np.median(err):.3f}, 90th percentile {np.percentile(err, 90):.3f} voxel; "
          f"unstable share {unstable.mean():.4f}")
    assert np.median(err) <= 0.25 and np.percentile(err, 90) <= 0.75
    # batch == one by one, in float64 too: the call continues from what the grid holds
    t, w, c = R.fresh(sc["dims"], False)
    for v in range(6):
        t, w, c, _ = R.integrate(t, w, c, sc["dims"], sc["origin"], np.float32(sc["voxel"]), sc["depth"][v:v + 1], sc["viewmatrix"][v:v + 1],
                                 sc["tanfovx"][v:v + 1], sc["tanfovy"][v:v + 1], None, None, np.float32(sc["trunc"]), np.float32(sc["near"]))
    assert np.array_equal(t, T) and np.array_equal(w, W)


def test_plane_scene_exercises_what_it_claims():
    """The second integration scene: poisoned pixels, a camera inside the grid and a narrow view, at an unstable share below 5 % on every grid
    the GPU tests use."""
    for dims in ((1, 1, 1), (63, 1, 1), (65, 3, 2), (28, 26, 24), (130, 5, 3)):
        for scene in (R.sphere_scene(dims), R.plane_scene(dims)):
            _, _, _, unstable = R.reference_of(scene)
            assert unstable.mean() <= 0.05, (dims, unstable.mean())
    sc = R.plane_scene()
    for name in ("depth", "weight_img"):
        a = sc[name]
        assert (a == 0).any() and (a < 0).any() and np.isnan(a).any() and np.isinf(a).any(), name
    X, Y, Z = R.centres(sc["dims"], sc["origin"], np.float32(sc["voxel"]))
    m = sc["viewmatrix"][2].astype(np.float64)
    zc = m[2] * X + m[6] * Y + m[10] * Z + m[14]
    assert (zc < 0).any() and (zc > sc["near"]).any(), "the third camera stands inside the grid: voxels behind it exist"
    T, W, C, _ = R.reference_of(sc)
    one = R.integrate(*R.fresh(sc["dims"], True), sc["dims"], sc["origin"], np.float32(sc["voxel"]), sc["depth"][3:], sc["viewmatrix"][3:],
                      sc["tanfovx"][3:], sc["tanfovy"][3:], sc["colour_img"][3:], sc["weight_img"][3:], np.float32(sc["trunc"]), np.float32(sc["near"]))
    share = (one[1] > 0).mean()
    assert 0.0 < share < 0.5, f"the narrow view sees part of the grid only ({share:.3f})"
    assert np.isfinite(T).all() and np.isfinite(W).all() and np.isfinite(C).all()
    assert T.min() >= -1.0 and T.max() <= 1.0
