"""The mesh ray reference pins itself, as test_ray_ref.py does for the primitives: on the shared test meshes the triangle intersection
of ray_mesh_ref (scipy's hull triangles, two-sided, nearest x >= 0) agrees with an independent method — marching the point-membership
test (all hull inequalities <= 0) along the ray and bisecting the first change.  CPU only, numpy / scipy only."""
import numpy as np
import pytest

import ray_mesh_ref as rm
import ray_ref as rr

MESHES = {"box": rm.box_points, "tetrahedron": rm.tetra_points, "ellipsoid points": rm.ellipsoid_points}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_triangles_agree_with_marching(name):
    vert = MESHES[name]()
    h = rm.hull_of(vert)
    tris = h.points[h.simplices]
    n = 0
    for k, fam in enumerate(("random", "inside", "face normal", "through edge", "through vertex")):
        P, V = rm.mesh_rays(vert, fam, 3.0, 40, seed=100 + k)
        got = rm.tri_ray(P, V, tris)
        want = rm.march(P, V, h.equations, length=5.0)
        hit = want >= 0
        # (a ray that only clips the hull over less than one marching step is a miss for the march: compare where both agree on hit / miss
        #  or the chord is long enough to be seen)
        assert ((got >= 0) == hit).mean() >= 0.95, fam
        both = hit & (got >= 0)
        assert both.sum() >= 20, fam
        scale = np.linalg.norm(V, axis=1)
        assert (np.abs(got - want)[both] * scale[both]).max() <= 1e-8, (fam, (np.abs(got - want)[both] * scale[both]).max())
        n += int(both.sum())
    assert n >= 150


def test_an_origin_inside_hits_the_far_surface():
    vert = rm.box_points()
    tris = rm.hull_triangles(vert)
    x = rm.tri_ray([[0.05, 0.02, -0.03]], [[0, 0, 2.0]], tris)
    assert x[0] == pytest.approx((0.1 + 0.03) / 2.0, abs=1e-14)
    x = rm.tri_ray([[0.0, 0.0, 1.0]], [[0, 0, -0.5]], tris)
    assert x[0] == pytest.approx(0.9 / 0.5, abs=1e-14)
    assert rm.tri_ray([[0.0, 0.0, 1.0]], [[0, 0, 1.0]], tris)[0] == -1.0
    assert rm.tri_ray([[0.5, 0.0, 1.0]], [[0, 0, -1.0]], tris)[0] == -1.0


def test_cast_merges_meshes_and_primitives_by_the_smaller_distance():
    """a ball inside the box mesh's shadow: from above the mesh is nearer, from below the ball; invisible meshes drop out"""
    tris = rm.hull_triangles(rm.box_points())
    scene = dict(pos=np.array([[0, 0, 1.0], [0, 0, 0.4]]), mat=np.tile(np.eye(3).ravel(), (2, 1)), size=np.array([[0, 0, 0], [0.2, 0, 0]], float),
                 type=np.array([rr.MESH, rr.SPHERE]), visible=np.ones(2, bool), hfield={}, mesh={0: tris})
    P = np.array([[0, 0, 2.0], [0, 0, -1.0], [0, 0, 2.0]]); V = np.array([[0, 0, -1.0], [0, 0, 1.0], [0, 0, 1.0]])
    d, g = rm.cast(P, V, scene)
    assert list(g) == [0, 1, -1] and d[0] == pytest.approx(0.9) and d[1] == pytest.approx(1.2) and d[2] == -1.0
    d, g = rm.cast(P, V, dict(scene, visible=np.array([False, True])))
    assert list(g) == [1, 1, -1] and d[0] == pytest.approx(1.4)
    d, g = rm.cast(P, V, scene, cutoff=1.0)
    assert list(g) == [0, -1, -1]
    assert rm.robust((P, V), scene).all()
    # a ray along the box's edge is not robust
    assert not rm.robust((np.array([[0.2, 0.15, 2.0]]), np.array([[0, 0, -1.0]])), scene)[0]
