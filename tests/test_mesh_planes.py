"""The hull planes of the compiled model (mesh_planeadr / mesh_planenum / mesh_plane: what a ray sees of a mesh geom) against
scipy.spatial.ConvexHull of the same kept vertices.  CPU only.

With ext the extent of a mesh's kept vertices (the diagonal of their bounding box) and the margin 1e-9 ext:
  * every kept vertex lies inside every plane within the margin (an extra plane that cuts the solid fails here);
  * every plane holds at least 3 non-collinear kept vertices within the margin (it is a facet's plane, not a vertex's or an edge's);
  * no two planes of a mesh coincide: equal normals and offsets within 1e-12 (times ext), the precision the box's planes are pinned to.
    (Planes a few 1e-8 rad apart are distinct facets, and common: the corners of a flat CAD quad are off their common plane by the
    float32 rounding of the mesh file, 1e-10 .. 1e-9 ext in armar6's and tiago's meshes; scipy reports two facets there as well.)
  * from the vertex centroid, along 2 000 Fibonacci directions, the exit distance through the planes equals the distance to scipy's
    hull triangles within the margin (a missing plane makes it longer)."""
import numpy as np
import pytest

import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr

ROBOT_FILES = rm.ROBOT_FILES
FIB = rm.fibonacci(2000)
_mesh_only_model = rm.mesh_only_model
_load_robot = rm.load_robot


def _box_planes_ok(planes):
    assert planes.shape == (6, 4)
    want = sorted((tuple(s * np.eye(3)[k]) + (rm.BOX_HALF[k],)) for k in range(3) for s in (-1.0, 1.0))
    got = sorted(tuple(np.where(np.abs(p) < 1e-12, 0.0, p)) for p in planes)
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=0, atol=1e-12)


def test_box_from_8_points_has_6_planes(lib):
    m = _mesh_only_model(lib, rm.box_points())
    assert m.c.nmesh == 1 and m.c.nmeshplane == 6 and list(m.array("mesh_planeadr")) == [0] and list(m.array("mesh_planenum")) == [6]
    _box_planes_ok(m.array("mesh_plane").reshape(-1, 4))


def test_box_from_stl_triangles_with_extra_points_has_6_planes(lib):
    vert, face = rm.box_stl_points()
    m = _mesh_only_model(lib, vert, face)
    _box_planes_ok(m.array("mesh_plane").reshape(-1, 4))
    # ... whichever of the face centres and edge midpoints the builder kept
    kept = m.array("mesh_vert").reshape(-1, 3)
    assert len(kept) >= 8


def test_tetrahedron_has_4_planes(lib):
    m = _mesh_only_model(lib, rm.tetra_points())
    assert m.c.nmeshplane == 4
    _check_mesh("tetrahedron", rm.model_mesh_verts(m)[0], rm.model_mesh_planes(m)[0])


def _check_mesh(name, vert, planes):
    ext = float(np.linalg.norm(vert.max(axis=0) - vert.min(axis=0)))
    margin = 1e-9 * ext
    assert len(planes) >= 4, name
    n, d = planes[:, :3], planes[:, 3]
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, rtol=0, atol=1e-12, err_msg=name)
    off = vert @ n.T - d      # [nvert, nplane]
    assert off.max() <= margin, (name, off.max() / ext)
    on = off >= -margin
    for k in range(len(planes)):
        s = vert[on[:, k]]
        assert len(s) >= 3, (name, k)
        # non-collinear: the supporting vertex farthest from the line through the two farthest apart is well off that line
        dd = np.linalg.norm(s[:, None] - s[None], axis=2)
        i, j = np.unravel_index(dd.argmax(), dd.shape)
        e = (s[j] - s[i]) / dd[i, j]
        h = np.linalg.norm(np.cross(s - s[i], e), axis=1).max()
        assert h > 1e-7 * ext, (name, k, h / ext)
    # no two planes coincide
    dn = np.linalg.norm(n[:, None] - n[None], axis=2); dd = np.abs(d[:, None] - d[None])
    same = (dn <= 1e-12) & (dd <= 1e-12 * ext) & ~np.eye(len(planes), dtype=bool)
    assert not same.any(), (name, np.argwhere(same)[:4])
    # exit distance from the centroid: planes against scipy's triangles
    cen = vert.mean(axis=0)
    num = d - n @ cen
    den = FIB @ n.T
    with np.errstate(divide="ignore"):
        t = np.where(den > 0, num / den, np.inf).min(axis=1)
    ref = rm.tri_ray(np.tile(cen, (len(FIB), 1)), FIB, rm.hull_triangles(vert))
    assert (ref > 0).all(), name
    assert np.abs(t - ref).max() <= margin, (name, np.abs(t - ref).max() / ext)


def test_ellipsoid_points(lib):
    m = _mesh_only_model(lib, rm.ellipsoid_points())
    vert = rm.model_mesh_verts(m)[0]
    assert len(vert) == 20, "every point on an ellipsoid is a hull vertex: all are kept"
    _check_mesh("ellipsoid points", vert, rm.model_mesh_planes(m)[0])
    assert m.c.nmeshplane == len(rm.hull_of(vert).simplices), "generic points: every facet is a triangle"


@pytest.mark.parametrize("name", sorted(ROBOT_FILES))
def test_robot_meshes(lib, name):
    m = _load_robot(lib, name)
    assert m.c.nmesh > 0 and m.c.nmeshplane > 0
    verts, planes = rm.model_mesh_verts(m), rm.model_mesh_planes(m)
    adr, num = m.array("mesh_planeadr"), m.array("mesh_planenum")
    assert adr[0] == 0 and (adr[1:] == np.cumsum(num)[:-1]).all() and num.sum() == m.c.nmeshplane
    for i in range(m.c.nmesh):
        _check_mesh(f"{name} mesh {i}", verts[i], planes[i])
    print(f"{name}: {m.c.nmesh} meshes, {m.c.nmeshplane} planes, per mesh {num.min()} .. {num.max()}")


def test_replicate_copies_the_plane_tables(lib):
    m = rr.mesh_model(lib)
    r = ms.Model(lib.mjh_model_replicate(m.ptr, 2), lib)
    assert r.c.nmeshplane == m.c.nmeshplane == 6
    for k in ("mesh_planeadr", "mesh_planenum", "mesh_plane"):
        assert np.array_equal(r.array(k), m.array(k)), k


def test_flat_mesh_has_no_planes_and_compiles(lib):
    """kept vertices that span no volume: the mesh stays invisible to rays, and compile does not fail because of it"""
    flat = np.array([[0.0, 0, 0], [0.3, 0, 0], [0.3, 0.2, 0], [0, 0.2, 0], [0.15, 0.1, 0]])
    m = _mesh_only_model(lib, flat)
    assert m.c.nmesh == 1 and m.c.nmeshplane == 0 and list(m.array("mesh_planenum")) == [0]
    assert m.array("mesh_plane").size == 0


def test_models_without_meshes_have_no_planes(lib):
    for m in (ms.scene("s24"), ms.scene("arm7", 0), ms.scene("pendulum")):
        assert m.c.nmesh == 0 and m.c.nmeshplane == 0
        assert m.array("mesh_plane").size == 0 and m.array("mesh_planeadr").size == 0
