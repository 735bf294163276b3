"""The model keeps a mesh's own triangles (mesh_triadr / mesh_trinum / mesh_tri): taken in add_mesh right after the vertices move into
the mesh's own frame and before they are de-duplicated and thinned, stored as coordinates, triangles without area dropped.  No GPU."""
import os
import re

import numpy as np

import ray_mesh_ref as rm
import ray_tri_ref as rt


def _area_volume(tris):
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    return 0.5 * np.linalg.norm(n, axis=1).sum(), np.einsum("ij,ij->i", tris[:, 0], np.cross(tris[:, 1], tris[:, 2])).sum() / 6.0


def test_box12_triangles_live_in_the_frame_of_the_hull(lib):
    m = rm.mesh_only_model(lib, *rt.box12())
    assert m.nmeshtri == 12 and list(m.array("mesh_trinum")) == [12] and list(m.array("mesh_triadr")) == [0]
    tris = rt.model_mesh_tris(m)[0]
    kept = rm.model_mesh_verts(m)[0]
    assert len(kept) == 8
    for corner in tris.reshape(-1, 3):
        assert any(np.array_equal(corner.view(np.uint64), k.view(np.uint64)) for k in np.ascontiguousarray(kept)), "every corner is bit-equal to a kept vertex"
    planes = rm.model_mesh_planes(m)[0]
    assert len(planes) == 6
    for t in tris:
        off = np.abs(t @ planes[:, :3].T - planes[:, 3])      # [3 corners, 6 planes]
        assert off.max(axis=0).min() <= 1e-12, "every triangle lies in one of the hull's planes"


def test_torus_frame_change_is_rigid(lib):
    vert, face = rt.torus()
    m = rm.mesh_only_model(lib, vert, face)
    tris = rt.model_mesh_tris(m)[0]
    assert tris.shape == (576, 3, 3) and m.nmeshtri == 576
    src = vert[face]
    (a0, v0), (a1, v1) = _area_volume(src), _area_volume(tris)
    assert abs(a1 - a0) <= 1e-12 * a0 and abs(v1 - v0) <= 1e-12 * abs(v0) and abs(v0) > 1e-3
    # pairwise corner distances: the triangles keep their order and their corners theirs
    rng = np.random.default_rng(2)
    i, j = rng.integers(576 * 3, size=(2, 4000))
    d0 = np.linalg.norm(src.reshape(-1, 3)[i] - src.reshape(-1, 3)[j], axis=1)
    d1 = np.linalg.norm(tris.reshape(-1, 3)[i] - tris.reshape(-1, 3)[j], axis=1)
    assert np.abs(d1 - d0).max() <= 1e-12
    # ... and a corner may lie outside the hull table's radius (the kept vertices are an inner approximation): never inside by much
    assert np.linalg.norm(tris.reshape(-1, 3), axis=1).max() >= np.linalg.norm(rm.model_mesh_verts(m)[0], axis=1).max() - 1e-12


def test_points_only_mesh_has_no_triangles(lib):
    m = rm.mesh_only_model(lib, rm.ellipsoid_points())
    assert m.nmeshtri == 0 and list(m.array("mesh_trinum")) == [0] and len(m.array("mesh_tri")) == 0
    assert m.c.nmeshplane > 0


def test_a_face_with_a_repeated_corner_is_dropped(lib):
    vert, face = rt.box12()
    bad = np.vstack([face[:5], [[3, 3, 6]], face[5:], [[1, 5, 1]]]).astype(np.int32)
    m = rm.mesh_only_model(lib, vert, bad)
    ref = rt.model_mesh_tris(rm.mesh_only_model(lib, vert, face))[0]
    got = rt.model_mesh_tris(m)[0]
    assert m.nmeshtri == 12 and np.array_equal(got, ref), "the degenerate faces are gone, the rest keep their order"
    # three collinear distinct corners: no area either
    v2 = np.vstack([vert, [[0.0, 0.0, 0.0]]])
    mid = 0.5 * (vert[0] + vert[1]); v2[-1] = mid
    m2 = rm.mesh_only_model(lib, v2, np.vstack([face, [[0, 8, 1]]]).astype(np.int32))
    assert m2.nmeshtri == 12


def test_flat_quad_has_triangles_but_no_hull(lib):
    m = rm.mesh_only_model(lib, *rt.flat_quad())
    assert m.nmeshtri == 2 and list(m.array("mesh_planenum")) == [0]
    a, _ = _area_volume(rt.model_mesh_tris(m)[0])
    assert abs(a - 0.4 * 0.3) <= 1e-12


def test_replicate_copies_the_triangles(lib):
    m, _, _ = rt.scene_model(lib, [("torus", (0, 0, 1.0), None, True), ("flat_quad", (1.0, 0, 1.0), None, True), ("five", (2.0, 0, 0.5), None, False)])
    r = m.replicate(3)
    assert r.nmeshtri == m.nmeshtri == 576 + 2 + 5
    for name in ("mesh_triadr", "mesh_trinum", "mesh_tri"):
        assert np.array_equal(r.array(name), m.array(name)), name
    assert list(m.array("mesh_trinum")) == [576, 2, 5] and list(m.array("mesh_triadr")) == [0, 576, 578]


def _stl_triangles(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[80:84], "<u4")[0])
    assert len(raw) == 84 + 50 * n, "binary STL"
    rec = np.frombuffer(raw[84:], np.uint8).reshape(n, 50)
    return np.ascontiguousarray(rec[:, 12:48]).view("<f4").reshape(n, 3, 3).astype(float)


def test_pr2_assets_keep_every_triangle_with_area(lib):
    from refmodels import model_dir
    m = rm.load_robot(lib, "pr2")
    xml = os.path.join(model_dir(), "test", rm.ROBOT_FILES["pr2"])
    text = open(xml).read()
    meshdir = re.search(r'meshdir="([^"]*)"', text)
    files = []
    for tag in re.findall(r"<mesh\b[^>]*>", text):
        f = re.search(r'\bfile="([^"]*)"', tag)
        s = re.search(r'\bscale="([^"]*)"', tag)
        if f:
            files.append((f.group(1), np.array([float(x) for x in s.group(1).split()]) if s else np.ones(3)))
    assert len(files) == m.c.nmesh and m.c.nmesh > 10
    num = m.array("mesh_trinum")
    want = []
    for name, scale in files:
        t = _stl_triangles(os.path.join(os.path.dirname(xml), meshdir.group(1) if meshdir else "", name)) * scale
        ext2 = float(((t.reshape(-1, 3).max(axis=0) - t.reshape(-1, 3).min(axis=0)) ** 2).sum())
        area2 = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        want.append(int((area2 > 1e-14 * ext2).sum()))
    assert list(num) == want
    assert m.nmeshtri == sum(want) and (np.array(want) > 0).all()
    assert np.array_equal(m.array("mesh_triadr"), np.concatenate([[0], np.cumsum(want)[:-1]]))
