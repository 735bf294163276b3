"""The fp64 ray reference (ray_ref.py) pinned on the CPU: its closed forms against marching the point-membership test (no formula
shared), the share of non-robust rays in every generated ray set the GPU tests use, and the ray symbols of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
import ray_ref as rr
from helpers import D
from mujoco_sim_amd import capi

HF = (rr.HF_NROW, rr.HF_NCOL, np.array(rr.HF_SIZE), rr.HF_ELEV)
SOLIDS = [(rr.PLANE, (0.0, 0.0, 0.05), None)] + [(t, s, None) for t, s in rr.PRIMITIVES] + [(rr.HFIELD, (0.0, 0.0, 0.0), HF)]
NAMES = {rr.PLANE: "plane", rr.SPHERE: "sphere", rr.CAPSULE: "capsule", rr.ELLIPSOID: "ellipsoid", rr.CYLINDER: "cylinder", rr.BOX: "box",
         rr.HFIELD: "hfield"}


def _one_geom_scene(t, s, hf):
    return dict(pos=np.zeros((1, 3)), mat=np.eye(3).reshape(1, 9), size=np.array([s], float), type=np.array([t]), visible=np.ones(1, bool),
                hfield={0: hf} if hf is not None else {})


def _frame_rays(t, s, hf, seed, n=80):
    """rays in the geom's own frame: origins outside, aimed at points near the geom, and a share of origins inside it"""
    rng = np.random.default_rng(seed)
    scene = _one_geom_scene(t, s, hf)
    lo, hi = ((-2.0, -2.0, 0.05), (2.0, 2.0, 2.0)) if t == rr.PLANE else ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))
    P, V = rr.make_rays(seed, scene, n, lo, hi)
    if t != rr.PLANE:      # origins inside the solid, any direction
        k = n // 4
        X = np.zeros((0, 3))
        ext = np.array([1.0, 0.6, 0.4]) if t == rr.HFIELD else np.full(3, rr.rbound(t, s))
        while len(X) < k:
            Y = rng.uniform(-ext, ext, size=(8 * k, 3))
            X = np.vstack([X, Y[rr.inside(t, Y, s, hf)]])
        P[:k] = X[:k]
        V[:k] = rng.normal(size=(k, 3))
    return P, V, scene


@pytest.mark.parametrize("t,s,hf", SOLIDS, ids=[NAMES[t] for t, _, _ in SOLIDS])
def test_closed_form_agrees_with_march(t, s, hf):
    P, V, scene = _frame_rays(t, s, hf, seed=100 + t)
    ref = rr.geom_ray(t, P, V, s, hf)
    rob = rr.robust((P, V), scene)
    got = rr.march(t, P, V, s, hf)
    assert rob.mean() >= 0.9
    hit = ref >= 0
    assert hit[rob].sum() >= 20 and (~hit[rob]).sum() >= 5, "the set must exercise hits and misses"
    assert ((got >= 0) == hit)[rob].all(), "misses agree"
    both = rob & hit
    assert np.abs(got - ref)[both].max() <= 1e-6


def test_plane_faces_and_bounds():
    s = (0.8, 0.5, 0.05)
    x = rr.geom_ray(rr.PLANE, [[0, 0, 1.0], [0, 0, -1.0], [0.9, 0, 1.0], [0, 0.6, 1.0], [0.79, 0.49, 2.0]],
                    [[0, 0, -1.0], [0, 0, 1.0], [0, 0, -1.0], [0, 0, -2.0], [0, 0, -4.0]], s)
    assert x.tolist() == [1.0, -1.0, -1.0, -1.0, 0.5]      # front hit; back face; beyond either edge; units of |vec|


def test_origin_inside_hits_the_far_surface():
    assert rr.geom_ray(rr.SPHERE, [[0.1, 0, 0]], [[1.0, 0, 0]], (0.22, 0, 0))[0] == pytest.approx(0.12)
    assert rr.geom_ray(rr.BOX, [[0.05, 0, 0]], [[0, -1.0, 0]], (0.25, 0.15, 0.2))[0] == pytest.approx(0.15)


def test_hfield_row_column_order():
    """height over grid point (r, c) is data[r, c]: x runs along the columns, y along the rows"""
    sx, sy, sz, _ = rr.HF_SIZE
    for r in range(rr.HF_NROW):
        for c in range(rr.HF_NCOL):
            x, y = -sx + 2 * sx * c / (rr.HF_NCOL - 1), -sy + 2 * sy * r / (rr.HF_NROW - 1)
            assert rr.hfield_height(HF, np.array([x]), np.array([y]))[0] == pytest.approx(rr.HF_ELEV[r, c] * sz)
    # straight down onto an interior grid point
    d = rr.geom_ray(rr.HFIELD, [[-0.5, 0.0, 2.0]], [[0, 0, -1.0]], (0, 0, 0), HF)[0]
    assert d == pytest.approx(2.0 - rr.HF_ELEV[1, 1] * sz)


def test_hfield_rays_on_grid_lines_agree_with_march():
    """the edge slack of the triangle test: rays that lie in the plane of a grid line, pass through nodes along a diagonal, or come
    straight down at nodes of a 9 x 9 field hit what marching the membership test finds — no ray falls between two triangles"""
    e = rr.rolling(9, 9, 77)
    hf = (9, 9, np.array([1.0, 0.8, 0.5, 0.2]), e)
    P, V, rc = rr.hfield_node_rays(hf)
    sets = [("nodes", (P, V)), ("row planes", rr.hfield_line_rays(hf, 1, 78, 60)), ("column planes", rr.hfield_line_rays(hf, 0, 79, 60)),
            ("diagonals", rr.hfield_diagonal_rays(hf, 80, 60))]
    scene = rr.terrain_scene(hf)
    for name, (P, V) in sets:
        ref = rr.geom_ray(rr.HFIELD, P, V, (0, 0, 0), hf)
        rob = rr.robust((P, V), scene)
        got = rr.march(rr.HFIELD, P, V, (0, 0, 0), hf)
        print(f"{name}: {len(P)} rays, robust {int(rob.sum())}, hits {int((ref >= 0).sum())}")
        assert rob.mean() >= 0.9, name
        assert ((got >= 0) == (ref >= 0))[rob].all(), name
        assert np.abs(got - ref)[rob & (ref >= 0)].max() <= 1e-6, name
        if name == "nodes":
            assert rob.all() and np.allclose(ref, (P[:, 2] - e[rc[:, 0], rc[:, 1]] * 0.5) / -V[:, 2], atol=1e-9)


# ---- the generated ray sets of tests/test_gpu_ray.py at the scenes' nominal poses
def _s24_scene(lib, env):
    m = ms.scene("s24")
    tab = m.s24_randomize(env, 1)
    ng = m.ngeom
    pos = m.array("geom_pos").reshape(ng, 3).copy(); mat = np.array([rr.quat2mat(q) for q in m.array("geom_quat").reshape(ng, 4)])
    body = m.array("geom_bodyid")
    for g in range(ng):
        if body[g] > 0:
            qa = 7 * (body[g] - 1)
            pos[g] = tab["qpos"][0, qa:qa + 3]; mat[g] = rr.quat2mat(tab["qpos"][0, qa + 3:qa + 7])
    return rr.scene_from_device(pos, mat, tab["geom_size"][0], m.array("geom_type"))


def _many_spheres_scene():
    spec = rr.many_spheres_spec()
    return rr.scene_from_spec(spec)


def _sets(lib):
    prim = rr.scene_from_spec(rr.primitives_spec())
    yield "primitives", prim, rr.primitive_rays(prim, 130)
    for n in (63, 65):
        P, V = rr.primitive_rays(prim, 130)
        yield "primitives[:%d]" % n, prim, (P[:n], V[:n])
    hs = rr.hfield_scene()
    yield "hfield", hs, rr.hfield_rays(hs)
    for env in (3, 4, 5, 6, 7):
        sc = _s24_scene(lib, env)
        yield "s24 env %d" % env, sc, rr.s24_rays(sc, 96)
    ms_ = _many_spheres_scene()
    yield "many spheres", ms_, rr.many_spheres_rays(ms_)
    for name in ("A", "B", "C"):      # the grid-line families (unrotated field at the origin: the frame rays are world rays)
        sc = rr.terrain_scene(rr.terrain(name))
        for fam, rays in rr.hfield_families(name):
            yield "terrain %s %s" % (name, fam), sc, rays
    two = rr.two_fields_scene()
    yield "two fields", two, rr.two_fields_rays(two)
    level = rr.scene_from_spec(rr.level_spec())
    yield "level scan", level, rr.level_rays()
    yield "far origins", prim, rr.far_rays(prim)
    yield "extreme points", prim, rr.extreme_point_rays(prim)[:2]


def test_non_robust_share_of_every_ray_set(lib):
    for name, scene, rays in _sets(lib):
        rob = rr.robust(rays, scene)
        print(f"{name}: {len(rob)} rays, non-robust share {1 - rob.mean():.3f}")
        assert 1 - rob.mean() <= 0.10, name
    prim = rr.scene_from_spec(rr.primitives_spec())
    assert rr.robust(tuple(a[:1] for a in rr.primitive_rays(prim, 130)), prim).all(), "the one-ray set"


# ---- C ABI
def test_ray_symbols_and_skipped_geoms(lib):
    for name in ("mjh_ray", "mjh_ray_device", "mjh_ray_default_options", "mjh_ray_skipped_geoms"):
        assert hasattr(lib, name), name
        assert name in [s[0] for s in capi.SYMBOLS]
    assert rr.mesh_model(lib).ray_skipped_geoms() == 2
    assert ms.scene("s24").ray_skipped_geoms() == 0
    # an hfield geom without an asset is skipped as well
    b = lib.mjh_builder_create()
    lib.mjh_builder_add_geom(b, b"h", 0, rr.HFIELD, D(1, 1, 1), None, None, None, -1, -1, -1, -1)
    bd = lib.mjh_builder_add_body(b, b"o", 0, D(0, 0, 1), None, 0.0)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"g", bd, rr.SPHERE, D(0.1, 0, 0), None, None, None, -1, -1, -1, -1)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    assert m.ray_skipped_geoms() == 1


def test_ray_default_options(lib):
    o = capi.RayOptions(site=7, bodyexclude=7, flg_static=7, per_env=7, cutoff=7.0)
    lib.mjh_ray_default_options(C.byref(o))
    assert (o.site, o.bodyexclude, o.flg_static, o.per_env, o.cutoff) == (-1, -1, 1, 0, 0.0)
