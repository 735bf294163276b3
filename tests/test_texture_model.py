"""Textures in the model: mjh_builder_add_texture / _builtin / mjh_builder_set_geom_texture (tables, defaults, limits, errors), the
builtin generators byte for byte against tests/texture_ref.py, name lookup (objtype 7), mjh_model_replicate's refusal, and <texture>
and a material's texture / texrepeat / texuniform in the MJCF loader (mode 1: attributes, defaults, default classes, precedence, every
skipped case with its note; mode 0: the tables and the notes of the loader before textures, character for character).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mujoco_sim_amd as ms
import refmodels
import texture_check as tc
import texture_ref as tr
from helpers import D
from mujoco_sim_amd import capi
from test_geom_rgba import LOADER

ERR_ARG = -1
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TEX_ARRAYS = [n for n, _, _ in capi._ARRAYS10 + capi._ARRAYS10B]
OLD_ARRAYS = [n for n, _, _ in capi._ARRAYS + capi._ARRAYS2 + capi._ARRAYS3 + capi._ARRAYS4 + capi._ARRAYS5 + capi._ARRAYS6 + capi._ARRAYS7 + capi._ARRAYS8 + capi._ARRAYS9]


def _builder(lib):
    """geoms added on bodies a, b, a_child: the compiler orders them a, a_child, b behind the world's"""
    b = lib.mjh_builder_create()
    floor = lib.mjh_builder_add_geom(b, b"floor", 0, 0, D(0, 0, 0.1), None, None, None, -1, -1, -1, -1)
    a1 = lib.mjh_builder_add_body(b, b"a", 0, D(0, 0, 1), None, 0.0)
    b1 = lib.mjh_builder_add_body(b, b"b", 0, D(1, 0, 1), None, 0.0)
    a2 = lib.mjh_builder_add_body(b, b"a_child", a1, D(0, 0, 1), None, 0.0)
    geoms = [floor]
    for bd, nm, gn in ((a1, b"ja", b"ga"), (b1, b"jb", b"gb"), (a2, b"jc", b"gc")):
        lib.mjh_builder_add_joint(b, nm, bd, 3, None, D(0, 1, 0), None, 0, 0, 0, 0, 0)
        geoms.append(lib.mjh_builder_add_geom(b, gn, bd, 6, D(0.1, 0.2, 0.3), None, None, None, -1, -1, -1, -1))
    return b, geoms


def _compile(lib, b):
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    lib.mjh_builder_destroy(b)
    return ms.Model(p, lib)


def test_builder_tables_follow_the_geom_order(lib):
    b, (floor, ga, gb, gc) = _builder(lib)
    t8, t75 = tc.distinct(1), tc.distinct(2, 7, 5)
    assert tc.add_texture(lib, b, b"eight", t8) == 0
    assert tc.add_builtin(lib, b, b"grid", tr.CHECKER, 4, 6, (0.1, 0.2, 0.3), (0.2, 0.3, 0.4)) == 1
    assert tc.add_texture(lib, b, b"odd", t75) == 2
    st = lib.mjh_builder_set_geom_texture
    assert st(b, floor, 1, D(1, 1), 1) == 0
    assert st(b, gb, 0, D(2.5, 0.5), 0) == 0
    assert st(b, gc, 2, None, 0) == 0                  # NULL texrepeat: 1 1
    assert st(b, ga, 2, D(3, 3), 1) == 0 and st(b, ga, -1, None, 0) == 0      # set, then cleared
    m = _compile(lib, b)
    assert (m.ntex, m.ntexdata) == (3, 64 + 24 + 35) and m.c.ntex == 3
    np.testing.assert_array_equal(m.array("tex_width"), [8, 4, 7])
    np.testing.assert_array_equal(m.array("tex_height"), [8, 6, 5])
    np.testing.assert_array_equal(m.array("tex_adr"), [0, 64, 88])
    assert m.array("tex_rgb").dtype == np.uint8 and m.array("tex_rgb").size == 3 * m.ntexdata
    got = tc.model_textures(m)
    np.testing.assert_array_equal(got[0], t8); np.testing.assert_array_equal(got[2], t75)
    np.testing.assert_array_equal(got[1], tr.builtin(tr.CHECKER, 4, 6, (0.1, 0.2, 0.3), (0.2, 0.3, 0.4)))
    # compiled geom order: floor, ga (body a), gc (a_child), gb (b)
    order = [m.name2id(2, n) for n in ("floor", "ga", "gc", "gb")]
    assert order == [0, 1, 2, 3]
    np.testing.assert_array_equal(m.array("geom_texid"), [1, -1, 2, 0])
    np.testing.assert_array_equal(m.array("geom_texrepeat").reshape(-1, 2), [[1, 1], [1, 1], [1, 1], [2.5, 0.5]])
    np.testing.assert_array_equal(m.array("geom_texuniform"), [1, 0, 0, 0])
    assert [m.name2id(7, n) for n in ("eight", "grid", "odd", "nope")] == [0, 1, 2, -1]
    assert [lib.mjh_id2name(m.ptr, 7, i) for i in range(3)] == [b"eight", b"grid", b"odd"]
    assert lib.mjh_id2name(m.ptr, 7, 3) is None and lib.mjh_id2name(m.ptr, 7, -1) is None and lib.mjh_id2name(m.ptr, 8, 0) is None
    assert m.name2id(6, "grid") == -1 and m.name2id(8, "grid") == -1
    assert not lib.mjh_model_replicate(m.ptr, 2)
    assert b"texture" in lib.mjh_last_error()


SIZES = [(8, 8), (7, 5), (1, 1)]
COLOURS = ((0.1, 0.2, 0.3), (0.9, 0.55, 0.4), (1.0, 0.0, 0.5))


@pytest.mark.parametrize("kind", [tr.FLAT, tr.CHECKER, tr.GRADIENT])
@pytest.mark.parametrize("mark", [tr.NONE, tr.EDGE, tr.CROSS])
def test_builtins_equal_the_reference_byte_for_byte(lib, kind, mark):
    b, _ = _builder(lib)
    for k, (w, h) in enumerate(SIZES):
        assert tc.add_builtin(lib, b, b"t%d" % k, kind, w, h, COLOURS[0], COLOURS[1], mark, COLOURS[2]) == k
    assert tc.add_builtin(lib, b, b"dflt", kind, 6, 4, mark=mark) == 3      # NULL colours: 0.8 0.8 0.8, 0.5 0.5 0.5, 0 0 0
    m = _compile(lib, b)
    got = tc.model_textures(m)
    for k, (w, h) in enumerate(SIZES):
        np.testing.assert_array_equal(got[k], tr.builtin(kind, w, h, COLOURS[0], COLOURS[1], mark, COLOURS[2]), err_msg=f"{kind} {mark} {w}x{h}")
    np.testing.assert_array_equal(got[3], tr.builtin(kind, 6, 4, mark=mark))


def test_builtin_definitions_by_hand():
    """the reference itself against values worked out by hand"""
    c = tr.builtin(tr.CHECKER, 4, 2, (0.1, 0.2, 0.3), (0.2, 0.3, 0.4))
    assert c[0, 0].tolist() == [26, 51, 77] and c[0, 2].tolist() == [51, 77, 102] and c[1, 0].tolist() == [51, 77, 102] and c[1, 3].tolist() == [26, 51, 77]
    g = tr.builtin(tr.GRADIENT, 3, 3, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert g[1, 1].tolist() == [0, 0, 0] and g[0, 0].tolist() == [255, 255, 255] and g[1, 0].tolist() == [255, 255, 255]
    g = tr.builtin(tr.GRADIENT, 5, 1, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert g[0, :, 0].tolist() == [255, 128, 0, 128, 255]
    e = tr.builtin(tr.FLAT, 4, 3, (1.0, 1.0, 1.0), mark=tr.EDGE, markrgb=(0.0, 0.0, 1.0))
    assert (e[1, 1:3] == 255).all() and (e[0] == [0, 0, 255]).all() and (e[:, 0] == [0, 0, 255]).all() and (e[:, 3] == [0, 0, 255]).all() and (e[2] == [0, 0, 255]).all()
    x = tr.builtin(tr.FLAT, 4, 3, (1.0, 1.0, 1.0), mark=tr.CROSS, markrgb=(0.0, 0.0, 1.0))
    assert (x[1] == [0, 0, 255]).all() and (x[:, 2] == [0, 0, 255]).all() and (x[0, [0, 1, 3]] == 255).all() and (x[2, [0, 1, 3]] == 255).all()
    # the mapping: the reference floor's 1 m squares with a corner at the origin; a box face in the middle of a texel
    row, col = tr.texel_index([[0.2, 0.3, 0], [-0.2, 0.3, 0], [0.2, -0.3, 0], [1.2, 0.3, 0], [0.2, 2.3, 0]], (1.0, 1.0), (1.0, 1.0), 512, 512)
    assert (col >= 256).tolist() == [True, False, True, False, True] and (row >= 256).tolist() == [False, False, True, False, False]
    row, col = tr.texel_index([[0.25, -0.15, 0.1]], tr.extents(6, (0.25, 0.15, 0.2), False), tc.REPEAT, 8, 8)
    assert (int(row[0]), int(col[0])) == (7, 7)      # u = 0.95, v = 0.9


def test_limits_and_errors(lib):
    assert (capi.MAXTEXSIZE, capi.MAXTEXDATA) == (4096, 1 << 24)
    hdr = open(os.path.join(ROOT, "include", "mjhip.h")).read()
    assert re.search(r"#define\s+MJH_MAXTEXSIZE\s+4096\b", hdr) and re.search(r"#define\s+MJH_MAXTEXDATA\s+\(1 << 24\)", hdr)
    b, (floor, ga, gb, gc) = _builder(lib)
    bi, at, st = lib.mjh_builder_add_texture_builtin, lib.mjh_builder_add_texture, lib.mjh_builder_set_geom_texture
    one = (C.c_ubyte * 3)(1, 2, 3)
    for w, h in ((0, 4), (4, 0), (-1, 4), (4097, 1), (1, 4097)):
        assert bi(b, b"bad", 0, 0, w, h, None, None, None) == ERR_ARG and b"4096" in lib.mjh_last_error(), (w, h)
        assert at(b, b"bad", w, h, one) == ERR_ARG and b"4096" in lib.mjh_last_error()
    assert at(b, b"bad", 1, 1, None) == ERR_ARG
    for kind, mark in ((-1, 0), (3, 0), (0, -1), (0, 3)):
        assert bi(b, b"bad", kind, mark, 4, 4, None, None, None) == ERR_ARG
    for bad in (dict(rgb1=D(1.5, 0, 0)), dict(rgb2=D(0, -0.1, 0)), dict(markrgb=D(0, 0, float("nan")))):
        assert bi(b, b"bad", 1, 1, 4, 4, bad.get("rgb1"), bad.get("rgb2"), bad.get("markrgb")) == ERR_ARG and b"[0, 1]" in lib.mjh_last_error()
    # 4096 x 4096 is the whole budget of a model: one fits, nothing more does
    assert bi(b, b"huge", 0, 0, 4096, 4096, None, None, None) == 0
    assert bi(b, b"more", 0, 0, 1, 1, None, None, None) == ERR_ARG and b"2^24" in lib.mjh_last_error()
    assert at(b, b"more", 1, 1, one) == ERR_ARG and b"2^24" in lib.mjh_last_error()
    for geom, tex, rep in ((-1, 0, D(1, 1)), (17, 0, D(1, 1)), (gb, 1, D(1, 1)), (gb, -2, D(1, 1)), (gb, 0, D(0, 1)), (gb, 0, D(1, -2)),
                           (gb, 0, D(float("inf"), 1)), (gb, 0, D(1, float("nan")))):
        assert st(b, geom, tex, rep, 0) == ERR_ARG and lib.mjh_last_error(), (geom, tex)
    m = _compile(lib, b)
    assert (m.ntex, m.ntexdata) == (1, 1 << 24) and (m.array("geom_texid") == -1).all(), "a refused call changes nothing"
    assert (m.array("tex_rgb") == 204).all()


def test_a_mesh_geom_takes_no_texture(lib):
    import ray_tri_ref as rt
    b = lib.mjh_builder_create()
    asset = rt.add_mesh(lib, b, *rt.MESHES["jaw"]())
    bd = lib.mjh_builder_add_body(b, b"mb", 0, D(0, 0, 1), None, 0.0)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    g = lib.mjh_builder_add_mesh_geom(b, b"mg", bd, asset, None, None, None, -1, -1, -1, -1)
    assert g >= 0 and tc.add_builtin(lib, b, b"t", tr.FLAT, 2, 2) == 0
    assert lib.mjh_builder_set_geom_texture(b, g, 0, None, 0) == ERR_ARG and b"mesh" in lib.mjh_last_error()
    lib.mjh_builder_destroy(b)


def test_models_without_textures(lib):
    m = ms.scene("s24")
    assert m.ntex == 0 and m.ntexdata == 0 and all(m.array(n).size == 0 for n in TEX_ARRAYS[:4])
    assert (m.array("geom_texid") == -1).all() and (m.array("geom_texrepeat") == 1).all() and (m.array("geom_texuniform") == 0).all()
    assert m.name2id(7, "anything") == -1 and lib.mjh_id2name(m.ptr, 7, 0) is None
    assert m.replicate(2).ntex == 0      # still packed


def test_every_new_symbol_is_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mjhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mjh_[a-z0-9_]+)\s*\(", hdr))
    new = {"mjh_builder_add_texture", "mjh_builder_add_texture_builtin", "mjh_builder_set_geom_texture", "mjh_load_set_textures",
           "mjh_render_set_texturing", "mjh_render_get_texturing"}
    assert new <= declared
    bound = {n for n, _, _ in capi.SYMBOLS}
    assert new <= bound and all(hasattr(lib, n) for n in new)
    assert capi.TEXBUILTIN == dict(flat=0, checker=1, gradient=2) and capi.TEXMARK == dict(none=0, edge=1, cross=2)
    for name, value in (("MJH_TEXBUILTIN_FLAT", 0), ("MJH_TEXBUILTIN_CHECKER", 1), ("MJH_TEXBUILTIN_GRADIENT", 2), ("MJH_TEXMARK_NONE", 0), ("MJH_TEXMARK_EDGE", 1), ("MJH_TEXMARK_CROSS", 2)):
        assert re.search(r"\b%s = %d\b" % (name, value), hdr), name


# ------------------------------------------------------------------ the loader
ASSETS = """<mujoco>
  <default>
    <texture rgb2="0.3 0.2 0.1"/>
    <material texrepeat="3 2"/>
    <default class="marked"><texture mark="edge" markrgb="1 0 0"/><material texuniform="true"/></default>
  </default>
  <asset>
    <texture name="grid" type="2d" builtin="checker" width="8" height="6" rgb1=".1 .2 .3"/>
    <texture name="plain" type="2d" builtin="flat" width="5"/>
    <texture name="glow" class="marked" type="2d" builtin="gradient" width="7" height="5" rgb1="1 1 1" rgb2="0 0 1"/>
    <texture name="cross" type="2d" builtin="flat" width="4" mark="cross" markrgb="0 1 0" rgb1="0.5 0.5 0.5"/>
    <texture name="sky" type="skybox" builtin="gradient" width="8" height="8"/>
    <texture name="die" type="cube" builtin="flat" width="8" height="8"/>
    <texture name="untyped" builtin="flat" width="8" height="8"/>
    <texture name="cat" type="2d" file="cat.png"/>
    <texture name="noise" type="2d" builtin="flat" width="8" mark="random" random="0.1"/>
    <texture name="wide" type="2d" builtin="flat" width="5000" height="2"/>
    <material name="grid" texture="grid" texuniform="true" texrepeat="1 1"/>
    <material name="plain" texture="plain" rgba="0.5 0.25 1 1"/>
    <material name="glow" class="marked" texture="glow" reflectance="0.2"/>
    <material name="ghost" texture="nope"/>
    <material name="catmat" texture="cat"/>
    <material name="bare" rgba="0 1 0 1"/>
  </asset>
  <worldbody>
    <geom name="floor" type="plane" size="0 0 0.1" material="grid"/>
    <geom name="own" type="box" size="0.1 0.1 0.1" pos="1 0 0" material="plain" rgba="0.25 0.5 0.75 1"/>
    <geom name="mat" type="box" size="0.1 0.1 0.1" pos="2 0 0" material="plain"/>
    <geom name="glow" type="sphere" size="0.1" pos="3 0 0" material="glow"/>
    <geom name="ghost" type="sphere" size="0.1" pos="4 0 0" material="ghost"/>
    <geom name="cat" type="sphere" size="0.1" pos="5 0 0" material="catmat"/>
    <geom name="bare" type="sphere" size="0.1" pos="6 0 0" material="bare"/>
    <geom name="none" type="sphere" size="0.1" pos="7 0 0"/>
    <body name="b" pos="0 0 1"><freejoint/><geom name="child" type="capsule" size="0.05 0.1" material="grid"/></body>
  </worldbody>
</mujoco>"""


def _tex(m, geom):
    g = m.name2id(2, geom)
    return int(m.array("geom_texid")[g]), m.array("geom_texrepeat").reshape(-1, 2)[g].tolist(), int(m.array("geom_texuniform")[g])


def test_loader_mode_1(lib):
    m = ms.load_mjcf(ASSETS, textures=True)
    assert m.ntex == 4 and [lib.mjh_id2name(m.ptr, 7, i) for i in range(4)] == [b"grid", b"plain", b"glow", b"cross"]
    got = tc.model_textures(m)
    # the unnamed default class gives rgb2; height defaults to width; the class "marked" adds the mark on top
    np.testing.assert_array_equal(got[0], tr.builtin(tr.CHECKER, 8, 6, (0.1, 0.2, 0.3), (0.3, 0.2, 0.1)))
    np.testing.assert_array_equal(got[1], tr.builtin(tr.FLAT, 5, 5, (0.8, 0.8, 0.8), (0.3, 0.2, 0.1)))
    np.testing.assert_array_equal(got[2], tr.builtin(tr.GRADIENT, 7, 5, (1, 1, 1), (0, 0, 1), tr.EDGE, (1, 0, 0)))
    np.testing.assert_array_equal(got[3], tr.builtin(tr.FLAT, 4, 4, (0.5, 0.5, 0.5), (0.3, 0.2, 0.1), tr.CROSS, (0, 1, 0)))
    assert _tex(m, "floor") == (0, [1.0, 1.0], 1) and _tex(m, "child") == (0, [1.0, 1.0], 1)
    assert _tex(m, "mat") == (1, [3.0, 2.0], 0), "texrepeat from the default class, texuniform false"
    assert _tex(m, "glow") == (2, [3.0, 2.0], 1), "texuniform from the class"
    # precedence: the geom's own rgba wins the colour, the material's texture is kept
    rgba = m.array("geom_rgba").reshape(-1, 4)
    assert rgba[m.name2id(2, "own")].tolist() == [0.25, 0.5, 0.75, 1.0] and _tex(m, "own") == (1, [3.0, 2.0], 0)
    assert rgba[m.name2id(2, "mat")].tolist() == [0.5, 0.25, 1.0, 1.0] and rgba[m.name2id(2, "floor")].tolist() == [1.0, 1.0, 1.0, 1.0]
    for plain in ("ghost", "cat", "bare", "none"):
        assert _tex(m, plain)[0] == -1, plain
    assert rgba[m.name2id(2, "ghost")].tolist() == [1.0, 1.0, 1.0, 1.0] and rgba[m.name2id(2, "bare")].tolist() == [0.0, 1.0, 0.0, 1.0]
    # every skipped case carries its note
    for part in ('skipped <texture sky type="skybox">', 'skipped <texture die type="cube">', 'skipped <texture untyped type="cube">',
                 "skipped <texture cat> (file textures are not supported", 'skipped <texture noise mark="random">', "skipped <texture wide> (", "4096",
                 "material ghost: texture nope not loaded", "material catmat: texture cat not loaded"):
        assert part in m.note, (part, m.note)
    # the remaining material attributes keep their note; texture, texrepeat and texuniform have none in this mode
    assert "ignored material attribute reflectance of glow (colour only)" in m.note
    assert not re.search(r"ignored material attribute tex", m.note), m.note


def test_loader_mesh_geom_keeps_its_plain_colour(lib, tmp_path):
    import ray_tri_ref as rt
    verts, faces = rt.MESHES["jaw"]()[:2]
    stl = tmp_path / "jaw.stl"
    with open(stl, "w") as f:
        f.write("solid jaw\n")
        for tri in np.asarray(faces):
            f.write("facet normal 0 0 0\nouter loop\n" + "".join("vertex %r %r %r\n" % tuple(float(x) for x in np.asarray(verts)[i]) for i in tri) + "endloop\nendfacet\n")
        f.write("endsolid jaw\n")
    xml = tmp_path / "scene.xml"
    xml.write_text("""<mujoco><asset><mesh name="jaw" file="jaw.stl"/><texture name="t" type="2d" builtin="flat" width="2"/>
      <material name="m" texture="t" rgba="1 0 0 1"/></asset><worldbody><geom name="ball" type="sphere" size="0.1" material="m"/>
      <body pos="0 0 1"><freejoint/><geom name="jawg" type="mesh" mesh="jaw" material="m"/></body></worldbody></mujoco>""")
    m = ms.load_mjcf(path=str(xml), textures=True)
    assert m.ptr and m.ntex == 1
    assert _tex(m, "ball")[0] == 0 and _tex(m, "jawg")[0] == -1
    assert m.array("geom_rgba").reshape(-1, 4)[m.name2id(2, "jawg")].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert "ignored texture of material m on mesh geom jawg" in m.note


def test_loader_mode_0_is_the_loader_before_textures(lib):
    off = ms.load_mjcf(ASSETS)
    on = ms.load_mjcf(ASSETS, textures=True)
    assert off.ntex == 0 and off.ntexdata == 0 and (off.array("geom_texid") == -1).all() and on.ntex == 4
    # (six materials: their own texture / texrepeat / texuniform and what the default classes add, 13 attributes in all)
    assert "<texture" not in off.note and off.note.count("ignored material attribute tex") == 13
    for n in OLD_ARRAYS:
        np.testing.assert_array_equal(off.array(n), on.array(n), err_msg=n)
    # the switch is per thread and stays where it was put
    lib.mjh_load_set_textures(1)
    try:
        assert ms.load_mjcf(ASSETS).ntex == 4
    finally:
        lib.mjh_load_set_textures(0)
    assert ms.load_mjcf(ASSETS).ntex == 0


# the notes of the loader before textures existed (the parent commit), character for character
NOTE_LOADER = ("no <option solver>: MuJoCo's default is Newton, this engine solves the same dual problem with PGS (100 iterations, tolerance 1e-8); ignored material attribute texture of tiles (colour only); ignored material attribute texrepeat of tiles (colour only); ignored material attribute reflectance of bare (colour only); ")
NOTE_EMPTY = ("integrator=RK4 ignored: the step1 / step2 split of the reference loop always integrates with Euler (mj_main.cpp:83,108); no <option solver>: MuJoCo's default is Newton, this engine solves the same dual problem with PGS (100 iterations, tolerance 1e-8); ignored material attribute texture of grid (colour only); ignored material attribute texrepeat of grid (colour only); ignored material attribute texuniform of grid (colour only); ignored material attribute reflectance of grid (colour only); ")


def test_mode_0_notes_character_for_character(lib):
    m = ms.load_mjcf(LOADER)
    assert m.ntex == 0 and m.note == NOTE_LOADER
    w = ms.load_mjcf(path=os.path.join(refmodels.model_dir(), "world", "empty.xml"))
    assert w.ntex == 0 and w.note == NOTE_EMPTY


def test_loader_string_of_the_colour_tests_in_mode_1(lib):
    m = ms.load_mjcf(LOADER, textures=True)
    assert m.ntex == 1 and _tex(m, "tiles") == (0, [2.0, 2.0], 0)
    np.testing.assert_array_equal(tc.model_textures(m)[0], tr.builtin(tr.CHECKER, 8, 8))
    assert "ignored material attribute reflectance of bare (colour only)" in m.note and "attribute tex" not in m.note


@pytest.mark.parametrize("path", ["world/empty.xml", "test/pendulum.xml", "ontology/scene.xml"])
def test_the_reference_world_files_in_mode_1(lib, path):
    """<texture name="grid" type="2d" builtin="checker" width="512" height="512" rgb1=".1 .2 .3" rgb2=".2 .3 .4"/> and
    <material name="grid" texture="grid" texrepeat="1 1" texuniform="true"/> in each; ontology/scene.xml is tests/golden/ontology_scene.xml"""
    p = os.path.join(HERE, "golden", "ontology_scene.xml") if path.startswith("ontology") else os.path.join(refmodels.model_dir(), path)
    m = ms.load_mjcf(path=p, textures=True)
    assert m.ptr, lib.mjh_last_error()
    floor = m.name2id(2, "floor")
    assert floor >= 0 and m.array("geom_texid")[floor] >= 0
    t = int(m.array("geom_texid")[floor])
    assert lib.mjh_id2name(m.ptr, 7, t) == b"grid"
    assert m.array("geom_texrepeat").reshape(-1, 2)[floor].tolist() == [1.0, 1.0] and m.array("geom_texuniform")[floor] == 1
    np.testing.assert_array_equal(tc.model_textures(m)[t], tr.builtin(**tc.CHECKER))
    assert "ignored material attribute tex" not in m.note
    off = ms.load_mjcf(path=p)
    assert off.ntex == 0
    for n in OLD_ARRAYS:
        np.testing.assert_array_equal(off.array(n), m.array(n), err_msg=n)
