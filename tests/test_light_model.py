"""Lights in the model: mjh_builder_add_light (defaults, errors, the ninth light), the compiled light_* tables and their reorder-following,
name lookup (objtype 6), mjh_model_replicate's refusal, and <light> in the MJCF loader (attributes, default classes, notes, the
reference's world files, a builder model and its MJCF twin).  No GPU."""
import os

import numpy as np
import pytest

import mujoco_sim_amd as ms
import refmodels
from helpers import D
from mujoco_sim_amd import capi

ERR_ARG = -1
HERE = os.path.dirname(os.path.abspath(__file__))
LIGHT_ARRAYS = [n for n, _, _ in capi._ARRAYS9]
OLD_ARRAYS = [n for n, _, _ in capi._ARRAYS + capi._ARRAYS2 + capi._ARRAYS3 + capi._ARRAYS4 + capi._ARRAYS5 + capi._ARRAYS6 + capi._ARRAYS7 + capi._ARRAYS8]


def _two_body_builder(lib):
    """bodies added as a, b, a_child: the compiler renumbers them depth-first to a, a_child, b"""
    b = lib.mjh_builder_create()
    a1 = lib.mjh_builder_add_body(b, b"a", 0, D(0, 0, 1), None, 0.0)
    b1 = lib.mjh_builder_add_body(b, b"b", 0, D(1, 0, 1), None, 0.0)
    a2 = lib.mjh_builder_add_body(b, b"a_child", a1, D(0, 0, 1), None, 0.0)
    for bd, nm in ((a1, b"ja"), (b1, b"jb"), (a2, b"jc")):
        lib.mjh_builder_add_joint(b, nm, bd, 3, None, D(0, 1, 0), None, 0, 0, 0, 0, 0)
        lib.mjh_builder_add_geom(b, None, bd, 2, D(0.1, 0, 0), None, None, None, -1, -1, -1, -1)
    return b, a1, b1, a2


def test_builder_lights_defaults_errors_and_reordering(lib):
    assert capi.MAXLIGHT == 8
    b, a1, b1, a2 = _two_body_builder(lib)
    add = lib.mjh_builder_add_light
    assert add(b, b"lamp", b1, D(0.1, 0.2, 0.3), D(0, 3, -4), 0, 0, D(0.5, 0.25, 1.5), D(0.1, 0.0, 0.2), 30.0, 2.0) == 0
    assert add(b, b"plain", a2, None, None, -1, -1, None, None, 45.0, 10.0) == 1      # every default
    assert add(b, b"sun", 0, None, D(1, 0, 0), 1, 1, None, None, 180.0, 0.0) == 2
    for bad, word in ((dict(dir=D(0, 0, 0)), b"dir"), (dict(dif=D(0.1, -0.1, 0.1)), b"colour"), (dict(amb=D(0.1, float("nan"), 0.1)), b"colour"),
                      (dict(dif=D(float("inf"), 0, 0)), b"colour"), (dict(cutoff=0.0), b"cutoff"), (dict(cutoff=180.5), b"cutoff"), (dict(cutoff=-3.0), b"cutoff"),
                      (dict(exponent=-1.0), b"exponent"), (dict(body=17), b"body"), (dict(body=-1), b"body")):
        rc = add(b, b"bad", bad.get("body", 0), None, bad.get("dir"), 0, 1, bad.get("dif"), bad.get("amb"), bad.get("cutoff", 45.0), bad.get("exponent", 10.0))
        assert rc == ERR_ARG and word in lib.mjh_last_error(), (bad, lib.mjh_last_error())
    assert lib.mjh_builder_set_light_active(b, 1, 0) == 0 and lib.mjh_builder_set_light_active(b, 3, 0) == ERR_ARG
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    assert m.nlight == 3 and m.c.nlight == 3
    # bodies renumbered depth-first (a 1, a_child 2, b 3): a light on a body declared late follows it
    np.testing.assert_array_equal(m.array("light_bodyid"), [m.name2id(0, "b"), m.name2id(0, "a_child"), 0])
    np.testing.assert_array_equal(m.array("light_bodyid"), [3, 2, 0])
    np.testing.assert_array_equal(m.array("light_pos").reshape(3, 3), [[0.1, 0.2, 0.3], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_allclose(m.array("light_dir").reshape(3, 3), [[0, 0.6, -0.8], [0, 0, -1], [1, 0, 0]], atol=1e-15)
    np.testing.assert_array_equal(m.array("light_directional"), [0, 0, 1])
    np.testing.assert_array_equal(m.array("light_castshadow"), [0, 1, 1])
    np.testing.assert_array_equal(m.array("light_active"), [1, 0, 1])
    np.testing.assert_array_equal(m.array("light_diffuse").reshape(3, 3), [[0.5, 0.25, 1.5], [0.7, 0.7, 0.7], [0.7, 0.7, 0.7]])
    np.testing.assert_array_equal(m.array("light_ambient").reshape(3, 3), [[0.1, 0.0, 0.2], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(m.array("light_cutoff"), [30.0, 45.0, 180.0])
    np.testing.assert_array_equal(m.array("light_exponent"), [2.0, 10.0, 0.0])
    assert [m.name2id(6, n) for n in ("lamp", "plain", "sun", "nope")] == [0, 1, 2, -1]
    assert [lib.mjh_id2name(m.ptr, 6, i) for i in (0, 1, 2)] == [b"lamp", b"plain", b"sun"]
    assert lib.mjh_id2name(m.ptr, 6, 3) is None and lib.mjh_id2name(m.ptr, 6, -1) is None and lib.mjh_id2name(m.ptr, 7, 0) is None
    assert m.name2id(0, "a_child") == 2 and m.name2id(5, "lamp") == -1 and m.name2id(7, "lamp") == -1
    assert not lib.mjh_model_replicate(m.ptr, 2)
    assert b"light" in lib.mjh_last_error()


def test_the_ninth_light(lib):
    b, a1, b1, a2 = _two_body_builder(lib)
    for k in range(8):
        assert lib.mjh_builder_add_light(b, b"l%d" % k, 0, None, None, 0, 1, None, None, 45.0, 10.0) == k
    assert lib.mjh_builder_add_light(b, b"l8", 0, None, None, 0, 1, None, None, 45.0, 10.0) == ERR_ARG
    assert b"8" in lib.mjh_last_error()
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    assert m.nlight == 8


def test_models_without_lights(lib):
    m = ms.scene("s24")
    assert m.nlight == 0 and all(m.array(n).size == 0 for n in LIGHT_ARRAYS)
    assert m.name2id(6, "anything") == -1 and lib.mjh_id2name(m.ptr, 6, 0) is None
    assert m.replicate(2).nlight == 0      # still packed


BODY = """
<mujoco>
  <compiler angle="degree"/>
  <default>
    <light diffuse="0.2 0.3 0.4" cutoff="60"/>
    <default class="warm"><light ambient="0.1 0.05 0" exponent="3"/></default>
  </default>
  <worldbody>
    <geom name="floor" type="plane" size="3 3 0.1"/>
    %s
    <body name="cart" pos="0 0 1">
      <joint name="slide" type="slide" axis="1 0 0"/>
      <geom name="cartg" type="box" size="0.2 0.1 0.05"/>
      %s
      <body name="pole" pos="0 0 0.1">
        <joint name="hinge" type="hinge" axis="0 1 0"/>
        <geom name="poleg" type="capsule" size="0.03 0.4" pos="0 0 0.4"/>
        %s
      </body>
    </body>
    %s
  </worldbody>
</mujoco>
"""
LIGHTS = ('<light name="top" pos="0 0 4" dir="0 0 -2" diffuse="1 1 1" castshadow="false"/>',
          '<light class="warm" pos="0.3 0 0.1" directional="true" specular="0.3 0.3 0.3"/>',
          '<light name="tip" mode="fixed" pos="0 0 0.8" dir="1 0 -1" active="false" attenuation="1 0.1 0"/>',
          '<light name="chase" mode="track" pos="0 -3 1"/> <light name="plainatt" attenuation="1 0 0"/>')


def test_loader_lights(lib):
    m = ms.load_mjcf(BODY % LIGHTS)
    assert m.nlight == 4
    assert "chase" in m.note and "track" in m.note
    assert m.note.count("specular / attenuation") == 2 and "light1" in m.note and "<light tip>" in m.note and "plainatt" not in m.note
    assert "ignored <light>" not in m.note
    assert [lib.mjh_id2name(m.ptr, 6, i) for i in range(4)] == [b"top", b"light1", b"tip", b"plainatt"]
    np.testing.assert_array_equal(m.array("light_bodyid"), [0, m.name2id(0, "cart"), m.name2id(0, "pole"), 0])
    np.testing.assert_array_equal(m.array("light_pos").reshape(4, 3), [[0, 0, 4], [0.3, 0, 0.1], [0, 0, 0.8], [0, 0, 0]])
    np.testing.assert_allclose(m.array("light_dir").reshape(4, 3), [[0, 0, -1], [0, 0, -1], [np.sqrt(0.5), 0, -np.sqrt(0.5)], [0, 0, -1]], atol=1e-15)
    np.testing.assert_array_equal(m.array("light_directional"), [0, 1, 0, 0])
    np.testing.assert_array_equal(m.array("light_castshadow"), [0, 1, 1, 1])
    np.testing.assert_array_equal(m.array("light_active"), [1, 1, 0, 1])
    # the unnamed default class gives diffuse and cutoff, the class "warm" adds ambient and exponent on top of it
    np.testing.assert_array_equal(m.array("light_diffuse").reshape(4, 3), [[1, 1, 1], [0.2, 0.3, 0.4], [0.2, 0.3, 0.4], [0.2, 0.3, 0.4]])
    np.testing.assert_array_equal(m.array("light_ambient").reshape(4, 3), [[0, 0, 0], [0.1, 0.05, 0], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(m.array("light_cutoff"), [60.0] * 4)
    np.testing.assert_array_equal(m.array("light_exponent"), [10.0, 3.0, 10.0, 10.0])


def test_loader_skips_the_ninth_light_and_reports_a_bad_one(lib):
    nine = " ".join('<light name="n%d" pos="%d 0 3"/>' % (k, k) for k in range(9))
    m = ms.load_mjcf(BODY % (nine, "", "", ""))
    assert m.nlight == 8 and "n8" in m.note and "at most 8" in m.note
    with pytest.raises(ms.engine.MjhError, match="dir is zero"):
        ms.load_mjcf(BODY % ('<light dir="0 0 0"/>', "", "", ""))


def test_lights_change_no_other_table(lib):
    a = ms.load_mjcf(BODY % ("", "", "", ""))
    b = ms.load_mjcf(BODY % LIGHTS)
    assert a.nlight == 0 and b.nlight == 4
    for n in OLD_ARRAYS:
        np.testing.assert_array_equal(a.array(n), b.array(n), err_msg=n)
    for t, cnt in ((0, a.c.nbody), (1, a.c.njnt), (2, a.c.ngeom)):
        assert [lib.mjh_id2name(a.ptr, t, i) for i in range(cnt)] == [lib.mjh_id2name(b.ptr, t, i) for i in range(cnt)]


@pytest.mark.parametrize("path", ["world/empty.xml", "test/pendulum.xml", "ontology/scene.xml"])
def test_the_reference_world_files_load_with_their_light(lib, path):
    """<light diffuse=".5 .5 .5" pos="0 0 5" dir="0 0 -1"/> in each; ontology/scene.xml is tests/golden/ontology_scene.xml"""
    p = os.path.join(HERE, "golden", "ontology_scene.xml") if path.startswith("ontology") else os.path.join(refmodels.model_dir(), path)
    m = ms.load_mjcf(path=p)
    assert m.ptr, lib.mjh_last_error()
    assert m.nlight == 1 and lib.mjh_id2name(m.ptr, 6, 0) == b"light0"
    np.testing.assert_array_equal(m.array("light_pos"), [0, 0, 5])
    np.testing.assert_array_equal(m.array("light_dir"), [0, 0, -1])
    np.testing.assert_array_equal(m.array("light_diffuse"), [0.5, 0.5, 0.5])
    np.testing.assert_array_equal(m.array("light_ambient"), [0, 0, 0])
    assert m.array("light_directional")[0] == 0 and m.array("light_castshadow")[0] == 1 and m.array("light_active")[0] == 1 and m.array("light_bodyid")[0] == 0
    assert m.array("light_cutoff")[0] == 45.0 and m.array("light_exponent")[0] == 10.0
    # every note is one the loader gave before lights existed: the integrator, the solver, material attributes
    for part in [s.strip() for s in m.note.split(";") if s.strip()]:
        assert part.startswith(("integrator=", "no <option solver>", "ignored material attribute")), part


def test_a_builder_model_and_its_mjcf_twin_have_equal_light_tables(lib):
    b = lib.mjh_builder_create()
    lib.mjh_builder_add_geom(b, b"floor", 0, 0, D(3, 3, 0.1), None, None, None, -1, -1, -1, -1)
    bd = lib.mjh_builder_add_body(b, b"cart", 0, D(0, 0, 1), None, 0.0)
    lib.mjh_builder_add_joint(b, b"slide", bd, 2, None, D(1, 0, 0), None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"cartg", bd, 6, D(0.2, 0.1, 0.05), None, None, None, -1, -1, -1, -1)
    assert lib.mjh_builder_add_light(b, b"top", 0, D(0, 0, 4), D(0.5, 0, -2), 0, 0, D(1, 0.5, 0.25), D(0.1, 0.1, 0.2), 35.0, 4.0) == 0
    assert lib.mjh_builder_add_light(b, b"head", bd, D(0.3, 0, 0.1), None, 1, 1, None, None, 45.0, 10.0) == 1
    assert lib.mjh_builder_set_light_active(b, 1, 0) == 0
    a = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    twin = ms.load_mjcf("""<mujoco><worldbody>
      <geom name="floor" type="plane" size="3 3 0.1"/>
      <light name="top" pos="0 0 4" dir="0.5 0 -2" castshadow="false" diffuse="1 0.5 0.25" ambient="0.1 0.1 0.2" cutoff="35" exponent="4"/>
      <body name="cart" pos="0 0 1"><joint name="slide" type="slide" axis="1 0 0"/><geom name="cartg" type="box" size="0.2 0.1 0.05"/>
        <light name="head" pos="0.3 0 0.1" directional="true" active="false"/></body>
    </worldbody></mujoco>""")
    assert a.nlight == twin.nlight == 2
    for n in LIGHT_ARRAYS:
        np.testing.assert_array_equal(a.array(n), twin.array(n), err_msg=n)
    assert [lib.mjh_id2name(a.ptr, 6, i) for i in range(2)] == [lib.mjh_id2name(twin.ptr, 6, i) for i in range(2)]
