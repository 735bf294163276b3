"""Height fields on the host: builder tables and checks, MJCF loading (inline, binary file, PNG skipped), pair rules and
capacity accounting, and the numpy / oracle reference of the prism narrow phase on hand-made cases (no GPU)."""
import ctypes as C
import struct

import numpy as np
import pytest

import mujoco_sim_amd as ms
import hfield_ref
from helpers import D, set_opt
from mujoco_sim_amd.engine import MjhError

HFIELD, SPHERE, CAPSULE, BOX, PLANE = 1, 2, 3, 6, 0


def _terrain(lib, elev, nrow, ncol, size=(1.0, 1.0, 0.5, 0.2), others=((SPHERE, (0.1, 0, 0)),), pos=None, quat=None,
             static_body=False, capacity=None, plane=False):
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002)
    if capacity:
        lib.mjh_builder_set_capacity(b, *capacity)
    e = None if elev is None else (C.c_double * len(elev))(*elev)
    h = lib.mjh_builder_add_hfield(b, b"terrain", nrow, ncol, D(*size), e)
    assert h == 0
    body = lib.mjh_builder_add_body(b, b"ground", 0, D(0, 0, 0), None, 0.0) if static_body else 0
    g = lib.mjh_builder_add_hfield_geom(b, b"hf", body, h, D(*pos) if pos else None, D(*quat) if quat else None, None, -1, -1, -1)
    assert g >= 0, lib.mjh_last_error()
    if plane:
        lib.mjh_builder_add_geom(b, b"floor", 0, PLANE, D(0, 0, 1), D(0, 0, -1), None, None, -1, -1, -1, -1)
    for k, (t, s) in enumerate(others):
        bd = lib.mjh_builder_add_body(b, b"o%d" % k, 0, D(0.1 * k, 0, 0.6), None, 0.0)
        lib.mjh_builder_add_joint(b, b"j%d" % k, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        lib.mjh_builder_add_geom(b, b"g%d" % k, bd, t, D(*s), None, None, None, -1, -1, -1, -1)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    return m


def test_builder_tables_normalisation_and_rbound(lib):
    elev = [2.0, 3.0, 4.0, 2.0, 6.0, 2.0]            # 2 x 3, min 2, max 6
    m = _terrain(lib, elev, 2, 3, size=(1.5, 0.5, 0.3, 0.1))
    assert m.nhfield == 1 and m.nhfielddata == 6
    assert list(m.array("hfield_nrow")) == [2] and list(m.array("hfield_ncol")) == [3] and list(m.array("hfield_adr")) == [0]
    np.testing.assert_allclose(m.array("hfield_size"), [1.5, 0.5, 0.3, 0.1])
    np.testing.assert_allclose(m.array("hfield_data"), (np.array(elev) - 2) / 4)
    assert m.c.hfield_names[0] == b"terrain"
    g = m.name2id(2, "hf")
    assert m.array("geom_type")[g] == HFIELD and m.array("geom_dataid")[g] == 0
    assert m.array("geom_rbound")[g] == pytest.approx(np.sqrt(1.5 ** 2 + 0.5 ** 2 + 0.3 ** 2))
    # flat field: all zeros after normalisation (no division by a zero range)
    m2 = _terrain(lib, [0.7] * 4, 2, 2)
    np.testing.assert_array_equal(m2.array("hfield_data"), np.zeros(4))
    m3 = _terrain(lib, None, 3, 3, size=(1, 1, 0.1, 0.5))     # NULL elevation: zeros; base above elevation sets the bound
    np.testing.assert_array_equal(m3.array("hfield_data"), np.zeros(9))
    assert m3.array("geom_rbound")[m3.name2id(2, "hf")] == pytest.approx(np.sqrt(2 + 0.25))


def test_builder_checks(lib):
    b = lib.mjh_builder_create()
    try:
        assert lib.mjh_builder_add_hfield(b, b"a", 1, 3, D(1, 1, 1, 1), None) == -1      # MJH_ERR_ARG
        assert lib.mjh_builder_add_hfield(b, b"a", 3, 1, D(1, 1, 1, 1), None) < 0
        for bad in [(0, 1, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)]:
            assert lib.mjh_builder_add_hfield(b, b"a", 2, 2, D(*bad), None) < 0
            assert "size" in lib.mjh_last_error().decode()
        h = lib.mjh_builder_add_hfield(b, b"ok", 2, 2, D(1, 1, 1, 1), None)
        assert h == 0
        assert lib.mjh_builder_add_hfield_geom(b, b"x", 0, 5, None, None, None, -1, -1, -1) < 0      # bad hfield id
        bd = lib.mjh_builder_add_body(b, b"moving", 0, D(0, 0, 1), None, 0.0)
        lib.mjh_builder_add_joint(b, b"j", bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_hfield_geom(b, b"x", bd, h, None, None, None, -1, -1, -1) == -5    # MJH_ERR_UNSUPPORTED
        assert "static" in lib.mjh_last_error().decode()
    finally:
        lib.mjh_builder_destroy(b)


def test_pair_rules_and_capacity(lib):
    others = ((SPHERE, (0.1, 0, 0)), (BOX, (0.1, 0.1, 0.1)), (CAPSULE, (0.05, 0.1, 0)))
    m = _terrain(lib, [0, 1, 2, 3], 2, 2, others=others, plane=True)
    g1, g2 = m.array("pair_geom1"), m.array("pair_geom2")
    types = m.array("geom_type")
    hf = m.name2id(2, "hf")
    hpairs = [(a, b) for a, b in zip(g1, g2) if hf in (a, b)]
    assert len(hpairs) == 3 and all(a == hf for a, b in hpairs)                    # hfield is geom1; no plane-hfield pair
    assert not any(types[a] == PLANE and types[b] == HFIELD for a, b in zip(g1, g2))
    # capacity: 50 per hfield pair, plane-box 4, box-box / sphere-x 1 ..., rows at condim 3 = 4 per contact
    caps = {(PLANE, SPHERE): 1, (PLANE, BOX): 4, (PLANE, CAPSULE): 2, (SPHERE, BOX): 1, (SPHERE, CAPSULE): 1, (CAPSULE, BOX): 1}
    want = 0
    for a, b in zip(g1, g2):
        ta, tb = sorted((types[a], types[b]))
        want += 50 if ta == HFIELD else caps[(ta, tb)]
    assert m.maxcon == want and m.c.maxefc == 4 * want
    # the raw staging of 50 contacts per hfield pair is part of the LDS plan
    buf = C.create_string_buffer(1 << 16)
    assert lib.mjh_debug_lds_layout(m.ptr, buf, len(buf)) >= 0
    nstage = int(buf.value.decode().split("nstage ")[1].split()[0])
    assert nstage == want
    m0 = _terrain(lib, [0, 1, 2, 3], 2, 2, others=others, plane=True, capacity=(20, 0))
    assert m0.maxcon == 20
    # (the full capacity takes the many-body layout, pools in global memory; at 20 contacts the staging of all three pairs,
    #  7 floats per raw contact, stays in the LDS-resident layout)
    assert lib.mjh_query_lds_bytes(m.ptr) > 0 and lib.mjh_query_lds_bytes(m0.ptr) >= want * 7 * 4
    # hfield on a static child body: fine; replicate: refused
    m1 = _terrain(lib, [0, 1, 2, 3], 2, 2, static_body=True)
    assert m1.npair == 1
    assert not lib.mjh_model_replicate(m1.ptr, 2)
    assert "height field" in lib.mjh_last_error().decode()


def test_add_geom_hfield_keeps_no_pairs(lib):
    b = lib.mjh_builder_create()
    lib.mjh_builder_add_geom(b, b"hf", 0, HFIELD, D(1, 1, 1), None, None, None, -1, -1, -1, -1)
    bd = lib.mjh_builder_add_body(b, b"o", 0, D(0, 0, 1), None, 0.0)
    lib.mjh_builder_add_joint(b, b"j", bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"s", bd, SPHERE, D(0.1, 0, 0), None, None, None, -1, -1, -1, -1)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    assert m.npair == 0 and m.nhfield == 0


_XML = """<mujoco>
  <option timestep="0.002"/>
  <default><default class="terrain"><geom friction="0.7 0.01 0.001" condim="4"/></default></default>
  <asset>
    <hfield name="bumps" nrow="3" ncol="4" size="2 1 0.4 0.1" elevation="1 2 3 4  5 6 7 8  9 10 11 13"/>
    %s
  </asset>
  <worldbody>
    <geom name="ground" type="hfield" hfield="bumps" class="terrain" pos="0.5 0 0" size="9 9 9"/>
    %s
    <body name="ball" pos="0 0 1"><freejoint/><geom type="sphere" size="0.1"/></body>
  </worldbody>
</mujoco>"""


def test_loader_inline(lib):
    m = ms.load_mjcf(_XML % ("", ""))
    assert m.nhfield == 1 and m.npair == 1
    g = m.name2id(2, "ground")
    assert m.array("geom_type")[g] == HFIELD and m.array("geom_dataid")[g] == 0
    np.testing.assert_allclose(m.array("hfield_size"), [2, 1, 0.4, 0.1])
    np.testing.assert_allclose(m.array("hfield_data"), (np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13]) - 1) / 12)
    np.testing.assert_allclose(m.array("geom_friction")[3 * g:3 * g + 3], [0.7, 0.01, 0.001])   # default class applied
    assert m.array("geom_condim")[g] == 4
    np.testing.assert_allclose(m.array("geom_pos")[3 * g:3 * g + 3], [0.5, 0, 0])
    assert m.array("geom_rbound")[g] == pytest.approx(np.sqrt(4 + 1 + 0.16))                     # the geom's size is ignored
    assert "hfield" not in m.note


def test_loader_binary_file_and_png(lib, tmp_path):
    data = np.arange(6, dtype=np.float32) * 0.5
    (tmp_path / "t.bin").write_bytes(struct.pack("<ii", 2, 3) + data.tobytes())
    (tmp_path / "img.png").write_bytes(b"\x89PNG\r\n\x1a\n")
    assets = '<hfield name="file" file="t.bin" size="1 1 0.2 0.05"/><hfield name="pic" file="img.png" size="1 1 1 1"/>'
    geoms = '<geom name="g2" type="hfield" hfield="file"/><geom name="g3" type="hfield" hfield="pic"/>'
    p = tmp_path / "scene.xml"
    p.write_text(_XML % (assets, geoms))
    m = ms.load_mjcf(path=str(p))
    assert m.nhfield == 2 and m.nhfielddata == 12 + 6
    assert list(m.array("hfield_nrow")) == [3, 2] and list(m.array("hfield_ncol")) == [4, 3]
    np.testing.assert_allclose(m.array("hfield_data")[12:], data / data.max(), rtol=1e-7)
    assert m.name2id(2, "g3") < 0 and m.name2id(2, "g2") >= 0
    assert "pic not loaded (PNG" in m.note and "skipped hfield geom (hfield pic" in m.note
    assert m.npair == 2


def test_loader_errors(lib, tmp_path):
    bad = _XML.replace('size="2 1 0.4 0.1"', 'size="2 1 0 0.1"') % ("", "")
    with pytest.raises(MjhError, match="size"):
        ms.load_mjcf(bad)
    for elev in ("1 2 3", "1 2 3 4 5 6 7 8 9 10 11 12 13"):        # too few, too many (nrow * ncol = 12)
        with pytest.raises(MjhError, match="nrow\\*ncol"):
            ms.load_mjcf(_XML.replace('elevation="1 2 3 4  5 6 7 8  9 10 11 13"', 'elevation="%s"' % elev) % ("", ""))
    moving = (_XML % ("", "")).replace("<freejoint/><geom type=\"sphere\" size=\"0.1\"/>",
                                        "<freejoint/><geom type=\"sphere\" size=\"0.1\"/><geom type=\"hfield\" hfield=\"bumps\"/>")
    with pytest.raises(MjhError, match="static"):
        ms.load_mjcf(moving)
    (tmp_path / "short.bin").write_bytes(struct.pack("<ii", 4, 4) + b"\0" * 8)
    p = tmp_path / "s.xml"
    p.write_text(_XML % ('<hfield name="f" file="short.bin" size="1 1 1 1"/>', ""))
    with pytest.raises(MjhError, match="binary height field"):
        ms.load_mjcf(path=str(p))


# ---- the reference of the prism narrow phase on hand-made cases

def _poses(m, placements):
    """world poses [ngeom, 3], [ngeom, 9]: geoms of the world at their model pose, others as given {geom: (pos, mat)}"""
    ng = m.ngeom
    gpos, gmat = np.zeros((ng, 3)), np.tile(np.eye(3).ravel(), (ng, 1))
    gp, gq = m.array("geom_pos").reshape(ng, 3), m.array("geom_quat").reshape(ng, 4)
    for g in range(ng):
        gpos[g] = gp[g]
        w, x, y, z = gq[g]
        gmat[g] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]).ravel()
    for g, (p, R) in placements.items():
        gpos[g] = p; gmat[g] = np.asarray(R, float).ravel()
    return gpos, gmat


def test_reference_sphere_over_one_triangle(lib):
    # 2 x 2 grid = one cell, tilted plane z = 0.1 + 0.1 x (the data normalised to [0, 1] then scaled by size[2] = 0.2)
    m = _terrain(lib, [0, 1, 0, 1], 2, 2, size=(1, 1, 0.2, 0.5))
    hf, s = m.name2id(2, "hf"), m.name2id(2, "g0")
    r = 0.1
    # a sphere above the point (-0.5, 0.3), interior of the second triangle ((0,0), (1,1), (1,0)), centre 0.09 above the surface
    x, y = -0.5, 0.3
    zs = 0.1 + 0.1 * x
    n = np.array([-0.1, 0, 1]) / np.sqrt(1.01)
    centre = np.array([x, y, zs]) + 0.09 * n
    gpos, gmat = _poses(m, {s: (centre, np.eye(3))})
    c = hfield_ref.expected_contacts(m, hf, s, gpos, gmat)
    assert len(c) == 1 and c[0]["prism"] == (0, 0, 1)
    assert c[0]["dist"] == pytest.approx(0.09 - r, abs=1e-6)          # (the portal refinement stops within its tolerance)
    np.testing.assert_allclose(c[0]["normal"], n, atol=1e-4)
    assert hfield_ref.expected_contacts(m, hf, s, *_poses(m, {s: (centre + 0.2 * n, np.eye(3))})) == []


def test_reference_box_over_patch(lib):
    # flat 5 x 5 field over [-1, 1]^2 (cells 0.5 wide), a flat box resting 1 mm into it over a 3 x 3 block of cells
    m = _terrain(lib, None, 5, 5, size=(1, 1, 0.3, 0.2), others=((BOX, (0.35, 0.35, 0.05)),))
    hf, bx = m.name2id(2, "hf"), m.name2id(2, "g0")
    gpos, gmat = _poses(m, {bx: ((-0.25, 0.25, 0.049), np.eye(3))})
    nrow, ncol, size, data = hfield_ref.hfield_of(m, hf)
    lp = gpos[bx] - gpos[hf]
    pr = hfield_ref.prisms(nrow, ncol, size, data, lp, m.array("geom_rbound")[bx], 0.0)
    # bounding radius 0.497 about (-0.25, 0.25): x in [-0.747, 0.247] -> cells 0..2, the same in y -> 3 x 3 cells, 18 prisms
    assert len(pr) == 18 and [p[:3] for p in pr[:4]] == [(1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
    c = hfield_ref.expected_contacts(m, hf, bx, gpos, gmat)
    assert 1 <= len(c) <= 18
    for x in c:
        assert x["dist"] == pytest.approx(-0.001, abs=1e-6)
        np.testing.assert_allclose(x["normal"], [0, 0, 1], atol=1e-6)
    assert [x["prism"] for x in c] == sorted(x["prism"] for x in c)


def test_reference_large_box_capped(lib):
    m = _terrain(lib, None, 12, 12, size=(1, 1, 0.3, 0.2), others=((BOX, (0.8, 0.8, 0.05)),))
    hf, bx = m.name2id(2, "hf"), m.name2id(2, "g0")
    gpos, gmat = _poses(m, {bx: ((0.0, 0.0, 0.045), np.eye(3))})
    c = hfield_ref.expected_contacts(m, hf, bx, gpos, gmat)
    full = hfield_ref.expected_contacts(m, hf, bx, gpos, gmat, maxcon=10 ** 6)
    assert len(full) > 50 and len(c) == 50 and [x["prism"] for x in c] == [x["prism"] for x in full[:50]]
