"""Packs the reference's model files that the CPU tests read (MJCF text under model/test and model/world, the STL / OBJ mesh
assets they name) into ONE fixture, tests/golden/reference_models.npz, so that those tests run from a clean checkout on any
machine.  MJCF text and ASCII meshes are stored byte for byte; a binary STL as its distinct float32 vertices plus a triangle
index, which tests/refmodels.py writes back as a binary STL with the same vertex values in the same order (normals and the
80-byte header are not read by any loader here).  The model files are those of HoangGiang93/mujoco_sim (MIT licence).

    python tests/golden/make_reference_models.py <checkout of the reference project>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_models.npz")
# the files the tests load: every robot of tests/test_independent_mjcf.py / test_robot_fixtures.py, C1 / C5's worlds, the floor
XML = ["test/pendulum.xml", "test/bowl.xml", "test/pr2/pr2.xml", "test/tiago/tiago.xml", "test/hsrb4s/hsrb4s.xml",
       "test/ridgeback_panda/ridgeback_panda.xml", "test/armar/armar6.xml", "world/empty.xml"]


def mesh_files(model_dir, xml):
    """relative paths of the mesh assets an MJCF file names (compiler meshdir, then the file attribute)"""
    import xml.etree.ElementTree as ET
    root = ET.parse(os.path.join(model_dir, xml)).getroot()
    comp = root.find("compiler")
    meshdir = (comp.get("meshdir") if comp is not None else None) or ""
    out = []
    for a in root.findall("asset"):
        for m in a.findall("mesh"):
            if m.get("file"):
                out.append(os.path.normpath(os.path.join(os.path.dirname(xml), meshdir, m.get("file"))))
    return out


def is_binary_stl(data):
    if data[:5] == b"solid" and b"facet" in data[:1029]:
        return False
    return len(data) >= 84 and len(data) == 84 + 50 * int(np.frombuffer(data[80:84], "<u4")[0])


def main(ref_root):
    model_dir = os.path.join(ref_root, "model")
    files = list(XML)
    for x in XML:
        files += mesh_files(model_dir, x)
    z = {}
    for k, rel in enumerate(sorted(set(files))):
        data = open(os.path.join(model_dir, rel), "rb").read()
        z[f"path_{k}"] = np.frombuffer(rel.encode(), np.uint8)
        if rel.lower().endswith(".stl") and is_binary_stl(data):
            n = int(np.frombuffer(data[80:84], "<u4")[0])
            tri = np.frombuffer(data[84:], np.uint8).reshape(n, 50)[:, 12:48].copy().view("<f4").reshape(n * 3, 3)
            # distinct vertices by their bit pattern (-0.0 and 0.0 stay apart: the file's exact values come back)
            vert, index = np.unique(tri.view(np.uint32), axis=0, return_inverse=True)
            z[f"vert_{k}"] = vert.view("<f4")
            z[f"tri_{k}"] = index.reshape(n, 3).astype(np.uint16 if len(vert) < 65536 else np.uint32)
        else:
            z[f"raw_{k}"] = np.frombuffer(data, np.uint8)
    np.savez_compressed(OUT, **z)
    print(f"{OUT}: {len(set(files))} files, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
