"""The reference project's model files the CPU tests read (robot MJCF, C1 / C5 worlds, the floor, their mesh assets), written out
once per process from tests/golden/reference_models.npz (tests/golden/make_reference_models.py) as a model/ tree:
model_dir() is the directory that holds test/ and world/."""
import atexit
import os
import shutil
import tempfile

import numpy as np

_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_models.npz")
_DIR = None


def _stl(vert, tri):
    """binary STL of the triangles vert[tri]: zero header, zero normals, zero attribute"""
    n = len(tri)
    rec = np.zeros((n, 50), np.uint8)
    rec[:, 12:48] = np.ascontiguousarray(vert[tri.astype(np.int64)].reshape(n, 9), "<f4").view(np.uint8)
    return bytes(80) + np.array([n], "<u4").tobytes() + rec.tobytes()


def model_dir():
    global _DIR
    if _DIR is None:
        root = tempfile.mkdtemp(prefix="mjh_refmodels_")
        atexit.register(shutil.rmtree, root, True)
        z = np.load(_FIXTURE)
        k = 0
        while f"path_{k}" in z.files:
            path = os.path.join(root, z[f"path_{k}"].tobytes().decode())
            os.makedirs(os.path.dirname(path), exist_ok=True)
            data = z[f"raw_{k}"].tobytes() if f"raw_{k}" in z.files else _stl(z[f"vert_{k}"], z[f"tri_{k}"])
            with open(path, "wb") as f:
                f.write(data)
            k += 1
        _DIR = root
    return _DIR
