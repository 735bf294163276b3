"""The comparison of one env's distances / image with the fp64 references on the robust rays, shared by tests/test_gpu_depth.py (the
depth kernel) and tests/test_ray_host.py (the kernels' shared code on the CPU)."""
import numpy as np

import ray_mesh_ref as rm

TOL = 5e-5
CAP = 0.02


def check(name, depth, gid, scene, rays, scale=None, cutoff=0.0):
    """ONE env's image against the reference on the robust pixels; returns (largest scaled error, non-robust share)"""
    depth = depth.reshape(-1).astype(float); gid = gid.reshape(-1)
    ref_d, ref_g = rm.cast(rays[0], rays[1], scene)
    if scale is not None:
        ref_d = np.where(ref_g >= 0, ref_d * scale, ref_d)
    if cutoff > 0:
        far = ref_d > cutoff
        ref_d = np.where(far, -1.0, ref_d); ref_g = np.where(far, -1, ref_g)
    rob = rm.robust(rays, scene)
    share = 1.0 - rob.mean()
    hit = rob & (ref_g >= 0)
    err = np.abs(depth - ref_d) / np.maximum(1.0, np.abs(ref_d))
    worst = float(err[hit].max()) if hit.any() else 0.0
    print(f"{name}: {len(rob)} pixels, non-robust share {share:.4f}, hits {int(hit.sum())}, max scaled error {worst:.3e}")
    assert share <= CAP, name
    assert (gid[rob] == ref_g[rob]).all(), name
    assert (depth[rob & (ref_g < 0)] == -1.0).all() and (depth[gid < 0] == -1.0).all(), name
    assert worst <= TOL, name
    return worst, share
