"""Height-scan grids and their rays in numpy fp64, shared by tests/test_heightscan_host.py (the kernel's grid code on the CPU) and
tests/test_gpu_heightscan.py (the kernel).  A grid is (width, height, (spacing_x, spacing_y), (offset_x, offset_y), above); a pose
is (o [3], S [3, 3]) with world = S local; align is "yaw", "base" or "world".  Nothing here is shared with the kernel's code."""
import numpy as np

ALIGNS = ("yaw", "base", "world")
ALIGN_ID = {"yaw": 0, "base": 1, "world": 2}
DEGENERATE = 1e-6      # squared length of the projected x axis below which a YAW grid has no heading

# the grids of the tests: partial tiles in both directions (41 x 23, 9 x 70), a single row (1 x 64 tiles), fewer rows than a tile
# (5 x 3: 4 x 16 tiles), one cell; offsets that move the grid off the sensor
GRIDS = {
    "41x23": (41, 23, (0.11, 0.07), (0.0, 0.0), 0.5),
    "130x1": (130, 1, (0.033, 0.1), (0.05, -0.4), 0.5),
    "9x70": (9, 70, (0.45, 0.03), (0.0, 0.0), 0.5),
    "5x3": (5, 3, (0.3, 0.25), (0.8, 0.3), 0.5),
    "1x1": (1, 1, (0.1, 0.1), (0.0, 0.0), 0.5),
}


def grid_frame(S, align):
    """G [3, 3], columns gx, gy, gz in the world"""
    S = np.asarray(S, float).reshape(3, 3)
    if align == "base":
        return S.copy()
    if align == "world":
        return np.eye(3)
    assert align == "yaw"
    px, py = S[0, 0], S[1, 0]      # the site's x axis is S's first column
    l2 = px * px + py * py
    gx = np.array([1.0, 0.0, 0.0]) if l2 < DEGENERATE else np.array([px, py, 0.0]) / np.sqrt(l2)
    gz = np.array([0.0, 0.0, 1.0])
    return np.stack([gx, np.cross(gz, gx), gz], axis=1)


def cells(grid):
    """(x [width], y [height]) in the grid frame"""
    width, height, spacing, offset, _ = grid
    return (offset[0] + (np.arange(width) - (width - 1) / 2) * spacing[0], offset[1] + (np.arange(height) - (height - 1) / 2) * spacing[1])


def rays64(pose, grid, align):
    """world-frame (origins [height width, 3], unit directions [height width, 3]) of the grid's rays, row-major (row i, column j)"""
    o, S = pose
    G = grid_frame(S, align)
    x, y = cells(grid)
    X, Y = np.meshgrid(x, y)      # [height, width]
    P = np.asarray(o, float) + X[..., None] * G[:, 0] + Y[..., None] * G[:, 1] + grid[4] * G[:, 2]
    return P.reshape(-1, 3), np.tile(-G[:, 2], (P.shape[0] * P.shape[1], 1))


def points64(grid, rng_, gid):
    """[..., height, width, 3]: (x_j, y_i, above - range), a miss with range 0, from the device's range / geom-id images"""
    x, y = cells(grid)
    X, Y = np.meshgrid(x, y)
    r = np.where(gid < 0, 0.0, rng_.astype(float))
    return np.stack([np.broadcast_to(X, r.shape), np.broadcast_to(Y, r.shape), grid[4] - r], axis=-1)


def tile_shape(height):
    """(TH, TW): TH the smallest power of two >= min(height, 8), TH TW = 64"""
    th = 1
    while th < min(height, 8):
        th *= 2
    return th, 64 // th


def kwargs(grid):
    """the grid as Engine.height_scan's arguments"""
    width, height, spacing, offset, above = grid
    return dict(width=width, height=height, spacing=spacing, offset=offset, above=above)
