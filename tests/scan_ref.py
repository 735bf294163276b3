"""Lidar scan patterns and their beams in numpy fp64, shared by tests/test_scan_host.py (the kernel's pattern code on the CPU) and
tests/test_gpu_scan.py (the kernel).  A pattern is (width, height, azimuth0, azimuth_step, elevation) with elevation a tuple
(elevation0, elevation_step) or an array of `height` angles; radians."""
import numpy as np

DEG = np.pi / 180.0

# an unordered 9-row table (a real lidar's rows are neither uniform nor sorted), with rows near both poles
TABLE9 = np.array([2.0, -80.0, 15.5, -1.0, 80.0, -30.25, 45.0, 0.0, -11.0]) * DEG

PATTERNS = {
    "1x1": (1, 1, -0.05, 0.0, (0.01, 0.0)),
    "planar 1x1081": (1081, 1, -135.0 * DEG, 0.25 * DEG, (0.0, 0.0)),
    "full turn 16x360": (360, 16, -np.pi, 2 * np.pi / 360, (-15.0 * DEG, 2.0 * DEG)),
    "5x3": (3, 5, -0.4, 0.35, (-0.5, 0.25)),
    "9x70": (70, 9, -1.9, 0.055, (-0.6, 0.13)),
    "table 9x70": (70, 9, -np.pi, 2 * np.pi / 70, TABLE9),
}

# further patterns of the cone test alone: rows at +-89 degrees; three columns 120 degrees apart (the tile spans more than pi: no cone,
# everything is kept); tiles whose azimuth half-span is just below pi/2
CONE_PATTERNS = dict(PATTERNS, **{
    "poles 4x100": (100, 4, -np.pi, 2 * np.pi / 100, np.array([-89.0, -30.0, 30.0, 89.0]) * DEG),
    "poles 2x40": (40, 2, 0.1, -2 * np.pi / 40, np.array([89.0, -89.0]) * DEG),
    "3 columns 120 degrees": (3, 5, -np.pi, 2 * np.pi / 3, (-0.5, 0.25)),
    "wide 8x8": (8, 8, -1.5, 25.0 * DEG, (-60.0 * DEG, 120.0 / 7 * DEG)),
    "wide 1x130": (130, 1, 0.0, 2.8 * DEG, (0.3, 0.0)),
})


def angles(pattern):
    """(azimuth [width], elevation [height]) in fp64, as the interface defines them"""
    width, height, az0, step, el = pattern
    az = az0 + np.arange(width) * step
    return az, (el[0] + np.arange(height) * el[1] if isinstance(el, tuple) else np.asarray(el, float))


def beams64(pattern):
    """[height, width, 3]: d = (cos el cos az, cos el sin az, sin el) in the sensor frame"""
    az, el = angles(pattern)
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    return np.stack([ce * np.cos(az)[None, :], ce * np.sin(az)[None, :], se * np.ones((1, len(az)))], axis=-1)


def tile_shape(height):
    """(TH, TW): TH the smallest power of two >= min(height, 8), TH TW = 64"""
    th = 1
    while th < min(height, 8):
        th *= 2
    return th, 64 // th


def scan_kwargs(pattern):
    """the pattern as Engine.scan's arguments"""
    width, height, az0, step, el = pattern
    return dict(width=width, height=height, azimuth=(az0, step), elevation=el)
