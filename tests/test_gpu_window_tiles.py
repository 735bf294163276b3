"""GPU test of csrc/window_tiles.h: the tile rows of the window kernel built on the matrix cores are, bit for bit, what the broadcast
multiply-add loop gives.

tests/window_tiles/tiles_check.hip is a stand-alone program (its own `main`) that instantiates the header's primitive both ways —
v_mfma_f32_16x16x1_4b_f32 plus the 4 x 4 transpose by lane swaps, and the v_fmac_f32_dpp row_newbcast loop — runs one wavefront per case and
compares every result of the two, and of each against the k-ordered fmaf chain computed on the host, as bit patterns.  It is compiled here
and run as a child process under a time limit.  Its cases: rows expanded as wn_load_row expands hand-over rows (at most two body slots of six
out of 24, zeros elsewhere, some entries -0), at S24's magnitude; scaled so that products and partial sums are subnormal, and so that they
reach FLT_MAX / 24; one, two and three lane groups all zero; a last window of 1 and of 15 live rows; A != B (the cross tile) and the 64-row
form's use (A the same in all four lane groups); and one case whose exact integer results name the lane and register they belong to, which
pins the layout of the MFMA's result: register 4 b + c of lane 16 h + j holds block b, row 4 h + c, column j."""
import os
import subprocess

import pytest

import hostbuild

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "window_tiles", "tiles_check.hip")
CSRC = os.path.join(ROOT, "mujoco_sim_amd", "csrc")


def test_matrix_core_tiles_are_bitwise_the_broadcast_loops(tmp_path):
    exe = str(tmp_path / "tiles_check")
    subprocess.check_call([hostbuild.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    diffs = [l for l in r.stdout.splitlines() if l.startswith(("DIFF", "  layout"))]
    assert r.returncode == 0, f"exit status {r.returncode}; " + ("\n".join(diffs) if diffs else r.stderr[-2000:])
    assert "IDENTICAL" in r.stdout
    assert "matrix cores vs broadcast multiply-adds: 0 of" in r.stdout
