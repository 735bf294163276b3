"""LDS budget of the assemble-only launch of a patch model's window chain (engine.hip: derive_device_model, DWpre; step_kernel.h: WPRE
instance 1).  S24's assemble workgroup must fit 13 LDS granules of 1280 B, so that one cohort of the headline (1365 workgroups) is resident
beside the other cohorts' window wavefronts at once (profiles/assemble_round_summary.md); the fused kernel's layout, and with it every other
instance, stays exactly as it was.  No device needed: the layout report (mjh_debug_lds_layout) is host code.

MJH_WPRE_SLIM3 is read once per process, so every report comes from a child process of its own."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

# The layout reports of the commit before this change (mjh_debug_lds_layout: float offsets, then the totals), taken from that commit's library.
PARENT = {
    "s24": "qpos 0 qvel 28 qvref 52 ws 76 qacc 100 smooth 124 asmooth 148 passive 172 bias 196 applied 220 tmpv 244 tmpv2 268 xpos 488 xquat 504 xmat 524 xipos 756 ximat 572 com 772 cinert 484 crb 484 cvel 484 cacc 484 cfrc 484 cfrcsub 484 xanchor 620 xaxis 632 cdof 484 cdofdot 484 qM 292 qLD 292 qLDinv 376 gpos 644 gmat 672 zero 464 dofpar 0 dofMadr 0 anc 0 p_gsize 400 p_rbound 428 p_mass 440 p_inertia 448 site 0 fext 0 con 788 blki 1428 blkf 1588 blkq 788 bv 2228 phi 2388 sched 2548 order 2228 J 2628 B 2628 ext 484 total 5120 lds_bytes 20480 lds_bytes_pre 18192 k1_floats 272 maxcon 40 maxblk 40 rowW 12 nstage 192 big 0",
    "s24pen96": "qpos 0 qvel 28 qvref 52 ws 76 qacc 100 smooth 124 asmooth 148 passive 172 bias 196 applied 220 tmpv 244 tmpv2 268 xpos 296 xquat 312 xmat 332 xipos 564 ximat 380 com 580 cinert 292 crb 292 cvel 292 cacc 292 cfrc 292 cfrcsub 292 xanchor 428 xaxis 440 cdof 292 cdofdot 292 qM 596 qLD 596 qLDinv 680 gpos 452 gmat 480 zero 10944 dofpar 0 dofMadr 0 anc 0 p_gsize 704 p_rbound 732 p_mass 744 p_inertia 752 site 0 fext 0 con 768 blki 2304 blkf 2688 blkq 768 bv 4224 phi 4608 sched 4992 order 4224 J 6336 B 6336 ext 5184 total 10948 lds_bytes 43792 lds_bytes_pre 16896 k1_floats 272 maxcon 96 maxblk 96 rowW 12 nstage 192 big 0",
    "arm7": "qpos 0 qvel 8 qvref 16 ws 24 qacc 32 smooth 40 asmooth 48 passive 56 bias 64 applied 72 tmpv 80 tmpv2 88 xpos 96 xquat 120 xmat 152 xipos 520 ximat 224 com 544 cinert 568 crb 296 cvel 832 cacc 880 cfrc 928 cfrcsub 976 xanchor 376 xaxis 400 cdof 648 cdofdot 1024 qM 692 qLD 720 qLDinv 748 gpos 424 gmat 448 zero 1420 dofpar 756 dofMadr 764 anc 772 p_gsize 424 p_rbound 448 p_mass 800 p_inertia 808 site 0 fext 0 con 832 blki 1068 blkf 1100 blkq 832 bv 96 phi 128 sched 1228 order 96 J 1244 B 1332 ext 96 total 1424 lds_bytes 5696 lds_bytes_pre 5680 k1_floats 424 maxcon 1 maxblk 8 rowW 8 nstage 0 big 0",
}
PARENT_S24_ASSEMBLE_BYTES = 18192      # lds_bytes_pre of the s24 report above: the parent commit's value, which its launch allocated (tests/test_abi.py pins it)
# The report of this commit ends with one more line, `lds_bytes_wpre`: what the assemble-only launch of the window chain allocates.  The lines
# before it (every offset, lds_bytes and lds_bytes_pre, which mjh_query_lds_bytes_assemble returns: that launch's extent in the fused layout's
# offsets) are the parent's.
GRANULE = 1280

_SCRIPT = r"""
import ctypes as C, json, sys
sys.path.insert(0, {root!r})
import mujoco_sim_amd as ms
lib = ms.capi.load()
def report(m):
    buf = C.create_string_buffer(8192)
    assert lib.mjh_debug_lds_layout(m.ptr, buf, 8192) > 0
    return dict(text=" ".join(buf.value.decode().split()), assemble=lib.mjh_query_lds_bytes_assemble(m.ptr), full=lib.mjh_query_lds_bytes(m.ptr))
print(json.dumps(dict(s24=report(ms.scene("s24")), s24pen96=report(ms.scene("s24pen", 0.175, 96)), arm7=report(ms.scene("arm7", 1)))))
"""


def _reports(slim3):
    env = dict(os.environ)
    env.pop("MJH_WPRE_SLIM3", None); env.pop("MJH_WPRE_SLIM2", None); env.pop("MJH_LDS_PAD", None)
    if slim3 is not None:
        env["MJH_WPRE_SLIM3"] = str(slim3)
    r = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _kv(text):
    w = text.split()
    return dict(zip(w[0::2], map(int, w[1::2])))


@pytest.fixture(scope="module")
def new():
    return _reports(None)


@pytest.fixture(scope="module")
def former():
    return _reports(0)


def _split(text):
    """(the parent's part of a report, lds_bytes_wpre)"""
    head, key, val = text.rpartition(" lds_bytes_wpre ")
    assert key, text
    return head, int(val)


def test_s24_assemble_only_extent_fits_13_granules(new):
    head, wpre = _split(new["s24"]["text"])
    L = _kv(head)
    assert 0 < wpre <= 13 * GRANULE, wpre
    assert wpre < L["lds_bytes_pre"] == new["s24"]["assemble"], "the query keeps the extent in the fused layout's offsets: an upper bound"
    # what the launch keeps: the contact records (bv / phi live there), the block tables and a base-row pool of the fused layout's size behind them
    jsz = _kv(PARENT["s24"])["lds_bytes_pre"] // 4 - _kv(PARENT["s24"])["J"]
    assert wpre == 4 * (L["blkf"] + 16 * L["maxblk"] + jsz)
    assert 8 * L["maxblk"] <= 16 * L["maxcon"], "bv and phi (4 floats per block each) fit the contact records (16 floats per contact)"


def test_knob_restores_the_parents_extent(former):
    assert _split(former["s24"]["text"])[1] == former["s24"]["assemble"] == PARENT_S24_ASSEMBLE_BYTES
    for name in PARENT:
        head, wpre = _split(former[name]["text"])
        assert head == PARENT[name], name
        assert wpre == former[name]["assemble"] == (_kv(PARENT[name])["lds_bytes_pre"] if name != "arm7" else 0), name          # (arm7 does not take the window chain)


@pytest.mark.parametrize("name", ["s24", "s24pen96", "arm7"])
def test_fused_layout_and_other_instances_unchanged(new, name):
    """lds_bytes and every array offset (what the fused kernel and every instance but the patch models' assemble-only one read) equal the
    parent's; for s24pen at capacity 96 (assemble-only instance 2) and arm7 what the assemble-only launch allocates as well."""
    head, wpre = _split(new[name]["text"])
    assert head == PARENT[name]
    assert new[name]["full"] == _kv(PARENT[name])["lds_bytes"]
    if name != "s24":
        assert wpre == new[name]["assemble"] == (_kv(PARENT[name])["lds_bytes_pre"] if name != "arm7" else 0)
