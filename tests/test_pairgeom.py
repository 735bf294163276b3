"""The oracle's analytic narrow-phase pairs (plane-{sphere, capsule, cylinder, ellipsoid, box, mesh}, sphere-sphere, sphere-capsule,
capsule-capsule, sphere-box) against geometry that shares nothing with them: tests/pairgeom.py.  The device runs the same families
in tests/test_gpu_pairs.py, the device's routines compiled for the host in tests/test_collide_host.py.  No GPU.

One small model per pair type (a static plane — horizontal, or tilted — or one free body, plus one free body; per-case geom sizes
through the env parameters), 2000 cases per family, `kinematics` + `collision`, the reference geoms from the oracle's own geom poses:
only the narrow phase is under test.

Tolerance 1e-9 (coordinates below 1 m, fp64 arithmetic), measured against pairgeom, never against the oracle itself.  Measured
worst (the smallest tolerance of a half-decade ladder from 1e-9 at which every robust case of the family passes): the first rung
in eight families.  Two need more and have a bound of their own, the measured worst times three:
  * capsule_capsule passes from 1e-7 (fails at 3.2e-8), bound 3e-7: axes a few 1e-6 rad apart sit just above the routine's
    `|det| < 1e-12` parallel switch, where x1, x2 = (rounding of det) / det leave the closest points that far apart along the axes
  * plane_cylinder passes from 1e-6 (fails at 3.2e-7), bound 3e-6: below its `len2 >= 1e-10` switch (tilt under 1e-5 rad from
    standing) the routine treats the cylinder as standing (the project's own convention, oracle and device alike): rim direction = the cylinder's x axis and the cap taken
    as level, an error of up to 2 r tilt = 1.6e-6 m at r = 0.08 m.  A property of the convention, below the device's 1e-5.
Every other figure of the run: non-robust share at most 1.65 % (plane_mesh), 1540 .. 1758 robust touching cases per family."""
import numpy as np
import pytest

import orc
import pairgeom as pg
from pairmodels import CAP, families, needed_tol, oracle_contacts, summarize

NCASE = 2000
TOL = {f: 1e-9 for f in pg.FAMILIES}
TOL["capsule_capsule"] = 3e-7
TOL["plane_cylinder"] = 3e-6


@pytest.mark.parametrize("family", pg.FAMILIES)
def test_oracle_passes_the_independent_geometry_check(lib, family):
    rows = []
    for fam in families(lib, family, NCASE):
        d = orc.OrcData(fam.m.ptr)
        for i in range(len(fam.cases)):
            g1, g2, dist, pos, n = oracle_contacts(fam, d, i)
            D = pg.true_distance(g1, g2)
            rob = pg.robust(g1, g2, 0.0, D=D)
            bad = pg.check_contacts(g1, g2, 0.0, dist, pos, n, tol=TOL[family], D=D) if rob else []
            rows.append((rob, len(dist) > 0, bad, needed_tol(g1, g2, dist, pos, n, D=D) if rob else 0.0, fam.cases[i]["tag"]))
    nrob, ntouch, fails, worst = summarize(f"oracle {family}", rows, TOL[family])
    assert len(rows) >= NCASE and nrob >= (1 - CAP) * len(rows) and ntouch >= 0.5 * len(rows)
    assert not fails, fails[:5]


@pytest.mark.parametrize("family", pg.FAMILIES)
def test_the_reference_alone_leaves_out_at_most_two_percent(lib, family):
    """the generators keep the reference's own decisions out of the 1e-4 band: the non-robust share is a property of the cases"""
    cs = [c for fam in families(lib, family, NCASE) for c in fam.cases]
    n = sum(not pg.robust(c["g1"], c["g2"], 0.0) for c in cs)
    assert len(cs) >= NCASE and n <= CAP * len(cs), (family, n, len(cs))
    tags = {c["tag"] for c in cs}
    assert len(tags) >= 2 or family == "plane_sphere", tags


def test_the_checker_is_not_vacuous(lib):
    """every kind of defect the checker claims to see, planted into correct contact lists, is reported.  The missing contact is
    the deepest one.  Which further rim points a cylinder and which further vertices a mesh reports no property pins (the device -
    oracle comparison of tests/test_gpu_pairs.py holds those), so where their deepest contact is tied with another — a standing
    or lying cylinder, a mesh on a facet — the drop is not planted, and such lists are counted apart"""
    seen = dict(flip=0, dist=0, extra=0)
    tried = slid = ncap = ndrop = seen_drop = unpinned = 0
    pinned_by = {}
    for family in pg.FAMILIES:
        for fam in families(lib, family, 96, seed=5):
            d = orc.OrcData(fam.m.ptr)
            for i in range(len(fam.cases)):
                g1, g2, dist, pos, n = oracle_contacts(fam, d, i)
                tol = TOL[family]
                chk = lambda dd, pp, nn: bool(pg.check_contacts(g1, g2, 0.0, dd, pp, nn, tol=tol))
                if not len(dist) or not pg.robust(g1, g2, 0.0) or pg.degenerate(g1, g2, 1e-3):
                    continue
                assert not chk(dist, pos, n)
                tried += 1
                seen["flip"] += chk(dist, pos, -n)
                d2 = dist.copy(); d2[-1] += 1e-4
                seen["dist"] += chk(d2, pos, n)
                seen["extra"] += chk(np.r_[dist, dist[-1]], np.vstack([pos, pos[-1]]), np.vstack([n, n[-1]]))
                if family in ("plane_cylinder", "plane_mesh") and len(dist) > 1 and np.sort(dist)[1] - dist.min() <= pg.BAND:
                    unpinned += 1
                else:
                    keep = np.arange(len(dist)) != int(np.argmin(dist))
                    ndrop += 1; pinned_by[family] = pinned_by.get(family, 0) + 1
                    seen_drop += chk(dist[keep], pos[keep], n[keep] if keep.any() else n[:1])
                if family == "capsule_capsule" and pg.axis_angle(g1, g2) > 0.1:
                    ncap += 1
                    slid += chk(dist, pos + 0.01 * g1[2][:, 2], n)       # slid along capsule 1's axis: leaves capsule 2's
    print(f"PAIRGEOM planted defects: {tried} lists, the drop planted in {ndrop} ({pinned_by}), {unpinned} with a tied deepest contact left out of it")
    assert tried > 600 and ncap > 10
    assert all(pinned_by.get(f, 0) >= 30 for f in pg.FAMILIES), pinned_by
    for what, cnt in seen.items():
        assert cnt == tried, f"planted defect '{what}' went unnoticed in {tried - cnt} of {tried} contact lists"
    assert seen_drop == ndrop, f"a missing deepest contact went unnoticed in {ndrop - seen_drop} of {ndrop} contact lists"
    assert slid == ncap, f"a contact slid 1 cm along a capsule axis went unnoticed in {ncap - slid} of {ncap} lists"
