"""The device's analytic narrow-phase pairs (dev_collide.h: c_plane_{sphere, capsule, cylinder, ellipsoid, box, mesh},
c_sphere_sphere, c_sphere_capsule, c_capsule_capsule, c_sphere_box, reached through mjh_forward + mjh_get_contacts) against the
independent fp64 geometry of tests/pairgeom.py, and against the oracle from the identical pose.

The families of tests/test_pairgeom.py, 1536 environments per family (a plane family: 768 on a horizontal plane, 768 on a tilted
one), every env its own pose and geom sizes; one forward(), the reference geoms from the device's own exported geom poses cast to
float64: only the narrow phase is under test.  Tolerance 1e-5 on `dist` and surface membership, the project's bound for the same
check on boxes at the same coordinate range (test_gpu_round4.py); cases with a decision of the reference within 1e-4 of the margin
are left out, at most 2 % of a family; envs over the contact capacity are skipped, fewer than 2 %.  Half of the capsule_capsule
cases have axes closer than 1e-3 rad.

Against the oracle (well-conditioned cases only — pairgeom.well_conditioned: no tied box face, a cylinder neither standing nor
lying, a unique deepest mesh vertex; capsule axes more than 0.1 rad apart, or more than 1e-2 rad apart with the stationary point at
least 1 cm outside the parameter box — narrower than "more than 1e-2 rad": the stationary point's parameters carry the operands'
fp32 rounding, 6e-8 at 0.5 m, divided by angle^2, which is 6e-4 m at 1e-2 rad against a bound of 2e-5, while a minimum on an edge of
the box needs no such division): equal counts, dist within 2e-6, pos within 2e-5, the
bounds of test_plane_contacts_of_round_geoms_match_oracle.  This pins what the properties cannot: which rim points a cylinder and
which vertices a mesh reports, and their order.

MEASURED on an MI355X (the run's `PAIRGEOM device ...` lines; `passes from`: the smallest tolerance of a half-decade ladder from
1e-7 at which every robust case of the family passes — the worst violation lies below it; each test takes under 2 s):

  family           cases  non-robust  robust touching  violations at 1e-5  passes from | oracle: cases  points  count mismatches  max |dist|  max |pos|  over capacity
  plane_sphere      1536    0.00 %         1228                0            1.0e-7    |         1536    1228         0          3.7e-8     3.3e-8       0
  plane_capsule     1536    0.72 %         1239                0            1.0e-7    |         1525    1659         0          5.4e-8     4.7e-8       0
  plane_cylinder    1536    0.91 %         1236                0            1.0e-6    |          495     446         0          2.9e-8     1.9e-7       0
  plane_ellipsoid   1536    0.00 %         1199                0            1.0e-7    |         1536    1199         0          3.3e-8     6.9e-8       0
  plane_box         1536    0.00 %         1219                0            1.0e-7    |         1536    3313         0          4.1e-8     5.2e-8       0
  plane_mesh        1536    1.56 %         1190                0            1.0e-7    |          878     881         0          4.7e-8     4.7e-8       0
  sphere_sphere     1536    0.00 %         1184                0            1.0e-7    |         1344     992         0          4.3e-8     2.8e-8       0
  sphere_capsule    1536    0.00 %         1262                0            1.0e-7    |         1344    1070         0          4.3e-8     3.9e-8       0
  capsule_capsule   1536    0.00 %         1212                0            1.0e-6    |          620     486         0          5.1e-8     4.4e-7       0
  sphere_box        1536    0.00 %         1359                0            1.0e-7    |         1312    1135         0          4.8e-8     4.0e-8       0
"""
import numpy as np
import pytest

import mujoco_sim_amd as ms
import orc
import pairgeom as pg
from pairmodels import CAP, families, needed_tol, oracle_contacts, summarize

pytestmark = pytest.mark.gpu
NENV = 1536
TOL = 1e-5
LADDER = [1e-7 * 10 ** (k / 2) for k in range(14)]


@pytest.mark.parametrize("family", pg.FAMILIES)
def test_device_pairs_pass_the_independent_geometry_check_and_match_the_oracle(lib, family):
    rows = []
    nover = ncmp = npts = 0
    worst_d = worst_p = 0.0
    mismatched = []
    for fam in families(lib, family, NENV):
        n = len(fam.cases)
        e = ms.Engine(fam.m, n)
        e.set_env_param("geom_size", fam.size.reshape(n, -1)); e.set_env_param("geom_rbound", fam.rbound)
        e.set_state(qpos=fam.qpos, qvel=np.zeros((n, fam.m.nv)))
        e.forward(); e.synchronize()
        gp, gm = e.get_geom_state()
        st = e.get_stats()
        d = orc.OrcData(fam.m.ptr)
        for i in range(n):
            if st[i, 3] & 1:
                nover += 1; continue            # (contact capacity exceeded: the list is cut)
            c = e.get_contacts(i)
            g1, g2 = fam.geoms(gp[i], gm[i], i)
            dist, pos, nrm = c["dist"], c["pos"], c["frame"][:, :3]
            assert all(tuple(g) == (0, 1) for g in c["geom"])
            D = pg.true_distance(g1, g2)
            rob = pg.robust(g1, g2, 0.0, D=D)
            need = needed_tol(g1, g2, dist, pos, nrm, LADDER, 0.0, D) if rob else 0.0
            bad = pg.check_contacts(g1, g2, 0.0, dist, pos, nrm, tol=TOL, D=D) if need > TOL else []
            rows.append((rob, len(dist) > 0, bad, need, fam.cases[i]["tag"]))
            if rob and pg.well_conditioned(g1, g2):
                _, _, od, op, _ = oracle_contacts(fam, d, i)
                ncmp += 1
                if len(od) != len(dist):
                    mismatched.append((i, fam.cases[i]["tag"], len(od), len(dist))); continue
                if len(od):
                    npts += len(od)
                    worst_d = max(worst_d, np.abs(od - dist).max()); worst_p = max(worst_p, np.abs(op - pos).max())
        e.close()
    nrob, ntouch, fails, worst = summarize(f"device {family}", rows, TOL)
    print(f"PAIRGEOM device {family} vs oracle: {ncmp} well-conditioned cases, {npts} points, count mismatches {len(mismatched)}, "
          f"max |dist - oracle| {worst_d:.2e}, max |pos - oracle| {worst_p:.2e}; {nover} envs over the capacity")
    assert nover < CAP * NENV, f"{nover} envs over the contact capacity"
    assert len(rows) + nover >= NENV and nrob >= (1 - CAP) * (len(rows) + nover), (len(rows), nrob)
    assert ntouch >= 1000, f"only {ntouch} robust touching cases"
    if family == "capsule_capsule":
        close = sum(pg.axis_angle(c["g1"], c["g2"]) < 1e-3 for fam in families(lib, family, NENV) for c in fam.cases)
        assert close >= NENV // 2, close
    assert not fails, (len(fails), fails[:5])
    assert ncmp >= 300 and npts >= 300, (ncmp, npts)
    assert not mismatched, mismatched[:5]
    assert worst_d <= 2e-6 and worst_p <= 2e-5, (worst_d, worst_p)
