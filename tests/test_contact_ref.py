"""The numpy reference of the contact report (tests/contact_ref.py) against the fp64 oracle, without a GPU: its cfrc_ext equals the oracle's
own on a model with a force sensor, a connect, a weld and xfrc_applied; its decoded contact forces reproduce qfrc_constraint through efc_J;
and the scenes the GPU tests use have the contacts they are meant to have, all in clear penetration."""
import numpy as np
import pytest

import contact_ref as cr
import contact_scenes as cs


def _stepped(m, q, v, xf=None):
    d = cs.oracle_at(m, q, v, xf)
    d.step(1)
    return d


def test_cfrc_ext_equals_the_oracles_own(lib):
    # both are fp64 sums of the same summands (xfrc_applied, contacts, connect and weld rows), in a different order.
    # Measured on the first run: worst |difference| / max|cfrc_ext| = 1.1e-16 over the five envs
    m = cs.arm_scene(lib, sensor=True)
    assert m.nsensor == 1 and m.neq == 2
    q, v, xf = cs.arm_states(m, 5)
    worst = 0.0
    for i in range(5):
        d = _stepped(m, q[i], v[i], xf[i])
        assert d.i("ncon") == cs.ARM_NCON and d.i("warn") == 0
        own = d.f("cfrc_ext").reshape(m.nbody, 6).copy()
        ref = cr.cfrc_ext(m, d)
        scale = np.abs(own).max()
        assert scale > 1.0
        # every source is present: contact, connect, weld, applied
        for name in ("l2", "box", "bob", "cube", "base"):
            assert np.abs(own[m.name2id(0, name)]).max() > 1e-3, name
        worst = max(worst, np.abs(ref - own).max() / scale)
    print(f"contact_ref.cfrc_ext vs oracle cfrc_ext: worst relative difference {worst:.2e}")
    assert worst <= 1e-10, worst


@pytest.mark.parametrize("scene", ["free3", "free4", "free1", "arm"])
def test_decoded_forces_reproduce_qfrc_constraint(scene, lib):
    if scene == "arm":
        m = cs.arm_scene(lib); q, v, xf = cs.arm_states(m, 2)
    else:
        m = cs.free_scene(lib, condim=int(scene[-1])); q, v = cs.free_states(m, 2, spin=5.0); xf = [None, None]
    for i in range(2):
        d = _stepped(m, q[i], v[i], xf[i])
        cons = d.contacts()
        cf = cr.contact_forces(m, d, cons)
        assert (cf[:, 0] > 0).all(), cf[:, 0]
        assert all(c["dim"] == (3 if scene == "arm" else int(scene[-1])) for c in cons)
        ref = d.f("qfrc_constraint")
        np.testing.assert_allclose(cr.qfrc_from_decoded(m, d, cons), ref, rtol=0, atol=1e-10 * max(1.0, np.abs(ref).max()))
        if scene == "free4":
            sph = [k for k, c in enumerate(cons) if m.array("geom_type")[c["geom"][1]] == cs.GEOM_SPHERE]
            assert len(sph) == 1 and abs(cf[sph[0], 3]) > 1e-6      # the spinning sphere's torsional friction is at work


@pytest.mark.parametrize("scene", ["free", "arm"])
def test_scene_contacts_are_in_clear_penetration_and_the_same_in_every_env(scene, lib):
    if scene == "arm":
        m = cs.arm_scene(lib); q, v, xf = cs.arm_states(m, 5); want = cs.ARM_NCON
    else:
        m = cs.free_scene(lib); q, v = cs.free_states(m, 5); xf = [None] * 5; want = cs.FREE_NCON
    pairs = None
    for i in range(5):
        d = _stepped(m, q[i], v[i], xf[i])
        cons = d.contacts()
        assert len(cons) == want, (i, len(cons))
        # the activation margin is 0: every contact at least 1e-4 inside it (and nothing hovers just outside: the count is exact)
        assert all(c["dist"] < -1e-4 for c in cons), [c["dist"] for c in cons]
        assert all(len(cr.contact_rows(d, k)) == 4 for k in range(len(cons)))
        p = sorted(c["geom"] for c in cons)
        pairs = p if pairs is None else pairs
        assert p == pairs, (i, p, pairs)


def test_body_sums_signs_and_filter(lib):
    m = cs.free_scene(lib)
    q, v = cs.free_states(m, 1)
    d = _stepped(m, q[0], v[0])
    cons = d.contacts(); cf = cr.contact_forces(m, d, cons)
    A, B, S = (m.name2id(0, n) for n in ("A", "B", "S"))
    F, cnt = cr.body_sums(m, cons, cf, [A, B, S, A, A], [-1, -1, -1, 0, B])
    assert list(cnt) == [8, 4, 1, 4, 4]
    np.testing.assert_allclose(F[0], F[3] + F[4], atol=1e-12)            # floor part + B part
    np.testing.assert_allclose(F[4], -F[1], atol=1e-12)                  # what B does to A is minus what A does to B
    assert F[1][2] > 0 and F[2][2] > 0 and F[3][2] > 0 and F[4][2] < 0   # supports push up, the load pushes down
    # the force half of cfrc_ext of a body without applied or equality force is its contact sum
    ext = cr.cfrc_ext(m, d, cons)
    for k, b in enumerate((A, B, S)):
        np.testing.assert_allclose(ext[b, 3:], F[k], atol=1e-12)
