"""CPU: the minimal solver of tools/pnp_model.py (p3p, rot_to_quat) against tests/golden/p3p_hp.npz, the P3P solved to 60 digits by a
route that shares nothing with the solver's (tests/golden/make_p3p_hp.py); the inputs are tests/p3p_cases.py.  Which cases are well-posed
is read off the reference alone (sigma_min, separation, stability of the number of solutions); for those the model must return every
solution and nothing else, within the error the generator measured; for EVERY case a slot marked valid must be a pose that explains its own
three points.  tests/test_p3p_gpu.py asserts the same of the kernel."""
import os

import numpy as np

from tools import pnp_model as pm

import p3p_cases as pc


def test_fixture_holds_the_inputs_of_p3p_cases():
    fx = pc.fixture()
    cls, names, X, uv, _, _ = pc.arrays()
    assert fx["X"].tobytes() == X.tobytes() and fx["uv"].tobytes() == uv.tobytes()        # bytes: NaN and inf included
    assert np.array_equal(fx["cls"], cls) and list(fx["names"]) == list(names) and list(fx["classes"]) == list(pc.CLASSES)
    assert np.array_equal(fx["K"], pc.K) and 300 <= len(cls) <= 500
    assert os.path.getsize(pc.FIXTURE) < os.path.getsize(os.path.join(os.path.dirname(pc.FIXTURE), "ref_golden.npz"))


def test_class_counts():
    fx = pc.fixture()
    by = {name: fx["cls"] == k for k, name in enumerate(pc.CLASSES)}
    assert by["baseline"].sum() == 100 and by["random-any"].sum() == 100
    for name in pc.BROAD:
        assert fx["well"][by[name]].mean() >= 0.8, name
    assert fx["well"][by["shape"]].sum() >= 5
    ill = by["ill-posed"]
    assert ill.sum() >= 20 and not fx["well"][ill].any()                   # every ill-posed construction is ill-posed, or has no solution
    # the definition, restated from the stored columns
    for i in range(len(fx["n"])):
        n = fx["n"][i]
        assert fx["well"][i] == bool(n >= 1 and (fx["sigma_min"][i, :n] >= 1e-4).all() and fx["min_sep"][i] >= 1e-3 and fx["stable"][i])
    # NaN, inf, collinear points and a repeated point have no solution at all
    for i in np.nonzero(ill)[0]:
        if any(k in str(fx["names"][i]) for k in ("nan", "inf", "/collinear", "repeated")):
            assert fx["n"][i] == 0
    # where the generating pose has every point in front of the camera it is among the reference's solutions; where not, it is not
    behind = by["behind"]
    assert (fx["gen"][behind] == -1).all() and (fx["gen"][fx["well"] & ~behind] >= 0).all()


def test_model_is_complete_accurate_and_sound():
    """Per class, the model's worst error over the well-posed cases as the generator measured it (fixture: model_worst; the bar of the
    kernel is max(1e-9, 4 x that)):
        baseline 1.6e-13, rotation 3.3e-14, far-world 9.0e-13, shape 2.1e-08 (the 1 cm triangle at 50 m), behind 2.0e-14, random-any 2.9e-13"""
    fx = pc.fixture()
    valid, R, t, pose = pc.model_output()
    worst = pc.check(fx, valid, R, t, pose, fx["model_worst"], zero_invalid=True)
    print("model worst per class:", dict(zip(pc.CLASSES, worst)))
    assert (worst == fx["model_worst"]).all()                              # the stored numbers are this model's
    assert (fx["bar"] == np.maximum(1e-9, 4.0 * fx["model_worst"])).all()


def test_no_valid_slot_without_a_rotation():
    """the near-collinear family: a needle whose height the rounding of its sides has eaten (e = 1e-6 used to return two `rotations'
    with |R R' - I| of 0.02 and 0.06) yields nothing rather than something that is no pose"""
    fx = pc.fixture()
    valid, R, _, _ = pc.model_output()
    for i in range(len(fx["n"])):
        for s in np.nonzero(valid[i])[0]:
            assert np.abs(R[i, s] @ R[i, s].T - np.eye(3)).max() < 1e-7, (fx["names"][i], s)
    i = list(fx["names"]).index("ill-posed/near-collinear-1e-06")
    assert not valid[i].any()
    # the exactly equilateral triangle seen on its axis: both cones of the pencil are plane pairs themselves (det = 0 twice); four poses
    i = list(fx["names"]).index("shape/equilateral-on-axis-5-id")
    assert fx["well"][i] and fx["n"][i] == 4 and valid[i].sum() == 4


def test_cut_offs_stand_where_the_docstring_says():
    """RESID_CUT is 2^24 x and AREA_CUT just under 1e6 x what the reference's own solutions, rounded to double, leave in the solver's
    arithmetic (tools/pnp_model.py gives the reasons)"""
    fx = pc.fixture()
    assert 0.98 * 2 ** 24 < pm.RESID_CUT / fx["ref_resid_worst"] < 1.02 * 2 ** 24
    assert 1e5 < pm.AREA_CUT / fx["ref_area_worst"] < 1e6
    # the model's own solutions of the well-posed cases are nowhere near either
    assert fx["model_resid_worst"] < 1e-6 * pm.RESID_CUT and fx["model_area_worst"] < 0.05 * pm.AREA_CUT


def test_rot_to_quat_on_every_branch():
    fx = pc.fixture()
    taken = np.zeros((len(pc.CLASSES), 4), int)
    for i in range(len(fx["n"])):
        for s in range(fx["n"][i]):
            R, q = fx["R"][i, s], fx["q"][i, s]
            got = pm.rot_to_quat(R)
            assert min(np.abs(got - q).max(), np.abs(got + q).max()) < 1e-14, (fx["names"][i], s)
            assert abs(np.sqrt((got * got).sum()) - 1) < 1e-15 and got[3] >= 0
            taken[fx["cls"][i], pc.quat_branch(R)] += 1
    assert (taken[pc.CLASSES.index("rotation")] >= 10).all(), taken
    assert (taken[pc.CLASSES.index("random-any")] >= 1).all(), taken


def test_rot_to_quat_at_exactly_half_a_turn():
    for k, e in enumerate(np.eye(3)):
        R = pc.rodrigues(e, np.pi)
        assert np.array_equal(R, np.diag(2 * e - 1))
        q = pm.rot_to_quat(R)
        assert q[3] == 0 and (np.array_equal(q[:3], e) or np.array_equal(q[:3], -e))
    q = pm.rot_to_quat(np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]))       # 120 degrees about (1, 1, 1): the trace is exactly 0
    np.testing.assert_allclose(q, [0.5, 0.5, 0.5, 0.5], rtol=0, atol=1e-16)
    s = np.sqrt(0.5)
    for R, want in ((np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]]), [s, s, 0, 0]),     # half a turn about (1, 1, 0): R00 = R11, the y branch
                    (np.array([[-1.0, 0, 0], [0, 0, 1], [0, 1, 0]]), [0, s, s, 0])):    # ... about (0, 1, 1): R11 = R22, the z branch
        q = pm.rot_to_quat(R)
        assert q[3] == 0
        assert min(np.abs(q - want).max(), np.abs(q + np.array(want)).max()) < 1e-15
