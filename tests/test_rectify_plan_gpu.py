"""GPU: lens models in the undistortion plan (csrc/undistort.hip: ssx_undistort_plan_add_lens, k_undistort_map) -- the stored map is
pack_map of tools/rectify_model.py's lens_map, array_equal; applying it gives ssx_undistort_lens's bytes; a radtan set is one map
whichever `add` it came through.  Expected bytes come from the model, never from the library."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import undistort as ud
from tools import rectify_model as rm
from tools import undistort_model as um

pytestmark = pytest.mark.gpu

K_L, K_R = (40.0, 40.0, 31.5, 23.5), (41.0, 39.5, 32.2, 22.9)
KB_L, KB_R = (-0.02, 0.005, -0.001, 0.0002), (0.03, -0.01, 0.002, -0.0003)
RT = (-0.28, 0.07, 0.004, -0.003, 0.01)


@pytest.fixture(scope="module")
def rig():
    return rm.rectify(dict(cam=[dict(model=rm.KB4, K=K_L, coeffs=KB_L), dict(model=rm.KB4, K=K_R, coeffs=KB_R)],
                           R=rm.rot(*np.deg2rad([1.5, -2.0, 1.0])), t=(-0.11, 0.004, -0.003), f=22.0))


def _image(rows, cols, seed, stride=None):
    rng = np.random.default_rng(seed)
    buf = rng.integers(1, 256, size=(rows, cols if stride is None else stride), dtype=np.uint8)
    return buf[:, :cols]


@pytest.mark.parametrize("side, rows, cols", [(0, 48, 64), (1, 45, 67)])
def test_the_stored_kb4_map_and_its_image_equal_the_model(ctx, rig, side, rows, cols):
    K, co, iR = (K_L, KB_L, rig["iR_l"]) if side == 0 else (K_R, KB_R, rig["iR_r"])
    prm = ud.make_lens_params(rm.KB4, K, co, iR)
    img = _image(rows, cols, 61 + side, 80)
    iu, iv = rm.lens_map(rows, cols, rm.KB4, K, co, iR)
    assert min(rm.rig_share(rows, cols, iu, iv)) > 0.03 and um.clamped_share(rows, cols, iu, iv) > 0.1    # every border path, and the clamp
    with ud.UndistortPlan(ctx, rows, cols) as plan:
        m = plan.add_lens(prm)
        assert m == 0 and plan.size() == (rows, cols, 1)
        assert plan.last_call() == dict(launches=1, syncs=1, bytes_up=0, bytes_down=0, copies_up=0, copies_down=0)
        for got, want, plane in zip(plan.packed_map(m), um.pack_map(rows, cols, iu, iv), ("xs", "ys", "ab")):
            assert np.array_equal(got, want), plane
        got = plan.apply([img], [m], dst_stride=73)[0]
        assert np.array_equal(got, um.remap(img, iu, iv))
        assert np.array_equal(got, ud.undistort_lens(ctx, [img], [prm])[0])      # the inline form on the same inputs
        assert plan.add_lens(prm) == 0 and plan.last_call()["launches"] == 0     # equal bytes: the map it has


def test_a_radtan_set_is_one_map_through_both_adds(ctx, rig):
    rows, cols = 45, 67
    img = _image(rows, cols, 63)
    with ud.UndistortPlan(ctx, rows, cols) as plan:
        a = plan.add(ud.make_params(K_R, RT, rig["iR_r"]))
        b = plan.add_lens(ud.make_lens_params(rm.RADTAN, K_R, RT, rig["iR_r"]))
        c = plan.add_lens(ud.make_lens_params(rm.KB4, K_R, RT, rig["iR_r"]))      # the same numbers as another lens: another map
        assert (a, b, c) == (0, 0, 1) and plan.size() == (rows, cols, 2)
        got = plan.apply([img, img], [a, c])
        assert np.array_equal(got[0], um.undistort(img, K_R, RT, rig["iR_r"]))
        assert np.array_equal(got[1], rm.rectify_image(img, rm.KB4, K_R, RT, rig["iR_r"])) and not np.array_equal(got[0], got[1])
        assert plan.last_call()["launches"] == 1 and plan.last_call()["syncs"] == 1
    with ud.UndistortPlan(ctx, rows, cols) as plan:                               # and the other way round
        assert plan.add_lens(ud.make_lens_params(rm.RADTAN, K_R, RT)) == 0 and plan.add(ud.make_params(K_R, RT)) == 0


def test_an_unknown_model_is_refused_and_the_plan_unchanged(ctx, rig):
    with ud.UndistortPlan(ctx, 48, 64) as plan:
        lib = plan.lib
        for model in (2, -1):
            m = C.c_int32(-7)
            prm = ud.make_lens_params(model, K_L, KB_L, rig["iR_l"])
            st = lib.ssx_undistort_plan_add_lens(plan.handle, C.byref(prm), C.byref(m))
            msg = lib.ssx_last_error(ctx.handle).decode()
            assert st == _lib.SSX_ERR_INVALID_ARG and msg.startswith("ssx_undistort_plan_add_lens:") and "lens model %d" % model in msg, msg
            assert m.value == -7 and plan.size() == (48, 64, 0) and plan.last_call()["launches"] == 0
        st = lib.ssx_undistort_plan_add_lens(plan.handle, None, C.byref(m))
        assert st == _lib.SSX_ERR_INVALID_ARG and "prm is null" in lib.ssx_last_error(ctx.handle).decode()
