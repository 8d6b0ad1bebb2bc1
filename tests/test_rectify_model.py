"""CPU: the contract of stereo rectification (tools/rectify_model.py) against what it must mean -- rectify's geometry, atan_c against a
40-digit atan, lens_map's two models."""
import mpmath
import numpy as np
import pytest

from tools import rectify_model as rm
from tools import undistort_model as um

K_L, K_R = (40.0, 40.0, 31.5, 23.5), (41.0, 39.5, 32.2, 22.9)
KB_L, KB_R = (-0.02, 0.005, -0.001, 0.0002), (0.03, -0.01, 0.002, -0.0003)


def rotated_rig(**over):
    rig = dict(cam=[dict(model=rm.KB4, K=K_L, coeffs=KB_L), dict(model=rm.KB4, K=K_R, coeffs=KB_R)],
               R=rm.rot(*np.deg2rad([1.5, -2.0, 1.0])), t=(-0.11, 0.004, -0.003))
    rig.update(over)
    return rig


def test_rotations_are_orthonormal_with_det_one():
    out = rm.rectify(rotated_rig())
    for Rs in (out["R_l"], out["R_r"]):
        assert np.abs(Rs @ Rs.T - np.eye(3)).max() < 1e-14
        assert abs(np.linalg.det(Rs) - 1.0) < 1e-14
    assert abs(out["b"] - np.linalg.norm(rotated_rig()["t"])) < 1e-15


def test_points_land_on_one_row_at_one_depth_a_baseline_apart():
    rig = rotated_rig()
    out = rm.rectify(rig)
    f, _, cx, cy = out["newK"]
    rng = np.random.default_rng(2)
    X = np.stack([rng.uniform(-2, 2, 200), rng.uniform(-1.5, 1.5, 200), rng.uniform(2, 20, 200)], 1)
    Xr = X @ np.asarray(rig["R"]).T + np.asarray(rig["t"])
    assert (Xr[:, 2] > 0).all()
    Pl, Pr = X @ out["R_l"].T, Xr @ out["R_r"].T
    vl, vr = f * Pl[:, 1] / Pl[:, 2] + cy, f * Pr[:, 1] / Pr[:, 2] + cy
    assert np.abs(vl - vr).max() < 1e-12
    assert np.abs(Pl[:, 2] - Pr[:, 2]).max() < 1e-12
    assert np.abs((Pl[:, 0] - Pr[:, 0]) - out["b"]).max() < 1e-12
    # and the common camera is the stated mean
    assert out["newK"].tolist() == [(40.0 + 40.0 + 41.0 + 39.5) / 4, (40.0 + 40.0 + 41.0 + 39.5) / 4, (31.5 + 32.2) / 2, (23.5 + 22.9) / 2]


def test_iR_is_the_inverse_of_newK_R():
    out = rm.rectify(rotated_rig(f=22.0))
    f, _, cx, cy = out["newK"]
    A = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    for Rs, iR in ((out["R_l"], out["iR_l"]), (out["R_r"], out["iR_r"])):
        assert np.abs(iR.reshape(3, 3) @ (A @ Rs) - np.eye(3)).max() < 1e-13


@pytest.mark.parametrize("K", [(40.0, 40.0, 31.5, 23.5), (718.856, 718.856, 607.1928, 185.2157)])
def test_a_rectified_rig_is_left_alone_bit_for_bit(K):
    cam = dict(model=rm.RADTAN, K=K, coeffs=(0.0,) * 5)
    out = rm.rectify(dict(cam=[cam, cam], R=np.eye(3), t=(-0.537, 0.0, 0.0)))
    eye = np.eye(3)
    assert out["R_l"].tobytes() == eye.tobytes() and out["R_r"].tobytes() == eye.tobytes()
    assert out["iR_l"].tobytes() == um.default_iR(K).tobytes() and out["iR_r"].tobytes() == um.default_iR(K).tobytes()
    assert out["b"] == 0.537 and out["newK"].tolist() == list(K)


def test_overrides_replace_the_means():
    out = rm.rectify(rotated_rig(f=22.0, cx=30.0, cy=25.0))
    assert out["newK"].tolist() == [22.0, 22.0, 30.0, 25.0]
    assert np.array_equal(out["R_l"], rm.rectify(rotated_rig())["R_l"])


def test_each_refusal_has_its_own_reason():
    Rbad = np.array(rotated_rig()["R"]); Rbad[0, 0] += 1e-5
    cases = {
        "model": rotated_rig(cam=[dict(model=2, K=K_L, coeffs=KB_L), dict(model=rm.KB4, K=K_R, coeffs=KB_R)]),
        "finite": rotated_rig(t=(np.nan, 0.0, 0.0)),
        "baseline": rotated_rig(t=(0.0, 0.0, 0.0)),
        "rotation": rotated_rig(R=Rbad),
        "side": rotated_rig(t=(0.11, 0.0, 0.0)),
        "axes": rotated_rig(R=np.eye(3), t=(-1e-9, 0.0, -0.1)),
    }
    seen = set()
    for name, rig in cases.items():
        with pytest.raises(ValueError) as e:
            rm.rectify(rig)
        assert str(e.value) == rm.REASONS[name], (name, str(e.value))
        seen.add(str(e.value))
    assert len(seen) == len(rm.REASONS)
    for bad in (dict(R=np.full((3, 3), np.inf)), dict(f=np.inf), dict(cam=[dict(model=rm.KB4, K=(np.nan, 1, 1, 1), coeffs=KB_L), dict(model=rm.KB4, K=K_R, coeffs=KB_R)])):
        with pytest.raises(ValueError, match="non-finite"):
            rm.rectify(rotated_rig(**bad))


def _ulp_error(x, got):
    """|got - atan(x)| in units of got's last place, atan to 40 digits"""
    mpmath.mp.dps = 40
    err = abs(mpmath.mpf(float(got)) - mpmath.atan(mpmath.mpf(float(x))))
    return float(err / mpmath.mpf(float(np.spacing(got))))


def test_atan_c_is_within_one_ulp_of_a_40_digit_atan():
    x = rm.atan_sweep()
    x = x[np.isfinite(x)]
    got = rm.atan_c(x)
    worst = max(_ulp_error(a, g) for a, g in zip(x, got) if a > 0)
    print("atan_c: worst error %.3f ulp over %d arguments" % (worst, len(x)))
    assert worst <= 1.0
    assert (np.diff(rm.atan_c(np.sort(x))) >= 0).all()                    # and it does not decrease across a breakpoint


def test_atan_c_special_values():
    got = rm.atan_c(np.array([0.0, np.nan, np.inf, 1e300, 2.0 ** 66]))
    assert got[0] == 0.0 and not np.signbit(got[0]) and np.isnan(got[1])
    assert got[2] == got[3] == got[4] == np.float64(np.pi / 2)
    assert rm.atan_c(np.float64(1.0)) == np.float64(np.pi / 4)


def test_radtan_is_undistort_map_array_for_array():
    dist = (-0.28, 0.07, 0.004, -0.003, 0.01)
    iR = rm.rectify(rotated_rig())["iR_r"]
    for r in (None, iR):
        a, b = rm.lens_map(45, 67, rm.RADTAN, K_R, dist, r), um.undistort_map(45, 67, K_R, dist, r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        rm.lens_map(4, 4, 7, K_R, dist)


def test_kb4_without_coefficients_is_f_theta():
    """iR = default_iR, all k = 0: the principal point maps to itself, a pixel at r = tan(theta) from it maps to f * theta"""
    K = (40.0, 40.0, 32.0, 24.0)
    iu, iv = rm.lens_map(48, 64, rm.KB4, K, (0.0,) * 4)
    assert iu[24, 32] == 32 * 32 and iv[24, 32] == 24 * 32
    jj, ii = np.meshgrid(np.arange(64.0), np.arange(48.0))
    x, y = (jj - 32.0) / 40.0, (ii - 24.0) / 40.0
    r = np.hypot(x, y)
    s = np.where(r > 0, np.arctan(r) / np.where(r > 0, r, 1.0), 1.0)
    assert np.abs(iu / 32.0 - (40.0 * x * s + 32.0)).max() <= 1 / 32 and np.abs(iv / 32.0 - (40.0 * y * s + 24.0)).max() <= 1 / 32
    assert np.abs(np.hypot(iu / 32.0 - 32.0, iv / 32.0 - 24.0) - 40.0 * np.arctan(r)).max() <= 1 / 32


def test_pixels_behind_the_camera_are_zero():
    """a 50 degree pitch at 48 x 64 with K = (22, 22, 31.5, 23.5): the rows with W <= 0 -- 12.5 % of the pixels -- read nothing"""
    K = (22.0, 22.0, 31.5, 23.5)
    iR = um.rotated_iR(K, np.deg2rad(50.0), 0.0, 0.0)
    W = (np.arange(64.0)[None, :] * iR[6] + np.arange(48.0)[:, None] * iR[7]) + iR[8]
    behind = ~(W > 0)
    assert abs(behind.mean() - 0.125) < 0.03
    img = np.random.default_rng(3).integers(1, 256, size=(48, 64), dtype=np.uint8)
    out = rm.rectify_image(img, rm.KB4, K, KB_L, iR)
    assert not out[behind].any() and out[~behind].any()
    iu, iv = rm.lens_map(48, 64, rm.KB4, K, KB_L, iR)
    assert (iu[behind] == um.INT32_MIN).all() and (iv[behind] == um.INT32_MIN).all()


def test_unrectify_then_rectify_gives_the_rendering_back():
    """the test-input helper inverts the contract: away from the border, a smooth image warped out and rectified again is itself to
    3 grey levels.  The image's slope is at most 12 levels a pixel and its curvature 2.4: each of the two bilinear resamplings errs by
    curvature / 8 = 0.3 and rounds by 0.5, and the map's 1/32 pixel is 0.4 -- 2.0 in all, and one level of margin."""
    rig = rotated_rig(f=30.0)
    out = rm.rectify(rig)
    jj, ii = np.meshgrid(np.arange(64.0), np.arange(48.0))
    img = np.rint(128 + 60 * np.sin(jj / 6.0) * np.cos(ii / 5.0)).astype(np.uint8)
    for side, model, K, co in ((0, rm.KB4, K_L, KB_L), (1, rm.RADTAN, K_R, (-0.05, 0.01, 0.001, -0.001, 0.0))):
        Rs, iR = (out["R_l"], out["iR_l"]) if side == 0 else (out["R_r"], out["iR_r"])
        raw = rm.unrectify_image(img, out["newK"], Rs, model, K, co)
        back = rm.rectify_image(raw, model, K, co, iR)
        inner = (slice(14, 34), slice(18, 46))
        assert np.abs(back[inner].astype(int) - img[inner].astype(int)).max() <= 3, side
