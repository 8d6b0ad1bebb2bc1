"""CPU: the contract of image undistortion, tools/undistort_model.py, held to what can be stated about it without OpenCV: the
identity at zero coefficients, the value on a ramp (where the bilinear sample is linear in the 1/32-pixel position), one pixel worked
by hand, and the non-finite / far-away positions, which are ordinary cases."""
import numpy as np
import pytest

from tools import undistort_model as um
from tools.synth import KITTI00_SETTINGS

KITTI_K = tuple(float(np.float32(KITTI00_SETTINGS["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))   # read as float, widened
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def _image(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(rows, cols), dtype=np.uint8)


@pytest.mark.parametrize("rows, cols, K", [(376, 1241, KITTI_K), (48, 64, (40.0, 40.0, 31.5, 23.5))])
def test_zero_coefficients_are_the_identity(rows, cols, K):
    img = _image(rows, cols, 1)
    iu, iv = um.undistort_map(rows, cols, K, ZERO)
    assert np.array_equal(iu, 32 * np.broadcast_to(np.arange(cols), (rows, cols)))
    assert np.array_equal(iv, 32 * np.broadcast_to(np.arange(rows)[:, None], (rows, cols)))
    assert np.array_equal(um.undistort(img, K, ZERO), img)


def test_ramp_identity_on_pixels_with_all_taps_inside():
    rows, cols = 48, 64
    K, dist = (40.0, 40.0, 31.5, 23.5), (0.25, 0.05, 0.001, -0.002, 0.0)
    x, y = np.meshgrid(np.arange(cols), np.arange(rows))
    src = (2 * x + y).astype(np.uint8)
    assert int((2 * x + y).max()) <= 255
    iu, iv = um.undistort_map(rows, cols, K, dist)
    inside = um.all_taps_inside(rows, cols, iu, iv)
    assert 0.5 < inside.mean() < 1.0                                   # the case has pixels of both kinds
    want = (32 * (2 * iu + iv) + 512) >> 10
    got = um.remap(src, iu, iv)
    assert np.array_equal(got[inside], want[inside].astype(np.uint8))


def test_a_pixel_worked_by_hand():
    """fx = fy = 32, cx = cy = 4, k1 = 0.5, pixel (row 6, column 8): x = 0.125, y = 0.0625, r2 = 0.01953125, kr = 1.009765625 (all exact
    in binary), xd = 0.126220703125, yd = 0.0631103515625, u = 8.0390625, v = 6.01953125 -> iu = q(257.25) = 257, iv = q(192.625) = 193:
    X0 = 8, a = 1, Y0 = 6, b = 1."""
    K, dist = (32.0, 32.0, 4.0, 4.0), (0.5, 0.0, 0.0, 0.0, 0.0)
    iu, iv = um.undistort_map(12, 16, K, dist)
    assert (int(iu[6, 8]), int(iv[6, 8])) == (257, 193)
    src = np.zeros((12, 16), np.uint8)
    src[6, 8], src[6, 9], src[7, 8], src[7, 9] = 200, 40, 100, 255
    want = (31 * 31 * 200 + 1 * 31 * 40 + 31 * 1 * 100 + 1 * 1 * 255 + 512) >> 10
    assert want == 192
    assert int(um.undistort(src, K, dist)[6, 8]) == want


def test_rounding_ties_go_to_even_and_fractions_of_negative_positions():
    # q: ties to even, NaN -> 0, clamped to int32
    t = np.array([0.5, 1.5, 2.5, -0.5, -1.5, np.nan, np.inf, -np.inf, 1e300, -1e300, 2147483646.5, -2147483648.5])
    assert um._q(t).tolist() == [0, 2, 2, 0, -2, 0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 2, -2 ** 31]
    # iu = -1: X0 = -1 (arithmetic shift), a = 31: the left tap is outside and reads 0, the right one is column 0
    src = np.full((4, 4), 255, np.uint8)
    out = um.remap(src, np.full((1, 1), -1, np.int64), np.full((1, 1), 32, np.int64))
    assert int(out[0, 0]) == (31 * 32 * 255 + 512) >> 10


@pytest.mark.parametrize("case", ["nan", "inf", "far", "w_zero"])
def test_non_finite_and_far_positions_yield_zero(case):
    rows, cols = 24, 32
    K = (20.0, 20.0, 15.5, 11.5)
    src = np.full((rows, cols), 255, np.uint8)
    iR = um.default_iR(K)
    if case == "nan":
        dist = (np.nan, 0.0, 0.0, 0.0, 0.0)
    elif case == "inf":
        dist = (np.inf, 0.0, 0.0, 0.0, 0.0)
    elif case == "far":
        dist = (1e12, 0.0, 0.0, 0.0, 0.0)                              # beyond +-2^26 pixels for every pixel off the centre
    else:
        dist = ZERO
        iR = iR.copy(); iR[8] = 0.0                                    # W = 0: w = inf, x = +-inf or NaN
    with np.errstate(all="raise"):                                     # the model raises nothing and warns of nothing
        iu, iv = um.undistort_map(rows, cols, K, dist, iR)
        out = um.remap(src, iu, iv)
    x, y = np.meshgrid(np.arange(cols), np.arange(rows))
    off_centre = (np.abs(x - 15.5) > 1) | (np.abs(y - 11.5) > 1)
    if case in ("nan", "w_zero"):
        # a NaN position (w_zero: 0 * inf inside kr) is q's first case: the quantised position is 0, an ordinary position like any other
        assert not iu.any() and not iv.any()
        assert (out == src[0, 0]).all()
        src2 = src.copy(); src2[0, 0] = 0
        assert not um.remap(src2, iu, iv).any()
        return
    assert (np.abs(iu[off_centre]) >= 2 ** 31 - 1).all()               # +-inf and beyond +-2^26 pixels clamp to the ends of int32
    assert not out[off_centre].any()


def test_default_iR():
    K = KITTI_K
    iR = um.default_iR(K)
    fx, fy, cx, cy = K
    assert iR.dtype == np.float64 and iR.tolist() == [1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0]
    # a general iR is the inverse of newK * R: at zero rotation it is default_iR up to rounding, and a rotation makes W vary
    assert np.allclose(um.rotated_iR(K, 0.0, 0.0, 0.0), iR, rtol=1e-12, atol=1e-15)
    r = um.rotated_iR(K, *np.deg2rad([2.0, 2.0, 2.0]))
    assert r[6] != 0 and r[7] != 0


def test_distort_image_then_undistort_returns_close_to_the_original():
    """distort_image is only a maker of test inputs, but it must be the inverse warp: a smooth image survives the round trip within the
    two interpolations' error where the source was visible"""
    rows, cols = 60, 80
    K, dist = (60.0, 60.0, 39.5, 29.5), (-0.2, 0.03, 0.0, 0.0, 0.0)
    x, y = np.meshgrid(np.arange(cols), np.arange(rows))
    img = (128 + 60 * np.sin(x / 7.0) + 50 * np.cos(y / 5.0)).astype(np.uint8)
    back = um.undistort(um.distort_image(img, K, dist), K, dist)
    inner = (slice(8, rows - 8), slice(8, cols - 8))
    assert np.abs(back[inner].astype(int) - img[inner].astype(int)).max() <= 6
