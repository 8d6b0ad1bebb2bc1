"""CPU: the stored form of an undistortion map, tools/undistort_model.py's pack_map / unpack_map (what ssx_undistort_plan keeps per
camera): sampling with the unpacked map gives the bytes of sampling with the map itself, although the integer position is clamped to
[-2, cols] x [-2, rows] to fit a u16.  Every case states the share of its pixels that the clamp changes, so that none is vacuous:
0 where every position is near the image, about a sixth for the pincushion maps (both below -2 and above the far edge), nine in ten
for the far-outside map and all of them for the infinite ones."""
import numpy as np
import pytest

from tools import undistort_model as um

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
K_A = (40.0, 40.0, 31.5, 23.5)
PINCUSHION = (0.25, 0.05, 0.0, 0.0, 0.0)
# name: (rows, cols, K, dist, iR or "rotated" or None, the clamped share: (low, high), both inclusive)
CASES = {
    # the five cases of tests/test_undistort_gpu.py
    "barrel": (48, 64, K_A, (-0.3, 0.1, 0.0, 0.0, 0.0), None, (0.0, 0.0)),
    "pincushion": (48, 64, K_A, PINCUSHION, None, (0.15, 0.18)),
    "tangential": (45, 67, (38.0, 41.0, 30.2, 20.7), (-0.28, 0.07, 0.004, -0.003, 0.01), None, (0.0, 0.0)),
    "small_third": (60, 80, (48.0, 48.0, 40.3, 29.6), (0.1, -0.2, 0.001, 0.0005, 0.05), None, (0.0, 0.0)),
    "rotated": (48, 64, K_A, PINCUSHION, "rotated", (0.15, 0.18)),
    "5 x 7": (5, 7, (6.0, 6.0, 3.0, 2.0), (-0.2, 0.05, 0.001, -0.001, 0.0), None, (0.0, 0.0)),
    "far outside": (48, 64, K_A, (50.0, 0.0, 0.0, 0.0, 0.0), None, (0.90, 0.93)),
    # the four non-finite sets: a NaN position quantises to 0, a position like any other; the infinite ones clamp everywhere
    "nan": (48, 64, K_A, (np.nan, 0, 0, 0, 0), None, (0.0, 0.0)),
    "inf": (48, 64, K_A, (np.inf, 0, 0, 0, 0), None, (1.0, 1.0)),
    "1e300": (48, 64, K_A, (1e300, 1e300, 0, 0, 1e300), None, (1.0, 1.0)),
    "-1e12": (48, 64, K_A, (-1e12, 0, 0, 0, 0), None, (1.0, 1.0)),
    "W = 0": (48, 64, K_A, ZERO, "w0", (0.0, 0.0)),
}


def _iR(K, kind):
    if kind == "rotated":
        return um.rotated_iR(K, *np.deg2rad([2.0, 2.0, 2.0]))
    if kind == "w0":
        iR = um.default_iR(K).copy()
        iR[8] = 0.0
        return iR
    return None


@pytest.mark.parametrize("name", list(CASES))
def test_sampling_through_the_stored_map_gives_the_same_bytes(name):
    rows, cols, K, dist, kind, (lo, hi) = CASES[name]
    iu, iv = um.undistort_map(rows, cols, K, dist, _iR(K, kind))
    xs, ys, ab = um.pack_map(rows, cols, iu, iv)
    assert xs.dtype == ys.dtype == ab.dtype == np.uint16 and xs.shape == ys.shape == ab.shape == (rows, cols)
    assert xs.max() <= cols + 2 and ys.max() <= rows + 2 and ab.max() < 1024
    iu2, iv2 = um.unpack_map(xs, ys, ab)
    rng = np.random.default_rng(7)
    for img in (rng.integers(1, 256, size=(rows, cols), dtype=np.uint8), np.full((rows, cols), 255, np.uint8)):
        assert np.array_equal(um.remap(img, iu2, iv2), um.remap(img, iu, iv))
    share = um.clamped_share(rows, cols, iu, iv)
    assert lo <= share <= hi, share
    # the clamp changes a position exactly where the case says it does, and nowhere else
    changed = (iu2 != iu) | (iv2 != iv)
    assert changed.mean() == share


def test_the_clamp_is_tight_on_both_sides():
    """positions at the clamp's four bounds and one beyond each: the stored value, and that all taps of the axis are outside"""
    rows, cols = 6, 9
    X0 = np.array([[-3, -2, -1, 0, cols - 1, cols, cols + 1, 5, 5]] * rows, dtype=np.int64)
    Y0 = np.array([[2, 2, 2, 2, 2, 2, 2, -3, rows + 1]] * rows, dtype=np.int64)
    iu, iv = (X0 << 5) | 17, (Y0 << 5) | 9
    xs, ys, ab = um.pack_map(rows, cols, iu, iv)
    assert xs[0].tolist() == [0, 0, 1, 2, cols + 1, cols + 2, cols + 2, 7, 7] and ys[0].tolist() == [4, 4, 4, 4, 4, 4, 4, 0, rows + 2]
    assert (ab == (17 | 9 << 5)).all()
    img = np.full((rows, cols), 200, np.uint8)
    iu2, iv2 = um.unpack_map(xs, ys, ab)
    out = um.remap(img, iu2, iv2)
    assert np.array_equal(out, um.remap(img, iu, iv))
    assert not out[:, [0, 1, 5, 6, 7, 8]].any() and out[:, [2, 3, 4]].all()


def test_a_side_above_65533_is_refused():
    z = np.zeros((1, 65534), dtype=np.int64)
    with pytest.raises(ValueError, match="65533"):
        um.pack_map(1, 65534, z, z)
    with pytest.raises(ValueError, match="65533"):
        um.pack_map(65534, 1, z.T, z.T)
    z = np.zeros((1, 65533), dtype=np.int64)
    xs, _, _ = um.pack_map(1, 65533, z + (65533 << 5), z)                # the far bound of the widest image fits
    assert int(xs[0, 0]) == 65535
