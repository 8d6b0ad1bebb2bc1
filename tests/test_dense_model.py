"""CPU: the contract of dense stereo, tools/dense_model.py, against values worked out by hand, and as a stereo matcher against the
ground truth of the project's own synthetic pair."""
import numpy as np
import pytest

from tools import dense_model as dm
from tools.synth import make_stereo_pair


def _census_by_definition(img, y, x):
    rows, cols = img.shape
    w = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            nb = img[min(max(y + dy, 0), rows - 1), min(max(x + dx, 0), cols - 1)]
            w = (w << 1) | int(nb < img[y, x])
    return w


def test_census_of_a_hand_made_patch():
    patch = np.array([[50] * 9,
                      [150] * 9,
                      [50, 150, 50, 150, 50, 150, 50, 150, 50],
                      [50, 50, 50, 50, 100, 100, 100, 100, 100],      # the centre (100) and, right of it, equal values: strict, so 0
                      [150] * 8 + [99],
                      [100] * 9,
                      [0] * 9], dtype=np.uint8)
    bits = "111111111" + "000000000" + "101010101" + "1111" + "0000" + "000000001" + "000000000" + "111111111"
    assert len(bits) == 62
    c = dm.census(patch)
    assert c.dtype == np.uint64 and c.shape == (7, 9)
    assert int(c[3, 4]) == int(bits, 2)


def test_census_border_is_clamped():
    y, x = np.mgrid[0:40, 0:40]
    ramp = (3 * x + 2 * y).astype(np.uint8)
    c = dm.census(ramp)
    assert int(c[0, 0]) == 0                                           # every clamped neighbour is >= the corner
    want = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx or dy:
                want = (want << 1) | int(dy < 0 or dx < 0)             # clamped to the corner itself unless above or left of it
    assert int(c[39, 39]) == want
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (40, 40), dtype=np.uint8)
    c = dm.census(img)
    for yy, xx in ((0, 0), (0, 39), (39, 0), (39, 39), (2, 3), (37, 36), (20, 20), (3, 4), (0, 17), (22, 39)):
        assert int(c[yy, xx]) == _census_by_definition(img, yy, xx), (yy, xx)


def test_cost_is_hamming_distance_and_63_outside():
    rng = np.random.default_rng(1)
    L, R = rng.integers(0, 256, (2, 40, 40), dtype=np.uint8)
    cl, cr = dm.census(L), dm.census(R)
    C = dm.cost_volume(cl, cr, 8)
    assert C[5, 3, 4] == 63 and C[5, 3, 7] == 63 and C[0, 0, 1] == 63
    assert C[5, 9, 4] == bin(int(cl[5, 9]) ^ int(cr[5, 5])).count("1") and C[7, 3, 3] == bin(int(cl[7, 3]) ^ int(cr[7, 0])).count("1")
    assert C.max() <= 63


TOY_C = np.array([[[2, 5, 1, 4], [3, 0, 6, 2], [1, 1, 1, 1], [0, 7, 7, 0], [5, 5, 0, 9]]], dtype=np.uint8)   # 1 x 5, D = 4
TOY_L = np.array([[[2, 5, 1, 4], [4, 1, 6, 3], [2, 1, 2, 3], [1, 7, 8, 2], [5, 6, 2, 10]]], dtype=np.uint8)  # P1 = 1, P2 = 3, by hand


def test_recurrence_on_a_toy_evaluated_by_hand():
    assert np.array_equal(dm.path_volume_from_cost(TOY_C, 0, 1, 3), TOY_L)
    assert np.array_equal(dm.path_volume_from_cost(TOY_C, (1, 0), 1, 3), TOY_L)
    # the opposite direction is the same walk over the mirrored row
    assert np.array_equal(dm.path_volume_from_cost(TOY_C[:, ::-1], 1, 1, 3), TOY_L[:, ::-1])
    # on one row a vertical or diagonal path never has a predecessor: L = C
    for k in range(2, 8):
        assert np.array_equal(dm.path_volume_from_cost(TOY_C, k, 1, 3), TOY_C), k
    # a column walks like a row
    col = np.ascontiguousarray(TOY_C.transpose(1, 0, 2))
    assert np.array_equal(dm.path_volume_from_cost(col, 2, 1, 3), TOY_L.transpose(1, 0, 2))
    # and a diagonal of a 5 x 5 image whose diagonal carries the toy
    C = np.full((5, 5, 4), 9, dtype=np.uint8)
    for i in range(5):
        C[i, i] = TOY_C[0, i]
    Ld = dm.path_volume_from_cost(C, 4, 1, 3)
    assert np.array_equal(np.stack([Ld[i, i] for i in range(5)])[None], TOY_L)


def test_a_path_value_fits_a_byte_at_p2_192():
    C = np.zeros((1, 5, 4), dtype=np.uint8)
    C[:, :, 1:] = 63
    L = dm.path_volume_from_cost(C, 0, 192, 192)
    assert L.dtype == np.uint8 and L.max() == 255 and L[0, 4, 3] == 255    # 63 + P2, reached
    dm.DenseParams(p2=192).check()
    with pytest.raises(AssertionError):
        dm.DenseParams(p2=193).check()
    with pytest.raises(AssertionError):
        dm.path_volume_from_cost(C, 0, 193, 193)                            # 63 + 193 = 256
    with pytest.raises(AssertionError):
        dm.DenseParams(p1=0).check()
    with pytest.raises(AssertionError):
        dm.DenseParams(p1=9, p2=8).check()


def test_sub_pixel_step_is_a_floor_division():
    assert dm.floor_div(-130, 60) == -3 and dm.floor_div(130, 60) == 2 and dm.floor_div(-120, 60) == -2
    S = np.full((1, 8, 4), 500, dtype=np.uint16)
    S[0, 5] = [10, 0, 20, 50]        # d0 = 1, den = 30, numerator = (10 - 20) * 16 + 30 = -130: floor(-130 / 60) = -3 (C truncates to -2)
    S[0, 6] = [20, 0, 10, 50]        # numerator 190: floor(190 / 60) = 3
    S[0, 7] = [0, 0, 0, 50]          # den = max(0, 1) = 1, numerator 1: 0
    out = dm.disparity_from_sum(S, dm.DenseParams(disparities=4, lr_tolerance=-1))
    assert out[0, 5] == 16 - 3 and out[0, 6] == 16 + 3
    assert out[0, 7] == dm.INVALID   # the first minimum is d0 = 0
    # uniqueness: a rival two away within the margin invalidates, a neighbour does not
    S[0, 5] = [10, 1, 1, 1]
    assert dm.disparity_from_sum(S, dm.DenseParams(disparities=4, lr_tolerance=-1))[0, 5] == dm.INVALID
    S[0, 5] = [10, 1, 1, 2]
    assert dm.disparity_from_sum(S, dm.DenseParams(disparities=4, lr_tolerance=-1))[0, 5] == 16 + dm.floor_div((10 - 1) * 16 + 9, 18)


def test_right_disparity_and_the_left_right_check():
    S = np.full((1, 8, 4), 500, dtype=np.uint16)
    S[0, 5, 2] = 3                   # left pixel 5 picks d = 2: right pixel 3
    S[0, 4, 1] = 3                   # left pixel 4 picks d = 1: right pixel 3 too, and the smaller d wins the tie there
    dR = dm.right_disparity_from_sum(S)
    assert dR[0, 3] == 1 and dR[0, 7] == 0
    loose = dm.disparity_from_sum(S, dm.DenseParams(disparities=4, lr_tolerance=1, uniqueness=0))
    tight = dm.disparity_from_sum(S, dm.DenseParams(disparities=4, lr_tolerance=0, uniqueness=0))
    assert loose[0, 5] > 0 and loose[0, 4] > 0 and tight[0, 5] == dm.INVALID and tight[0, 4] > 0


def test_flat_and_identical_images_are_all_invalid():
    flat = np.full((40, 48), 90, dtype=np.uint8)
    L, _, _ = make_stereo_pair(seed=2, h=40, w=48, n_blobs=20, bf=60.0)
    for D in (64, 128):
        assert np.all(dm.disparity(flat, flat, dm.DenseParams(disparities=D)) == dm.INVALID)
        assert np.all(dm.disparity(L, L, dm.DenseParams(disparities=D)) == dm.INVALID)


@pytest.mark.parametrize("bf,D,paths", [(200.0, 64, 8), (200.0, 64, 4), (386.0, 128, 8)])
def test_the_model_is_a_stereo_matcher(bf, D, paths):
    """valid fraction and fraction of valid pixels more than 1 px off the generator's truth (a map in right-image coordinates):
    0.960 / 0.036, 0.956 / 0.038, 0.923 / 0.039 for the three cases"""
    L, R, truth = make_stereo_pair(seed=1, h=96, w=320, n_blobs=263, bf=bf)
    prm = dm.DenseParams(disparities=D, paths=paths)
    S = dm.sum_volume(L, R, prm)
    out = dm.disparity_from_sum(S, prm)
    valid = out > 0
    ys, xs = np.nonzero(valid)
    d0 = S.argmin(axis=2)[ys, xs]
    off = np.abs(out[ys, xs] / 16.0 - truth[ys, xs - d0]) > 1.0
    print(f"bf {bf} D {D} paths {paths}: valid {valid.mean():.3f}, > 1 px off {off.mean():.3f}")
    assert valid.mean() >= 0.90 and off.mean() <= 0.06
