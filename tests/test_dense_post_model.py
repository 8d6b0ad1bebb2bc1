"""CPU: the contract of the speckle filter and the keyframe's samples (tools/dense_post_model.py) -- against a flood fill written
here, hand-evaluated toys, its own invariants, tools/dense_model.py's cloud_samples, and as a filter of the model's maps."""
from collections import deque

import numpy as np
import pytest

from dense_post_cases import made_maps
from tools import dense_model as dm
from tools import dense_post_model as pm
from tools.synth import make_stereo_pair


def _flood(disp, rng):
    """independent of the model's union-find: a breadth-first fill from every unvisited valid pixel, in raster order"""
    rows, cols = disp.shape
    d = disp.astype(np.int64)
    size = np.zeros((rows, cols), dtype=np.int32)
    root = np.full((rows, cols), -1, dtype=np.int32)
    for y0 in range(rows):
        for x0 in range(cols):
            if d[y0, x0] <= 0 or root[y0, x0] >= 0:
                continue
            seed = y0 * cols + x0                                 # raster order: the first pixel met is the smallest index
            root[y0, x0] = seed
            q, members = deque([(y0, x0)]), [(y0, x0)]
            while q:
                y, x = q.popleft()
                for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= ny < rows and 0 <= nx < cols and root[ny, nx] < 0 and d[ny, nx] > 0 and abs(d[ny, nx] - d[y, x]) <= rng:
                        root[ny, nx] = seed
                        q.append((ny, nx))
                        members.append((ny, nx))
            for y, x in members:
                size[y, x] = len(members)
    return size, root


def _check_against_flood(disp, rng, sizes):
    size, root = pm.components(disp, rng)
    fs, fr = _flood(disp, rng)
    assert size.dtype == np.int32 and root.dtype == np.int32
    assert np.array_equal(size, fs) and np.array_equal(root, fr)
    for s in sizes:
        got = pm.filter_speckles(disp, s, rng)
        want = np.where((disp > 0) & (fs <= s), pm.INVALID, disp) if s > 0 else disp
        assert got.dtype == np.int16 and np.array_equal(got, want), s
        # survivors keep their values, nothing that was not valid changes, and a second pass changes nothing
        assert np.array_equal(got[disp <= 0], disp[disp <= 0]) and np.all((got == disp) | (got == pm.INVALID))
        assert np.array_equal(pm.filter_speckles(got, s, rng), got)
    return size, root


@pytest.mark.parametrize("shape", [(40, 48), (41, 67), (50, 150)])
def test_made_maps_against_a_flood_fill(shape):
    maps = made_maps(*shape)
    assert len(maps) == 10
    for name, (m, rng, sizes) in maps.items():
        size, root = _check_against_flood(m, rng, sizes + [0])
        pix = m.size
        if name in ("constant", "ramp_at_range"):
            assert np.all(size == pix) and np.all(root == 0)
            assert np.array_equal(pm.filter_speckles(m, pix - 1, rng), m) and np.all(pm.filter_speckles(m, pix, rng) == pm.INVALID)
        if name == "checkerboard":
            assert set(np.unique(size)) == {0, 1}
        if name in ("serpentine", "comb"):
            assert np.all(size[m > 0] == (m > 0).sum()) and np.all(root[m > 0] == 0)
        if name == "ramp_past_range":
            assert np.all(size == shape[0]) and np.array_equal(root[5], np.arange(shape[1]))
        if name == "no_wrap":
            assert size.sum() == 2 and size.max() == 1
        if name == "blobs":
            out = pm.filter_speckles(m, sizes[0], rng)
            assert sorted(set(size[m > 0])) == [49, 50, 51] and (out > 0).sum() == 51
        if name == "extremes":
            assert list(size[20, 10:18]) == [1, 0, 1, 0, 1, 0, 2, 2] and size[21, 11] == 1


def test_random_maps_against_a_flood_fill():
    rng = np.random.default_rng(7)
    for k in range(6):
        rows, cols = int(rng.integers(5, 30)), int(rng.integers(5, 30))
        m = rng.integers(-20, 60, size=(rows, cols)).astype(np.int16)
        _check_against_flood(m, int(rng.integers(0, 12)), [0, 1, 2, 5, rows * cols])


def test_hand_evaluated_toys():
    I = pm.INVALID
    m = np.array([[10, 12, I, 50, 50],
                  [I, 14, I, I, 50],
                  [30, 16, 0, 90, I],
                  [30, I, -1, 92, 94],
                  [31, 33, 35, I, 96]], dtype=np.int16)
    size, root = pm.components(m, 2)
    # the ramp 10 12 14 16 is one component although 16 - 10 > 2; 30 30 31 33 35 another; 90 92 94 96; 50 50 50
    assert np.array_equal(size, [[4, 4, 0, 3, 3], [0, 4, 0, 0, 3], [5, 4, 0, 4, 0], [5, 0, 0, 4, 4], [5, 5, 5, 0, 4]])
    assert np.array_equal(root, [[0, 0, -1, 3, 3], [-1, 0, -1, -1, 3], [10, 0, -1, 13, -1], [10, -1, -1, 13, 13], [10, 10, 10, -1, 13]])
    assert np.array_equal(pm.filter_speckles(m, 3, 2), np.where(size == 3, I, m))
    assert np.array_equal(pm.filter_speckles(m, 4, 2), np.where((size == 3) | (size == 4), I, m))
    assert np.array_equal(pm.filter_speckles(m, 0, 2), m)
    # range 0 joins equal values only
    size0, _ = pm.components(m, 0)
    assert np.array_equal(size0, [[1, 1, 0, 3, 3], [0, 1, 0, 0, 3], [2, 1, 0, 1, 0], [2, 0, 0, 1, 1], [1, 1, 1, 0, 1]])
    # the last pixel of a row and the first of the next do not join
    w = np.full((5, 5), I, dtype=np.int16)
    w[1, 4] = w[2, 0] = 40
    assert pm.components(w, 16)[0].sum() == 2


def test_min_disp16_is_the_first_disparity_within_the_depth():
    for bf, z in [(25.0, 40.0), (386.1448, 40.0), (200.0, 10.0), (379.8145, 0.0001), (1.0, 1e9), (60.0, 0.03), (2047.9375, 1.0), (2048.0, 1.0), (2048.0001, 1.0)]:
        ok = np.float64(bf) * 16.0 / np.arange(1, 32768, dtype=np.float64) <= np.float64(z)
        want = int(np.argmax(ok)) + 1 if ok.any() else 32768
        assert pm.min_disp16(bf, z) == want, (bf, z)
    assert pm.min_disp16(25.0, 40.0) == 10 and pm.min_disp16(1.0, 1e9) == 1 and pm.min_disp16(379.8145, 0.0001) == 32768


SWEEP = [(25.0, 40.0), (25.0, 39.999), (386.1448, 40.0), (200.0, 10.0), (200.0, 1e9), (200.0, 1e-3), (60.0, 3.7)]


def test_samples_equal_the_dense_models_cloud_samples():
    rng = np.random.default_rng(3)
    disp = rng.integers(-20, 400, size=(41, 67)).astype(np.int16)
    disp[4, 8] = 10                                               # bf = 25, max_depth = 40: z = 25 * 16 / 10 = 40 exactly, a tie that passes
    disp[8, 4] = 9
    left = rng.integers(0, 256, size=(41, 67)).astype(np.uint8)
    for stride in (1, 3, 4, 7):
        for bf, z in SWEEP:
            want = dm.cloud_samples(disp, left, stride, bf, z)
            got = pm.samples(disp, left, stride, pm.min_disp16(bf, z))
            assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (stride, bf, z)
    tie = pm.samples(disp, left, 4, pm.min_disp16(25.0, 40.0))
    assert [4 * 2, 4, 10, int(left[4, 8])] in tie.tolist() and not any(r[2] == 9 for r in tie.tolist())
    assert len(pm.samples(disp, left, 4, pm.min_disp16(200.0, 1e9))) == (disp[::4, ::4] > 0).sum()     # a bar below every disparity
    assert len(pm.samples(disp, left, 4, pm.min_disp16(200.0, 1e-3))) == 0                               # and one above all of them


def test_postprocess_is_the_filter_then_the_samples_of_the_filtered_map():
    m, rng, _ = made_maps(41, 67)["random"]
    left = np.random.default_rng(5).integers(0, 256, size=m.shape).astype(np.uint8)
    post = pm.DensePost(speckle_size=20, speckle_range=rng, cloud_stride=3, cloud_min_disp16=105)
    out, smp = pm.postprocess(m, left, post)
    assert np.array_equal(out, pm.filter_speckles(m, 20, rng)) and np.array_equal(smp, pm.samples(out, left, 3, 105))
    assert len(smp) < len(pm.samples(m, left, 3, 105))
    assert pm.postprocess(m, left, pm.DensePost())[1] is None and np.array_equal(pm.postprocess(m, left, pm.DensePost())[0], m)


# the three cases of test_dense_model.py::test_the_model_is_a_stereo_matcher
MATCHER_CASES = [(200.0, 64, 4), (200.0, 64, 8), (386.0, 128, 8)]


@pytest.mark.parametrize("bf,D,paths", MATCHER_CASES)
def test_the_filter_does_not_hurt_the_matcher(bf, D, paths):
    """size 100 / range 16 on the seed-1 pair: the valid pixels more than 1 px off the truth do not grow in number and the valid share
    falls by less than 0.02.  Measured (bad before -> after, valid share before -> after):
        bf 200 / D  64 / 4 paths:  1118 -> 1059,  0.956 -> 0.953
        bf 200 / D  64 / 8 paths:  1069 -> 1000,  0.960 -> 0.956
        bf 386 / D 128 / 8 paths:  1102 ->  918,  0.923 -> 0.916"""
    L, R, truth = make_stereo_pair(seed=1, h=96, w=320, n_blobs=263, bf=bf)
    prm = dm.DenseParams(disparities=D, paths=paths)
    S = dm.sum_volume(L, R, prm)
    disp = dm.disparity_from_sum(S, prm)
    out = pm.filter_speckles(disp, 100, 16)
    d0 = S.argmin(axis=2)

    def bad_and_share(d):
        ys, xs = np.nonzero(d > 0)                                # (the truth is a map in right-image coordinates)
        return int((np.abs(d[ys, xs] / 16.0 - truth[ys, xs - d0[ys, xs]]) > 1.0).sum()), float((d > 0).mean())

    b0, s0 = bad_and_share(disp)
    b1, s1 = bad_and_share(out)
    print(f"bf {bf:g} / D {D} / {paths} paths: bad {b0} -> {b1}, valid share {s0:.3f} -> {s1:.3f}")
    assert b1 <= b0 and s0 - s1 < 0.02
