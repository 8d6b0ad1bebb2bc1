"""GPU: ssx_stereo_dense (csrc/dense.hip) writes the bits of its contract, tools/dense_model.py -- array_equal, no tolerance: every
value of census + semi-global matching is a small integer.  On a mismatch the stage taps (census, one direction's L, S, dR) are
compared with the model's stages in order and the first that differs is named.

The shapes are the smallest that reach each way the kernels can go wrong: cols < D (lanes whose x - d < 0 for a whole row; also the
smallest legal image), true disparities past the range (winners on D-2 / D-1), two disparities per lane and the d = 63 | 64 seam
(D = 128), an odd width with pitched inputs and a pitch of its own for the map, more than one block everywhere."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import dense as dn
from tools import dense_model as dm
from tools.synth import make_stereo_pair

pytestmark = pytest.mark.gpu

# name: (rows, cols, D, bf, seed, blobs)
SHAPES = {
    "smallest_cols_below_D": (40, 48, 64, 60.0, 2, 20),
    "past_the_range": (64, 200, 64, 1200.0, 8, 110),
    "two_per_lane": (96, 320, 128, 386.0, 1, 263),
    "odd": (41, 67, 64, 90.0, 4, 30),
}
_pairs, _want = {}, {}


def _pair(name):
    if name not in _pairs:
        rows, cols, _, bf, seed, blobs = SHAPES[name]
        L, R, _ = make_stereo_pair(seed=seed, h=rows, w=cols, n_blobs=blobs, bf=bf)
        L.setflags(write=False); R.setflags(write=False)
        _pairs[name] = (L, R)
    return _pairs[name]


def _key(prm):
    return (prm.disparities, prm.p1, prm.p2, prm.uniqueness, prm.lr_tolerance, prm.paths)


def _model(name, L, R, prm):
    """the model's map, computed once per (images, parameters)"""
    k = (name,) + _key(prm)
    if k not in _want:
        out = dm.disparity(L, R, dm.DenseParams(*_key(prm)))
        out.setflags(write=False)
        _want[k] = out
    return _want[k]


def _first_differing_stage(ctx, L, R, prm):
    mp = dm.DenseParams(*_key(prm))
    for direction in range(prm.paths):
        got = dn.stages(ctx, np.ascontiguousarray(L), np.ascontiguousarray(R), prm, direction=direction)
        if direction == 0:
            cl, cr = dm.census(L), dm.census(R)
            if not (np.array_equal(got["census_left"], cl) and np.array_equal(got["census_right"], cr)):
                return "census"
            Cv = dm.cost_volume(cl, cr, prm.disparities)
        if not np.array_equal(got["path_volume"], dm.path_volume_from_cost(Cv, direction, prm.p1, prm.p2)):
            return f"path volume L of direction {direction} {dm.DIRECTIONS[direction]}"
    S = dm.sum_volume_from_cost(Cv, mp)
    if not np.array_equal(got["sum_volume"], S):
        return "sum volume S"
    if not np.array_equal(got["right_disparity"], dm.right_disparity_from_sum(S)):
        return "right disparity dR"
    return "the left disparity (k_dense_select); every stage before it equals the model"


def _check(ctx, name, L, R, prm, got=None):
    want = _model(name, L, R, prm)
    if got is None:
        got = dn.dense_disparity(ctx, L, R, prm)
    if not np.array_equal(got, want):
        bad = int((got != want).sum())
        pytest.fail(f"{name} {_key(prm)}: {bad} of {want.size} pixels differ from the model; first differing stage: {_first_differing_stage(ctx, L, R, prm)}")
    return want


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", ["smallest_cols_below_D", "past_the_range", "two_per_lane"])
def test_equals_the_model(ctx, name, paths):
    L, R = _pair(name)
    prm = dn.DenseParams(disparities=SHAPES[name][2], paths=paths)
    want = _check(ctx, name, L, R, prm)
    # the case is what its name says
    if name == "past_the_range" and paths == 8:
        S = dm.sum_volume(L, R, dm.DenseParams(*_key(prm)))
        d0 = S.argmin(axis=2)
        assert (d0 == 62).sum() > 10 and (d0 == 63).sum() > 10 and (want == dm.INVALID).mean() > 0.3
    if name == "two_per_lane" and paths == 8:
        assert (want > 0).mean() > 0.9


def test_winners_on_both_sides_of_the_lane_seam(ctx):
    """D = 128: three bands of rows shifted by 63, 64 and 65 pixels, so the winners and the sub-pixel neighbours they read lie on both
    sides of d = 63 | 64 (the generator's scenes have next to no disparity that large)"""
    L, _ = _pair("past_the_range")
    L = L[:48]
    rows, cols = L.shape
    R = np.empty_like(L)
    for band, sh in enumerate((63, 64, 65)):
        ys = slice(16 * band, 16 * band + 16)
        R[ys, :cols - sh] = L[ys, sh:]
        R[ys, cols - sh:] = L[ys, cols - 1:]
    want = _check(ctx, "seam", L, R, dn.DenseParams(disparities=128))
    for band, sh in enumerate((63, 64, 65)):
        inner = want[16 * band + 5:16 * band + 11, 80:-8]
        assert ((inner[inner > 0] + 8) >> 4 == sh).all() and (inner > 0).mean() > 0.9, sh


def test_pitched_inputs_and_a_pitch_of_its_own_for_the_map(ctx):
    name = "odd"
    L0, R0 = _pair(name)
    rows, cols = L0.shape
    Lb, Rb = np.full((rows, 80), 0xAB, dtype=np.uint8), np.full((rows, 72), 0xCD, dtype=np.uint8)
    Lb[:, :cols] = L0; Rb[:, :cols] = R0
    prm = dn.DenseParams(disparities=64)
    got = dn.dense_disparity_batch(ctx, [(Lb[:, :cols], Rb[:, :cols])], prm, disp_stride=75)[0]
    assert got.strides[0] == 150 and np.all(got.base[:, cols:] == 0x5a5a)        # the pitch elements stay untouched
    _check(ctx, name, L0, R0, prm, got=got)


EXTREMES = {
    "p1_1_p2_192": dict(p1=1, p2=192),
    "p1_equals_p2": dict(p1=30, p2=30),
    "uniqueness_0": dict(uniqueness=0),
    "uniqueness_99": dict(uniqueness=99),
    "lr_off": dict(lr_tolerance=-1),
    "lr_0": dict(lr_tolerance=0),
}


@pytest.mark.parametrize("case", list(EXTREMES))
def test_parameter_extremes(ctx, case):
    name = "past_the_range"
    L, R = _pair(name)
    _check(ctx, name, L, R, dn.DenseParams(disparities=64, **EXTREMES[case]))
    if case in ("p1_1_p2_192", "lr_off"):                                         # and with two disparities per lane
        L, R = _pair("two_per_lane")
        _check(ctx, "two_per_lane", L, R, dn.DenseParams(disparities=128, **EXTREMES[case]))


def test_flat_saturated_and_identical_images_are_all_invalid(ctx):
    rows, cols = 40, 48
    flat = np.full((rows, cols), 77, dtype=np.uint8)
    sat = np.full((rows, cols), 255, dtype=np.uint8)
    L, _ = _pair("smallest_cols_below_D")
    for D in (64, 128):
        prm = dn.DenseParams(disparities=D)
        for nm, a, b in (("flat", flat, flat), ("saturated", sat, sat), ("identical", L, L)):
            got = dn.dense_disparity(ctx, a, b, prm)
            want = _model(nm, a, b, prm)
            assert np.array_equal(got, want), (nm, D, _first_differing_stage(ctx, a, b, prm))
            assert np.all(want == dm.INVALID), (nm, D)


def test_a_shift_of_five_pixels(ctx):
    """right(u) = left(u + 5): in the interior C(., 5) = 0 on every path, so S(5) = 0 and d0 = 5 -- the map is 80 up to the sub-pixel
    step.  That step is round(8 (S(4) - S(6)) / (S(4) + S(6))) by the contract's formula, which is 0 only where the two neighbours
    cost about the same: the model gives exactly 80 on 30 % of the interior and 74 .. 86 on the rest, and the device must give the
    model's value everywhere."""
    L, _ = _pair("two_per_lane")
    L = L[:64, :200]
    rows, cols = L.shape
    R = np.empty_like(L)
    R[:, :cols - 5] = L[:, 5:]                                                    # right(u) = left(u + 5)
    R[:, cols - 5:] = L[:, cols - 1:]
    prm = dn.DenseParams(disparities=64)
    want = _check(ctx, "shift5", L, R, prm)
    inner = want[8:-8, 24:-24]
    assert (inner > 0).mean() > 0.99 and ((inner[inner > 0] + 8) >> 4 == 5).all() and (inner == 80).mean() > 0.2


def _three(rows=41, cols=67):
    out = []
    for seed, bf in ((4, 90.0), (5, 40.0), (6, 200.0)):
        L, R, _ = make_stereo_pair(seed=seed, h=rows, w=cols, n_blobs=30, bf=bf)
        out.append((L, R))
    return out


def test_three_jobs_in_one_call_equal_three_single_calls(ctx):
    pairs = _three()
    prm = dn.DenseParams(disparities=64)
    singles = [dn.dense_disparity(ctx, L, R, prm) for L, R in pairs]
    _check(ctx, "odd", *pairs[0], prm, got=singles[0])                            # (seed 4 is the "odd" pair)
    got = dn.dense_disparity_batch(ctx, pairs, prm)
    st = dn.last_call(ctx)
    assert st["syncs"] == 1 and st["groups"] == 1 and st["launches"] == 6
    assert st["bytes_down"] == 3 * 2 * 41 * 67
    for k in range(3):
        assert np.array_equal(got[k], singles[k]), k
    assert not np.array_equal(singles[0], singles[1])


def test_three_jobs_on_device_tensors(ctx):
    import torch
    pairs = _three()
    prm = dn.DenseParams(disparities=64)
    singles = [dn.dense_disparity(ctx, L, R, prm) for L, R in pairs]
    dev = [(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()) for L, R in pairs]
    got = dn.dense_disparity_batch(ctx, dev, prm, on_device=True)
    st = dn.last_call(ctx)
    assert st["bytes_down"] == 0 and st["syncs"] == 1 and st["launches"] == 6
    for k in range(3):
        assert np.array_equal(got[k].cpu().numpy(), singles[k]), k


def test_three_jobs_on_pinned_host_memory(ctx):
    lib = ctx.lib
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    pairs = _three()
    rows, cols = pairs[0][0].shape
    prm = dn.DenseParams(disparities=64)
    singles = [dn.dense_disparity(ctx, L, R, prm) for L, R in pairs]
    ls, ds = 72, 70                                                               # pitches: bytes for the images, elements for the map
    per = 2 * rows * ls + 2 * rows * ds
    p = lib.ssx_host_alloc(3 * per)
    assert p
    try:
        arena = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(3 * per,))
        arena[:] = 0xAB
        jobs = []
        for k, (L, R) in enumerate(pairs):
            base = k * per
            arena[base:base + rows * ls].reshape(rows, ls)[:, :cols] = L
            arena[base + rows * ls:base + 2 * rows * ls].reshape(rows, ls)[:, :cols] = R
            jobs.append((p + base, ls, p + base + rows * ls, ls, p + base + 2 * rows * ls, ds))
        dn.dense_ptrs(ctx, jobs, rows, cols, prm, images_on_device=True)
        assert dn.last_call(ctx)["bytes_down"] == 0
        for k in range(3):
            d = arena[k * per + 2 * rows * ls:(k + 1) * per].view(np.int16).reshape(rows, ds)
            assert np.array_equal(d[:, :cols], singles[k]), k
            assert np.all(d[:, cols:].view(np.uint8) == 0xAB), k
    finally:
        lib.ssx_host_free(p)


def test_two_calls_with_different_D_on_one_context(ctx):
    """workspace reuse: the volume of the first call is larger than, then smaller than, the second's"""
    L, R = _pair("two_per_lane")
    for D in (128, 64, 128):
        _check(ctx, "two_per_lane", L, R, dn.DenseParams(disparities=D))
