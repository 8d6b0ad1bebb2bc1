"""CPU: the inputs of tests/lk_image_cases.py are what their names say, shown with the CPU oracle (oracle/src/lk_oracle.cpp) and the
plan hook (ssx_lk_debug_plan) alone -- no device.  tests/test_lk_images_gpu.py compares the device with the oracle on the same inputs;
what is asserted here is that those comparisons reach the code they are meant for:

  A  the level lists of the table, from the halving rule, from the oracle's pyramid and from the plan; which pyramid builder the plan
     gives a call of one job and of 17; a level no larger than the border where the name says so
  B  at least 15 of 45 points end with status 1 and a displacement whose larger component exceeds margin + 1 pixels.  k_lk_track's
     region_holds is true only while |floor(n) - floor(n at the level's start)| <= margin, so each of these points had its
     neighbourhood copied again at least once: the coverage is inferred from this bound, nothing is counted on the device
  C  maxCount 0 keeps points with status 1, an error above zero and the guess as the result; epsilon 0 and 10 give different results;
     values outside the clamps give the bytes of the clamped ones
  D  the points kept per texture and threshold; the diagonal stripes at threshold 0 leave the image
  G  every non-finite or out-of-range coordinate is refused with status 0, the ordinary points beside them are untouched"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_image_cases as ic  # noqa: E402

from ssvio_amd import _lib, lk  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@functools.lru_cache(maxsize=None)
def track(family, name, **kw):
    """the oracle on frames[0] -> frames[1] of a case, once per (case, parameters)"""
    from oracle import pyoracle as po
    po.build()
    c = {"geometry": ic.geometry_case, "step": ic.step_case, "limit": ic.limit_case, "texture": ic.texture_case}[family](name)
    guess = c.get("guess", c["pts"] if family in ("geometry", "texture") else None)
    prm = po.lk_params(win=c.get("win", 11), max_level=c.get("max_level", 3), use_initial_flow=int(guess is not None), **kw)
    return po.lk_track(c["frames"][0], c["frames"][1], c["pts"], guess, prm=prm)


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", list(ic.GEOMETRY))
def test_geometry_case_has_the_levels_and_the_builder_of_the_table(po, lib, name):
    c = ic.geometry_case(name)
    rows, cols, win = c["level_rows"], c["level_cols"], c["win"]
    assert ic.levels(c["rows"], c["cols"], win, c["max_level"]) == (rows, cols)
    o = track("geometry", name)
    assert o[3] == len(rows) - 1
    img = c["frames"][0]
    for l in range(len(rows)):                                          # the oracle's pyramid, level by level
        if l > 0:
            img = po.lk_pyr_down(img)
        assert img.shape == (rows[l], cols[l])
    if len(rows) <= c["max_level"]:                                     # cut short: the next level would not be larger than the window
        assert min((rows[-1] + 1) // 2, (cols[-1] + 1) // 2) <= win
    p = lk.debug_plan(lib, c["rows"], c["cols"], [dict(slot=0, fresh=True, n=len(c["pts"]))], win=win, max_level=c["max_level"])
    assert p.status == _lib.SSX_OK, p.error
    assert p.levels == len(rows) and list(p.rows[:p.levels]) == rows and list(p.cols[:p.levels]) == cols
    assert bool(p.use_fused) == c["fused"]
    wide = lk.debug_plan(lib, c["rows"], c["cols"], [dict(slot=s_, fresh=True, n=1) for s_ in range(ic.WIDE)], win=win, max_level=c["max_level"])
    assert wide.status == _lib.SSX_OK and not wide.use_fused
    small = min(min(rows), min(cols))
    if name.startswith("fused_limit"):
        assert len(rows) == 4 and min(rows[-1], cols[-1]) == win + 3                         # border + 2: the last size with one fold per coordinate
    if name.startswith("first_unfused"):
        assert len(rows) == 4 and min(rows[-1], cols[-1]) == win + 2
    if name.startswith("double_fold"):
        assert small == win + 1                                                              # a level as wide as its border: two reflections
    if name.startswith("below_window"):
        assert len(rows) == 1 and small <= win + 1
    if name == "eight_levels":
        assert len(rows) == 8
    assert (o[1] > 0).sum() > 0 or small <= win                        # something is tracked wherever a window fits into the image
    print("\nreach %-20s levels %s x %s, fused %d, kept %d of %d" % (name, rows, cols, p.use_fused, (o[1] > 0).sum(), len(o[1])))


def test_nine_levels_are_refused_by_the_plan(lib):
    p = lk.debug_plan(lib, 700, 800, [dict(slot=0, fresh=True, n=1)], win=5, max_level=8)
    assert p.status == _lib.SSX_ERR_INVALID_ARG and b"max_level 8" in p.error
    assert lk.debug_plan(lib, 700, 800, [dict(slot=0, fresh=True, n=1)], win=5, max_level=7).status == _lib.SSX_OK


# ---------------------------------------------------------------------------------------------------------------- B
def test_step_table_is_the_issue_s():
    assert [ic.margin(w) for w in (3, 5, 11, 15)] == [14, 13, 10, 8]
    for win in (3, 5, 11, 15):
        shifts = sorted(abs(v[1]) for n, v in ic.STEPS.items() if v[0] == win and n.startswith("step_w%d_s" % win))
        assert shifts == [ic.margin(win) + e for e in (1, 3, 6)]
    assert ic.STEPS["step_w11_y_only"][2] == 0 and ic.STEPS["step_w11_opposite"][1] == -ic.STEPS["step_w11_s13"][1]
    assert ic.step_points().shape == (45, 2)
    img = ic.smooth(12.0, 7)
    assert img.shape == (120, 160) and img.min() == 0 and img.max() == 255


@pytest.mark.parametrize("name", list(ic.STEPS))
def test_step_case_moves_points_beyond_the_margin(name):
    c = ic.step_case(name)
    o = track("step", name)
    assert o[3] == 0
    d = o[0] - c["pts"]
    far = (o[1] == 1) & (np.abs(d).max(1) > ic.margin(c["win"]) + 1)
    print("\nreach %-20s shift %s: kept %d, beyond margin + 1: %d, median displacement %s" % (name, c["shift"], (o[1] == 1).sum(), far.sum(),
                                                                                           np.median(d[o[1] == 1], 0)))
    assert far.sum() >= 15
    # ... and they went where the image went: the median of the far points is the shift (window 3 finds other minima on the way, and
    # is held to the count alone)
    if c["win"] > 3:
        assert np.abs(np.median(d[far], 0) - np.array(c["shift"])).max() < 0.05


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", ic.LIMITS)
def test_limit_case_reaches_the_paths(name):
    c = ic.limit_case(name)
    start = c["pts"] if c["guess"] is None else c["guess"]
    zero = track("limit", name, max_iters=0)
    kept = zero[1] == 1
    assert kept.sum() > 0 and (zero[2][kept] > 0).all() and zero[0].tobytes() == start.tobytes()          # no step: the error of the guess
    one, two, many = (track("limit", name, max_iters=k) for k in (1, 2, 100))
    assert not same(zero, one) and not same(one, two) and not same(two, many)
    tight, loose = track("limit", name, eps=0.0), track("limit", name, eps=10.0)
    assert not same(tight, loose)
    moved = lambda r: np.abs(r[0] - start).max(1)[(tight[1] == 1) & (loose[1] == 1)].sum()                # noqa: E731
    assert moved(tight) > moved(loose)
    for k, k_ in ic.CLAMPED_COUNT.items():
        for e in ic.EPSILONS:
            assert same(track("limit", name, max_iters=k, eps=e), track("limit", name, max_iters=k_, eps=ic.CLAMPED_EPS.get(e, e))), (k, e)
    for e, e_ in ic.CLAMPED_EPS.items():
        assert same(track("limit", name, eps=e), track("limit", name, eps=e_)), e
    print("\nreach %-8s maxCount 0 keeps %d of %d, mean err %.3f; epsilon 0 / 10 move %.2f / %.2f px in all" % (name, kept.sum(), len(kept), zero[2][kept].mean(),
                                                                                                           moved(tight), moved(loose)))


# ---------------------------------------------------------------------------------------------------------------- D
KEPT = {"checker_8": (15, 30, 35, 0)}                                   # every other texture: nothing, at every threshold


@pytest.mark.parametrize("name", ic.TEXTURES)
def test_texture_case_keeps_what_the_gate_lets_through(name):
    c = ic.texture_case(name)
    assert c["frames"][0].shape == (96, 128) and len(c["pts"]) == 35
    res = [track("texture", name, min_eig_threshold=th) for th in ic.MIN_EIGS]
    assert all(r[3] == 3 for r in res)
    kept = tuple(int((r[1] == 1).sum()) for r in res)
    far = [float(np.abs(r[0] - c["pts"]).max()) for r in res]
    print("\nreach %-14s kept %s, furthest result %s px from its start" % (name, kept, ["%.1f" % f for f in far]))
    assert kept == KEPT.get(name, (0, 0, 0, 0))
    if name == "stripes_diag":                                          # threshold 0: near-singular systems pass, the iteration leaves the image
        assert far[0] > 80 and (res[0][1] == 0).all()
    if name in ("flat_90", "saturated", "checker_1"):                   # no gradient at any level: nothing moves
        assert max(far) == 0
    if name == "checker_1":
        from oracle import pyoracle as po
        assert not po.lk_scharr(c["frames"][0])[1:-1, 1:-1].any()


# ---------------------------------------------------------------------------------------------------------------- G
def test_coordinate_case_is_refused_point_by_point(po):
    c = ic.coordinate_case()
    good, bad = c["good"], c["bad"]
    rows, cols = c["frames"][0].shape
    assert len(good) == 12 and np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    for v in (1e30, -1e30, 3e9, -3e9, 2147483648.0, -2147483904.0):
        assert (bad == np.float32(v)).any(), v
    assert float(np.float32(2147483648.0)) == 2.0 ** 31 and float(np.float32(-2147483904.0)) == -(2.0 ** 31) - 256     # 2^31 and the float below -2^31
    assert ((bad != 0) & (np.abs(bad) < np.finfo(np.float32).tiny)).any()                   # the denormal
    assert bad[-1, 0] < cols and bad[-1, 1] < rows and bad[-1, 0] > cols - 1.01
    outside = ~np.isfinite(bad).all(1) | (np.abs(bad) > 1e9).any(1)
    assert outside.sum() == len(bad) - 4                                # the denormal beside an ordinary value (twice), with itself, the last sub-pixel
    alone = po.lk_track(c["frames"][0], c["frames"][1], good, good)
    assert (alone[1] == 1).all()
    guess_bad = np.concatenate([good, np.full_like(bad, 60.0)])
    for bad_is_guess, (prev, guess) in enumerate(((np.concatenate([good, bad]), guess_bad), (guess_bad, np.concatenate([good, bad])))):
        o = po.lk_track(c["frames"][0], c["frames"][1], prev, guess)
        assert all(o[k][:12].tobytes() == alone[k].tobytes() for k in range(3))
        assert (o[1][12:][outside] == 0).all() and (o[2][12:][outside] == 0).all()
        if bad_is_guess:
            assert np.isnan(o[0]).any() and np.isinf(o[0]).any()        # both rules of the GPU comparison are used
        else:
            assert o[0][12:][outside].tobytes() == guess[12:][outside].tobytes()             # a refused point keeps its guess
