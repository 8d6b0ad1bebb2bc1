"""GPU parity of the pyramidal LK tracker on the inputs of tests/lk_image_cases.py, BIT FOR BIT against the CPU oracle: pyramid levels,
derivative images, tracked positions (f32 bit patterns), status flags, errors and the level count.

tests/test_lk_gpu.py draws every image with tools.synth.make_stereo_pair and moves it by a pixel or two per level.  These inputs
reach what that leaves out -- the last geometry k_lk_pyramid accepts and the first it must refuse, levels no wider than their border,
eight levels, steps beyond the neighbourhood k_lk_track keeps in LDS, maxCount 0 and the clamps, textures that the minEig / D gate
refuses or, at threshold 0, lets through, and coordinates that are no positions at all.  That each case reaches what its name says is
asserted from the oracle alone in tests/test_lk_image_cases.py; in particular, that the neighbourhood is copied again in family B is
inferred there from how far the points move, not counted on the device.

Tried once on a copy of lk.hip in which the neighbourhood, when it is copied AGAIN inside a level, is read one column off (reads
inside the copy only): 27 of the 43 tests here fail -- all 14 of family B, the step case of family C, every geometry with window 3
or 5, the diagonal stripes and the 8-pixel checkerboard at thresholds 0 and 1e-4, the coordinates.  tests/test_lk_gpu.py notices it
too (11 of 24, through points that wander off near a border and are dropped); family B is where points that are KEPT go through the
second copy and still land on the oracle's bits."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_image_cases as ic  # noqa: E402

from ssvio_amd import _lib, lk  # noqa: E402

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same(g, o):
    """next_pts, status and err byte for byte; the level count where both sides report one"""
    return _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]) and (len(g) < 4 or len(o) < 4 or g[3] == o[3])


@functools.lru_cache(maxsize=None)
def oracle(family, name, first=0, **kw):
    """the oracle on frames[first] -> frames[first + 1] of a case, once per (case, parameters)"""
    from oracle import pyoracle as po
    po.build()
    c = {"geometry": ic.geometry_case, "step": ic.step_case, "limit": ic.limit_case, "texture": ic.texture_case}[family](name)
    guess = c.get("guess", c["pts"] if family in ("geometry", "texture") else None)
    prm = po.lk_params(win=c.get("win", 11), max_level=c.get("max_level", 3), use_initial_flow=int(guess is not None), **kw)
    return po.lk_track(c["frames"][first], c["frames"][first + 1], c["pts"], guess, prm=prm)


def check_images(po, c, prev, nxt, levels, what, derivatives_only=False):
    """slot 0 of context c: every level of both pyramids and the previous image's derivative images against the oracle's"""
    for level in range(levels):
        if level > 0:
            prev, nxt = po.lk_pyr_down(prev), po.lk_pyr_down(nxt)
        if not derivatives_only:
            assert np.array_equal(lk.stage_level(c, 0, level), prev) and np.array_equal(lk.stage_level(c, 1, level), nxt), (what, level)
        assert np.array_equal(lk.stage_deriv(c, level), po.lk_scharr(prev)), (what, "Scharr", level)


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", list(ic.GEOMETRY))
def test_geometry_at_the_limits(po, name):
    """One job on a context of its own: the pyramid builder the table names, every level and derivative image, the result; a chained
    third frame (the derivative images of its previous image were written one call earlier, or are written now); then the same two
    calls as slot 0 of a call of 17 jobs, which the per-level kernels build whatever the geometry: the bytes of the one-job calls."""
    from ssvio_amd import Context
    c = ic.geometry_case(name)
    f0, f1, f2 = c["frames"]
    pts, nlev = c["pts"], len(c["level_rows"])
    kw = dict(winSize=c["win"], maxLevel=c["max_level"])
    o1, o2 = oracle("geometry", name), oracle("geometry", name, first=1)
    one = Context(0)
    try:
        g1 = lk.calcOpticalFlowPyrLK(one, f0, f1, pts, pts, **kw)
        info = lk.last_call(one)
        assert bool(info.use_fused) == c["fused"]
        assert g1[3] == nlev - 1 and (list(info.rows[:nlev]), list(info.cols[:nlev])) == (c["level_rows"], c["level_cols"])
        check_images(po, one, f0, f1, nlev, "fresh")
        assert same(g1, o1)
        g2 = lk.calcOpticalFlowPyrLK(one, None, f2, pts, pts, **kw)
        assert bool(lk.last_call(one).use_fused) == c["fused"]
        check_images(po, one, f1, f2, nlev, "chained")
        assert same(g2, o2)
    finally:
        one.close()
    wide = Context(0)
    try:
        for k, (single, prev, nxt) in enumerate(((g1, f0, f1), (g2, f1, f2))):
            jobs = [dict(slot=0, prev=None if k else f0, next=nxt, prev_pts=pts, next_pts=pts)]
            jobs += [dict(slot=s_, prev=None if k else fr[0], next=fr[k + 1], prev_pts=pts, next_pts=pts) for s_, fr in enumerate(c["others"], 1)]
            assert len(jobs) == ic.WIDE
            got = lk.track_batch(wide, jobs, **kw)
            assert not lk.last_call(wide).use_fused
            check_images(po, wide, prev, nxt, nlev, ("wide", k))
            assert same(got[0], single), ("wide", k)
    finally:
        wide.close()


def test_nine_levels_are_refused_and_the_context_goes_on(po):
    """max_level 8 would be a ninth level: SSX_ERR_INVALID_ARG, on a context that has a chain (which stays) and on a new one"""
    from ssvio_amd import Context
    c = ic.geometry_case("double_fold_w3")
    f0, f1, f2 = c["frames"]
    kw = dict(winSize=c["win"], maxLevel=c["max_level"])
    ctx = Context(0)
    try:
        with pytest.raises(_lib.SsxError) as e:
            lk.calcOpticalFlowPyrLK(ctx, f0, f1, c["pts"], c["pts"], winSize=c["win"], maxLevel=8)
        assert e.value.status == _lib.SSX_ERR_INVALID_ARG and "max_level 8" in str(e.value)
        assert same(lk.calcOpticalFlowPyrLK(ctx, f0, f1, c["pts"], c["pts"], **kw), oracle("geometry", "double_fold_w3"))
        with pytest.raises(_lib.SsxError) as e:
            lk.calcOpticalFlowPyrLK(ctx, f1, f2, c["pts"], c["pts"], winSize=c["win"], maxLevel=8)
        assert e.value.status == _lib.SSX_ERR_INVALID_ARG
        assert same(lk.calcOpticalFlowPyrLK(ctx, None, f2, c["pts"], c["pts"], **kw), oracle("geometry", "double_fold_w3", first=1))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("name", list(ic.STEPS))
def test_steps_beyond_the_staged_region(ctx, name):
    c = ic.step_case(name)
    g = lk.calcOpticalFlowPyrLK(ctx, c["frames"][0], c["frames"][1], c["pts"], None, winSize=c["win"], maxLevel=0)
    assert same(g, oracle("step", name))


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", ic.LIMITS)
def test_iteration_limits_and_their_clamps(ctx, name):
    c = ic.limit_case(name)
    got = {}
    for k in ic.MAX_COUNTS:
        for e in ic.EPSILONS:
            got[k, e] = lk.calcOpticalFlowPyrLK(ctx, c["frames"][0], c["frames"][1], c["pts"], c["guess"], winSize=c["win"], maxLevel=c["max_level"], maxCount=k, epsilon=e)
            assert same(got[k, e], oracle("limit", name, max_iters=k, eps=e)), (k, e)
    for (k, e), g in got.items():                                       # a value outside the clamp IS the clamped one
        assert same(g, got[ic.CLAMPED_COUNT.get(k, k), ic.CLAMPED_EPS.get(e, e)]), (k, e)
    zero = got[0, 0.0]
    assert (zero[1] == 1).any() and (zero[2][zero[1] == 1] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("name", ic.TEXTURES)
def test_degenerate_textures_under_every_threshold(ctx, name):
    c = ic.texture_case(name)
    for th in ic.MIN_EIGS:
        g = lk.calcOpticalFlowPyrLK(ctx, c["frames"][0], c["frames"][1], c["pts"], c["pts"], minEigThreshold=th)
        assert same(g, oracle("texture", name, min_eig_threshold=th)), th


@pytest.mark.parametrize("th", ic.MIN_EIGS)
def test_textures_as_jobs_of_one_call(ctx, th):
    cases = [ic.texture_case(n) for n in ic.TEXTURES]
    got = lk.track_batch(ctx, [dict(slot=s_, prev=c["frames"][0], next=c["frames"][1], prev_pts=c["pts"], next_pts=c["pts"]) for s_, c in enumerate(cases)],
                         minEigThreshold=th)
    for n, c, g in zip(ic.TEXTURES, cases, got):
        assert same(g, lk.calcOpticalFlowPyrLK(ctx, c["frames"][0], c["frames"][1], c["pts"], c["pts"], minEigThreshold=th)), n
        assert same(g, oracle("texture", n, min_eig_threshold=th)), n


# ---------------------------------------------------------------------------------------------------------------- G
def test_coordinates_that_are_no_positions(ctx, po):
    """status and err byte for byte; next_pts byte for byte where the oracle's value is a number or an infinity, NaN where it is NaN
    (the payload of a NaN is not part of the contract); the ordinary points of the call as if the others were not there"""
    c = ic.coordinate_case()
    f0, f1 = c["frames"]
    good, bad = c["good"], c["bad"]
    alone = lk.calcOpticalFlowPyrLK(ctx, f0, f1, good, good)
    assert same(alone, po.lk_track(f0, f1, good, good))
    valid = np.concatenate([good, np.full_like(bad, 60.0)])
    for what, prev, guess in (("bad prev_pts", np.concatenate([good, bad]), valid), ("bad guess", valid, np.concatenate([good, bad]))):
        g = lk.calcOpticalFlowPyrLK(ctx, f0, f1, prev, guess)
        o = po.lk_track(f0, f1, prev, guess)
        assert g[3] == o[3] and _same(g[1], o[1]) and _same(g[2], o[2]), what
        nan = np.isnan(o[0])
        assert g[0].shape == o[0].shape and np.isnan(g[0][nan]).all() and g[0][~nan].tobytes() == o[0][~nan].tobytes(), what
        assert all(_same(g[k][:len(good)], alone[k]) for k in range(3)), what
