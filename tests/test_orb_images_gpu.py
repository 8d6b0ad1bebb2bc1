"""GPU parity of the ORB front-end on the images of tests/orb_image_cases.py, BIT FOR BIT against the CPU oracle: every pyramid
level and blurred level, the grid-FAST candidates of EVERY level (with the oracle's mask level where a mask is set), the outputs of
Detect and DetectAndCompute, ScreenAndComputeKPsParams_CalcDescriptors on keypoints given at the edge of its screen and on halves,
and pitched / unaligned views through Detect, DetectAndCompute, DetectBoxes and DetectBoxesBatch against their contiguous copies.

tests/test_orb_gpu.py draws every image with tools.synth.make_stereo_pair (smooth blobs in mid grey, C-contiguous); what these images
reach instead is counted, case by case, in tests/test_orb_image_cases.py, which also shows that none of them exceeds a capacity.

What this file notices, tried once each on a copy of orb.hip with one line changed (138 tests):
  * NMS `>=` for one neighbour: 54 fail -- candidates and outputs of every noise, checkerboard, tie, mask, pitched and batch case;
  * the left mirror source of gauss_fix_edges off by one: 39 fail -- the blurred levels of every case but the flat and the
    one-dot-per-cell images, four outputs, both describe cases that keep keypoints;
  * the quick test one grey level too strict (`sub_sat(lo, s2 + 1)`): 8 fail -- dots/p4, dots/p2, checker/p1, blobs/saturated;
  * the quick test's saturating `v - t` made a wrapping one: NONE fails, and none can.  The quick test only filters for the full
    segment test; for v < t the wrapped value is huge, the pixel passes the filter and the full test decides as before."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_image_cases as ic  # noqa: E402

from ssvio_amd import orb as sorb  # noqa: E402

pytestmark = pytest.mark.gpu


def extractor(ctx, prm):
    return sorb.ORBextractor(ctx, prm["nfeatures"], prm["scale_factor"], prm["nlevels"], prm["ini_th"], prm["min_th"])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's side of an extract case, computed once: levels, mask levels, blurred levels, candidates per level, outputs"""
    from oracle import pyoracle as po
    po.build()
    case = ic.cases()[name]
    img, prm = np.ascontiguousarray(case["img"]), case["prm"]
    mask = None if case["mask"] is None else np.ascontiguousarray(case["mask"])
    rows, cols = po.level_sizes(img.shape[0], img.shape[1], prm["scale_factor"], prm["nlevels"])
    lv, mk = [img], [mask]
    for l in range(1, prm["nlevels"]):
        lv.append(po.resize_linear(lv[-1], rows[l], cols[l]))
        mk.append(None if mask is None else po.resize_linear(mk[-1], rows[l], cols[l]))
    oprm = po.orb_params(**prm)
    kps, desc = po.orb_extract(img, mask, oprm)
    return dict(levels=lv, masks=mk, blur=[po.gauss7(a) for a in lv], cand=[po.orb_grid_fast(a, m, prm["ini_th"], prm["min_th"]) for a, m in zip(lv, mk)],
                kps=kps, desc=desc, det=po.orb_detect(img, mask, oprm))


def same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ic.names("extract"))
def test_pyramid_and_blur_bit_exact(ctx, name):
    case, o = ic.cases()[name], oracle(name)
    ex = extractor(ctx, case["prm"])
    ex.DetectAndCompute(case["img"], case["mask"])
    for l, (ref, blur) in enumerate(zip(o["levels"], o["blur"])):
        got = ex.stage_level(l)
        assert got.shape == ref.shape and np.array_equal(got, ref), f"pyramid level {l}: {int((got != ref).sum())} pixels differ"
        got = ex.stage_level(l, blurred=True)
        assert np.array_equal(got, blur), f"blurred level {l}: {int((got != blur).sum())} pixels differ"


@pytest.mark.parametrize("name", ic.names("extract"))
def test_candidates_of_every_level_bit_exact(ctx, name):
    case, o = ic.cases()[name], oracle(name)
    ex = extractor(ctx, case["prm"])
    ex.DetectAndCompute(case["img"], case["mask"])
    for l, ref in enumerate(o["cand"]):
        got = ex.stage_candidates(l)
        assert same(got, ref), f"level {l}: {len(got)} candidates, the oracle has {len(ref)}"


@pytest.mark.parametrize("name", ic.names("extract"))
def test_detect_and_extract_bit_exact(ctx, name):
    case, o = ic.cases()[name], oracle(name)
    ex = extractor(ctx, case["prm"])
    gk, gd = ex.DetectAndCompute(case["img"], case["mask"])
    assert len(gk) == len(o["kps"]), (len(gk), len(o["kps"]))
    assert gk.tobytes() == o["kps"].tobytes()           # positions, size, angle (f32), response, octave
    assert np.array_equal(gd, o["desc"])
    assert same(ex.Detect(case["img"], case["mask"]), o["det"])


def boxes_for(img, seed):
    """rectangles as FrontEnd::DetectFeatures makes them (21 x 21 around a point, clipped), and the mask they rasterise to"""
    rng = np.random.default_rng(seed)
    h, w = img.shape
    x, y = rng.integers(0, w, 12), rng.integers(0, h, 12)
    b = np.stack([np.maximum(x - 10, 0), np.maximum(y - 10, 0), np.minimum(x + 10, w - 1), np.minimum(y + 10, h - 1)], 1).astype(np.int32)
    mask = np.full(img.shape, 255, np.uint8)
    for x0, y0, x1, y1 in b:
        mask[y0:y1 + 1, x0:x1 + 1] = 0
    return b, mask


@pytest.mark.parametrize("name", ic.names("pitched"))
def test_pitched_views_equal_their_contiguous_copies(ctx, po, name):
    """a row-strided view at a byte offset into a buffer that ends with its last pixel, through Detect, DetectAndCompute, DetectBoxes and
    ScreenAndComputeKPsParams_CalcDescriptors: level 0 is the image, the results are the contiguous copy's and the oracle's bytes"""
    case = ic.cases()[name]
    view, copy, prm = case["img"], case["contiguous"], case["prm"]
    assert not view.flags["C_CONTIGUOUS"] and sorb._img(view) is view
    oprm = po.orb_params(**prm)
    ex = extractor(ctx, prm)
    vk, vd = ex.DetectAndCompute(view)
    assert np.array_equal(ex.stage_level(0), copy)
    ck, cd = ex.DetectAndCompute(copy)
    ok, od = po.orb_extract(copy, prm=oprm)
    assert len(ok) > 100 and same(vk, ck) and same(vk, ok) and np.array_equal(vd, cd) and np.array_equal(vd, od)
    mview = ic.pitched(ic.stripe_mask(*copy.shape, True), view.strides[0] + 2, 7 - case["offset"])     # a mask with a stride of its own
    vk, vd = ex.DetectAndCompute(view, mview)
    ok, od = po.orb_extract(copy, np.ascontiguousarray(mview), oprm)
    assert len(ok) > 100 and same(vk, ok) and np.array_equal(vd, od)
    od = po.orb_detect(copy, prm=oprm)
    assert len(od) > 100 and same(ex.Detect(view), od) and same(ex.Detect(copy), od)
    boxes, mask = boxes_for(copy, 1)
    om = po.orb_detect(copy, mask, oprm)
    assert len(om) > 50 and same(ex.DetectBoxes(view, boxes), om) and same(ex.DetectBoxes(copy, boxes), om) and same(ex.Detect(view, mask), om)
    rep = np.concatenate([ok[:40]] * prm["nlevels"])
    rep["octave"] = np.repeat(np.arange(prm["nlevels"]), 40)
    gk, gd = ex.ScreenAndComputeKPsParams_CalcDescriptors(view, rep)
    rk, rd = po.orb_describe_at(copy, rep, oprm)
    assert len(rk) > 0 and same(gk, rk) and np.array_equal(gd, rd)


@pytest.mark.parametrize("name", ic.names("batch"))
def test_batch_of_differently_aligned_views(ctx, po, name):
    """DetectBoxesBatch has one pointer per image: four views of one stride at four alignments, in one call and in another order,
    against DetectBoxes on each contiguous copy and against the oracle on the rasterised mask"""
    case = ic.cases()[name]
    views, copies, prm = case["views"], case["contiguous"], case["prm"]
    ex = extractor(ctx, prm)
    bm = [boxes_for(a, 10 + k) for k, a in enumerate(copies)]
    want = [po.orb_detect(a, m, po.orb_params(**prm)) for a, (_, m) in zip(copies, bm)]
    for sel in ([0, 1, 2, 3], [3, 1, 0], [2]):
        got = ex.DetectBoxesBatch([views[i] for i in sel], [bm[i][0] for i in sel])
        for i, g in zip(sel, got):
            assert len(want[i]) > 50 and same(g, want[i]), (sel, i)
    for i in range(4):
        assert same(ex.DetectBoxes(copies[i], bm[i][0]), want[i])
    # views of different strides: the wrapper hands the call contiguous copies
    mixed = [views[0], copies[1], ic.pitched(copies[2], copies[2].shape[1] + 8, 3)]
    for i, g in enumerate(ex.DetectBoxesBatch(mixed, [bm[i][0] for i in range(3)])):
        assert same(g, want[i]), i


@pytest.mark.parametrize("name", ic.names("describe"))
def test_describe_at_the_screen_and_on_halves(ctx, po, name):
    case = ic.cases()[name]
    img, prm, kin = case["img"], case["prm"], case["kps"]
    ok, od = po.orb_describe_at(img, kin, po.orb_params(**prm))
    gk, gd = extractor(ctx, prm).ScreenAndComputeKPsParams_CalcDescriptors(img, kin)
    assert len(gk) == len(ok), (len(gk), len(ok))
    assert np.array_equal(gk["class_id"], ok["class_id"])                 # the same keypoints pass the screen, in the given order
    assert gk.tobytes() == ok.tobytes() and np.array_equal(gd, od)
    assert (len(ok) == 0) == (prm["min_th"] == 255)


@pytest.mark.parametrize("cols,stride,offset", [(163, 168, 0), (161, 164, 3), (167, 167, 1)])
def test_pitched_images_on_the_device(ctx, cols, stride, offset):
    """ssx_stereo_batch_dev reads the caller's device images with their row stride: k_copy_level0's 8-byte loads (pointer, stride and
    image size multiples of 8: they run into the row padding) and its aligned dwords cut at any byte offset, clamped to the dword of the
    input's last byte -- here the last byte of the buffer handed in.  Per pair the results of the contiguous batch."""
    import torch
    pairs, rows = 2, 72
    imgs = np.stack([ic.noise(rows, cols, seed=40 + k) for k in range(2 * pairs)]).reshape(pairs, 2, rows, cols)
    prm = sorb.OrbParams(300, 1.2, 3, 20, 7)
    dev = torch.from_numpy(imgs).to("cuda:0")
    torch.cuda.synchronize()
    c0 = sorb.stereo_batch_dev(ctx, dev.data_ptr(), pairs, cols, rows, cols, orb=prm).copy()
    want = [sorb.stereo_batch_fetch(ctx, p, 2048) for p in range(pairs)]
    assert c0[:, :2].min() > 100
    whole_rows = offset == 0 and stride % 8 == 0                                              # the 8-byte loads read the padding of the last row too
    host = np.full(offset + 2 * pairs * rows * stride - (0 if whole_rows else stride - cols), 0xA5, np.uint8)      # else: ends with the last pixel
    v = np.ndarray((pairs, 2, rows, cols), np.uint8, buffer=host, offset=offset, strides=(2 * rows * stride, rows * stride, stride, 1))
    v[:] = imgs
    pdev = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    c1 = sorb.stereo_batch_dev(ctx, pdev.data_ptr() + offset, pairs, stride, rows, cols, orb=prm).copy()
    assert np.array_equal(c0, c1)
    for p in range(pairs):
        got = sorb.stereo_batch_fetch(ctx, p, 2048)
        for key in ("kL", "kR"):
            assert got[key].tobytes() == want[p][key].tobytes()
        for key in ("dL", "dR", "match_idx", "match_dist", "xyz", "ok"):
            assert np.array_equal(got[key], want[p][key]), (p, key)
