"""CPU: the images of tests/orb_image_cases.py reach what they claim, and none exceeds a capacity of the kernels.

Every case goes through the CPU oracle cell by cell: `reach` counts, per case, the facts the case table names (corners on pixels
within a threshold of 0 or 255, responses of 254, equal scores next to each other, cells that take the minThFAST pass, cells whose
survivors are all masked, angles on an axis, descriptors with a zero byte, levels below 8 px, ...).  A count a case claims must be
above zero; all counts are printed.  On the way the cell-by-cell candidates are held against po.orb_grid_fast (so the restated grid
of orb_image_cases.cells is the oracle's), the cell counts against ssx_orb_debug_plan (so it is the plan's), and every level-0 cell's
po.fast_roi against the plain numpy statement of FAST-9 + score + NMS, orb_image_cases.fast9_numpy -- the tie-breaker should kernel
and oracle ever disagree.

Capacities (orb_ws.hpp): at most CELL_CAP NMS survivors per cell, CAND_CAP candidates and SEL_CAP selected per level, keypoints
within the wrapper's _cap() -- the GPU run of these cases never enters an overflow path."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import orb_image_cases as ic  # noqa: E402

from ssvio_amd import _lib  # noqa: E402
from ssvio_amd import orb as sorb  # noqa: E402
from tools.orb_plan_ab import case as plan_case, plan_info  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def oracle_levels(po, img, mask, prm):
    """the oracle's pyramid: level images and mask levels (None without a mask), po.resize_linear chained as ComputePyramid does"""
    rows, cols = po.level_sizes(img.shape[0], img.shape[1], prm["scale_factor"], prm["nlevels"])
    lv, mk = [np.ascontiguousarray(img)], [None if mask is None else np.ascontiguousarray(mask)]
    for l in range(1, prm["nlevels"]):
        lv.append(po.resize_linear(lv[-1], rows[l], cols[l]))
        mk.append(None if mask is None else po.resize_linear(mk[-1], rows[l], cols[l]))
    return lv, mk


def cell_survivors(po, lvl, prm, level0=False):
    """per cell of the level: (x, y, score of the NMS survivors at bordered-cell coordinates, the threshold that found them, whether the
    cell took the second pass).  level0: every po.fast_roi call is held against fast9_numpy, whose pre-NMS scores give the ties."""
    out, ties = [], 0
    for x0, y0, w, h, ox, oy in ic.cells(*lvl.shape):
        roi = np.ascontiguousarray(lvl[y0:y0 + h, x0:x0 + w])
        second = False
        for th in (prm["ini_th"], prm["min_th"]):
            xs, ys, sc = po.fast_roi(roi, th)
            if level0:
                nx, ny, ns, score, corner = ic.fast9_numpy(roi, th)
                assert np.array_equal(nx, xs) and np.array_equal(ny, ys) and np.array_equal(ns, sc), "po.fast_roi differs from the numpy statement"
                p = np.pad(score, 1)
                hh, ww = score.shape
                eq = np.zeros_like(corner)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if (dx, dy) != (0, 0):
                            eq |= p[1 + dy:1 + dy + hh, 1 + dx:1 + dx + ww] == score
                ties += int((corner & (score > 0) & eq).sum())
            if len(xs):
                break
            second = True
        out.append(dict(x=xs + ox, y=ys + oy, sc=sc, th=th, second=second and len(xs) > 0, px=roi[ys, xs] if len(xs) else np.zeros(0, np.uint8)))
    return out, ties


@functools.lru_cache(maxsize=None)
def _reach(name):
    from oracle import pyoracle as po
    po.build()
    case = ic.cases()[name]
    img, prm = np.ascontiguousarray(case["img"]), case["prm"]
    mask = None if case["mask"] is None else np.ascontiguousarray(case["mask"])
    oprm = po.orb_params(**prm)
    lv, mk = oracle_levels(po, img, mask, prm)
    r = dict(sat_corners=0, resp254=0, ties=0, second_pass_cells=0, masked_out_cells=0, masked_candidates=0, max_per_cell=0, max_per_level=0)
    per_level = []
    for l, (lvl, m) in enumerate(zip(lv, mk)):
        cs, ties = cell_survivors(po, lvl, prm, level0=(l == 0))
        cand = []
        for c in cs:
            keep = np.ones(len(c["x"]), bool) if m is None else m[c["y"], c["x"]] != 0
            r["max_per_cell"] = max(r["max_per_cell"], len(keep))
            r["second_pass_cells"] += int(c["second"])
            r["masked_candidates"] += int((~keep).sum())
            r["masked_out_cells"] += int(len(keep) > 0 and not keep.any())
            r["resp254"] += int((c["sc"][keep] == 254).sum())
            if l == 0:
                v = c["px"].astype(int)
                r["sat_corners"] += int(((v < c["th"]) | (v + c["th"] > 255)).sum())
            cand += [(x, y, s) for x, y, s in zip(c["x"][keep], c["y"][keep], c["sc"][keep])]
        if l == 0:
            r["ties"] = ties
            r["level0_cells"] = len(cs)
            r["level0_candidates"] = len(cand)
            r["level0_presurvivors"] = sum(len(c["x"]) for c in cs)
            r["all_level0_254"] = int(len(cand) > 0 and all(s == 254 for _, _, s in cand))
            r["all_level0_11"] = int(len(cand) > 0 and all(s == 11 for _, _, s in cand))
            r["all_cells_second_pass"] = int(len(cs) > 0 and all(c["second"] for c in cs))
            r["one_per_cell"] = int(len(cs) > 0 and all(len(c["x"]) == 1 for c in cs))
        # the restated grid is the oracle's: the same candidates in the same order
        g = po.orb_grid_fast(lvl, m, prm["ini_th"], prm["min_th"])
        assert [(int(k["x"]), int(k["y"]), int(k["response"])) for k in g] == [(int(x), int(y), int(s)) for x, y, s in cand], (name, l)
        r["max_per_level"] = max(r["max_per_level"], len(cand))
        per_level.append(len(cand))
    r["level0_empty"] = int(r["level0_presurvivors"] == 0 and r["level0_cells"] > 0)
    r["level0_no_candidates"] = int(r["level0_candidates"] == 0 and r["level0_cells"] > 0)
    kps, desc = po.orb_extract(img, mask, oprm)
    det = po.orb_detect(img, mask, oprm)
    r["keypoints"], r["detected"] = len(kps), len(det)
    r["no_keypoints"] = int(len(kps) == 0 and len(det) == 0)
    r["max_selected_per_level"] = int(np.bincount(kps["octave"], minlength=1).max()) if len(kps) else 0
    r["axis_angles"] = int(np.isin(kps["angle"], (0.0, 90.0, 180.0, 270.0)).sum())
    r["zero_desc_bytes"] = int((desc == 0).any(axis=1).sum()) if len(desc) else 0
    r["small_levels"] = sum(1 for a in lv if min(a.shape) < 8)
    r["px_at_0"], r["px_at_255"] = int((img == 0).sum()), int((img == 255).sum())
    r["mask_values"] = 0 if mask is None else int(set(np.unique(mask)) >= {0, 1, 128, 255})
    r["mask_strided"] = 0 if case["mask"] is None else int(case["mask"].strides[0] > case["mask"].shape[1])
    r["levels"] = [a.shape for a in lv]
    r["candidates_per_level"] = per_level
    return r


EXTRACT = ic.names("extract")


@pytest.mark.parametrize("name", EXTRACT)
def test_extract_case_reaches_what_it_claims(po, lib, name):
    case = ic.cases()[name]
    r = _reach(name)
    print("\nreach %-24s %s" % (name, {k: v for k, v in r.items() if v}))
    for claim in case["claims"]:
        assert r[claim] > 0, (name, claim)
    # capacities: the GPU run takes no overflow path
    prm = case["prm"]
    assert r["max_per_cell"] <= ic.CELL_CAP and r["max_per_level"] <= ic.CAND_CAP
    assert max(po.features_per_level(prm["nfeatures"], prm["scale_factor"], prm["nlevels"])) + 8 <= ic.SEL_CAP and r["max_selected_per_level"] <= ic.SEL_CAP
    cap = sorb.ORBextractor(None, prm["nfeatures"], prm["scale_factor"], prm["nlevels"], prm["ini_th"], prm["min_th"])._cap()
    assert r["keypoints"] <= cap and r["detected"] <= cap
    # the restated grid is the plan's, and the plan takes the key
    rows, cols = case["img"].shape
    p = plan_info(lib, plan_case(rows, cols, mask=int(case["mask"] is not None), nfeatures=prm["nfeatures"], nlevels=prm["nlevels"], scale=prm["scale_factor"],
                                 ini=prm["ini_th"], mn=prm["min_th"]))
    assert p.status == _lib.SSX_OK, p.error
    for l, shape in enumerate(r["levels"]):
        assert (p.lvl_rows[l], p.lvl_cols[l]) == shape
        assert p.lvl_cell0[l + 1] - p.lvl_cell0[l] == len(ic.cells(*shape))
    assert r["keypoints"] <= p.out_cap


def test_the_families_as_the_issue_observed_them():
    """checkerboards and period-2 dots give no level-0 candidate at either threshold and keypoints on the resized levels only; binary
    noise and period-4 dots respond 254 everywhere; the densest isolated-corner lattice stays below CELL_CAP"""
    for name in ("checker/p1", "checker/p4", "checker/p7", "dots/p2"):
        r = _reach(name)
        assert r["level0_presurvivors"] == 0 and r["keypoints"] > 100
    assert _reach("dots/p4")["max_per_cell"] <= 225 and _reach("dots/p4")["axis_angles"] > 50
    assert _reach("noise/uniform")["level0_candidates"] > 500
    r = _reach("cell/one_corner")
    assert r["level0_candidates"] == r["level0_cells"] > 0
    r = _reach("cell/all_tie")
    assert r["level0_candidates"] == r["level0_cells"] == r["second_pass_cells"] > 0 and r["ties"] >= 2 * r["level0_cells"]
    r = _reach("cell/one_corner_masked")
    assert r["masked_out_cells"] >= r["level0_cells"] > 0 and r["level0_candidates"] == 0 and r["second_pass_cells"] == 0


@pytest.mark.parametrize("name", ["noise/uniform", "noise/binary", "dots/p4", "blobs/saturated"])
@pytest.mark.parametrize("th", [0, 1, 7, 20, 100, 254, 255])
def test_fast_roi_is_the_numpy_statement(po, name, th):
    """po.fast_roi on the whole image == segment test, score as the largest passing threshold, strict 3x3 NMS, in plain numpy"""
    img = ic.cases()[name]["img"]
    xs, ys, sc = po.fast_roi(img, th)
    nx, ny, ns, score, corner = ic.fast9_numpy(img, th)
    assert np.array_equal(xs, nx) and np.array_equal(ys, ny) and np.array_equal(sc, ns)
    assert score.max() <= 254 and (score[corner] >= th).all()
    for x, y in list(zip(nx, ny))[:50]:
        assert po.is_fast_corner(img, x, y, th)


def test_score_zero_corners_never_survive(po):
    """threshold 0: a pixel whose arc is darker by exactly 1 is a corner of score 0, which the strict '>' drops"""
    img = ic.noise()
    _, _, _, score, corner = ic.fast9_numpy(img, 0)
    xs, ys, sc = po.fast_roi(img, 0)
    assert (corner & (score == 0)).sum() > 0 and (sc > 0).all()


@pytest.mark.parametrize("value", [0, 255])
@pytest.mark.parametrize("scale", [1.2, 2.3])
def test_constant_images_stay_constant(po, value, scale):
    """resize and blur identities: every level and every blurred level of a constant image is that constant, at 0 and at 255"""
    for rows, cols in ((120, 160), (41, 131), (40, 160)):
        img = np.full((rows, cols), value, np.uint8)
        lv, _ = oracle_levels(po, img, None, dict(scale_factor=scale, nlevels=4))
        for a in lv:
            assert a.size > 0 and (a == value).all() and (po.gauss7(a) == value).all()


@pytest.mark.parametrize("name", ic.names("pitched") + ic.names("batch"))
def test_pitched_views_lie_as_they_claim(name):
    case = ic.cases()[name]
    views = case.get("views", [case["img"]])
    copies = case["contiguous"] if case["kind"] == "batch" else [case["contiguous"]]
    addr = set()
    for v, a in zip(views, copies):
        rows, cols = v.shape
        assert v.strides[1] == 1 and v.strides[0] > cols and not v.flags["C_CONTIGUOUS"] and a.flags["C_CONTIGUOUS"]
        assert np.array_equal(v, a)
        buf = v.base
        first = v.ctypes.data - buf.ctypes.data
        assert first in ic.OFFSETS and first + (rows - 1) * v.strides[0] + cols == buf.size          # the last row ends the allocation
        assert sorb._img(v) is v                                                                      # passed as it lies
        addr.add(v.ctypes.data % 8)
    if case["kind"] == "batch":
        assert len(addr) == len(views) == 4 and len({v.strides[0] for v in views}) == 1
    print("\nreach %-24s stride %d cols %d (cols %% 8 = %d) offsets %s" % (name, views[0].strides[0], views[0].shape[1], views[0].shape[1] % 8,
                                                                           sorted(v.ctypes.data - v.base.ctypes.data for v in views)))


def test_pitched_table_covers_the_combinations():
    cs = [ic.cases()[n] for n in ic.names("pitched")]
    assert {(c["stride_kind"], c["offset"]) for c in cs} == {(s, o) for s in ic.STRIDES for o in ic.OFFSETS}
    assert sorted(c["img"].shape[1] % 8 for c in cs) == sorted(list(range(8)) * 2)


def test_img_keeps_existing_callers_unchanged():
    """_img: only 2-D uint8 arrays with unit column stride and a row stride of at least a row pass as they lie"""
    a = ic.noise(50, 60)
    assert sorb._img(a) is a
    for b in (a[:, ::2], a[::-1], a.T, a.astype(np.int32), a.astype(np.float64), np.asfortranarray(a)):
        c = sorb._img(b)
        assert c.flags["C_CONTIGUOUS"] and c.dtype == np.uint8 and np.array_equal(c, b.astype(np.uint8))
    assert sorb._img(a[:, 3:50]).strides == (60, 1)
    with pytest.raises(ValueError):
        sorb._img(np.zeros((2, 3, 4), np.uint8))


@pytest.mark.parametrize("name", ic.names("describe"))
def test_describe_case_reaches_what_it_claims(po, name):
    case = ic.cases()[name]
    img, prm, kin, want = case["img"], case["prm"], case["kps"], case["want"]
    rows, cols = po.level_sizes(img.shape[0], img.shape[1], prm["scale_factor"], prm["nlevels"])
    scales = ic.level_scales(prm)
    inside = np.zeros(len(kin), bool)
    for i, k in enumerate(kin):                              # the given coordinate divides back to the wanted level position
        l = int(k["octave"])
        if 0 <= l < prm["nlevels"]:
            px, py = np.float32(k["x"] / scales[l]), np.float32(k["y"] / scales[l])
            assert (px == want[i, 0] or (want[i, 0] == np.float32(18.999) and px < 19)) and (py == want[i, 1] or (want[i, 1] == np.float32(18.999) and py < 19))
            inside[i] = py - 19 >= 0 and py + 19 < rows[l] and px - 19 >= 0 and px + 19 < cols[l]
    ok, od = po.orb_describe_at(img, kin, po.orb_params(**prm))
    kept = np.zeros(len(kin), bool)
    kept[ok["class_id"]] = True
    assert not (kept & ~inside).any()
    l = kin["octave"].clip(0, prm["nlevels"] - 1)
    far_x, far_y = np.asarray(cols)[l] - 20, np.asarray(rows)[l] - 20
    frac = (want - np.floor(want) == 0.5).all(axis=1)
    even = (np.floor(want).astype(int) % 2 == 0)
    r = dict(given=len(kin), kept=int(kept.sum()),
             at_19=int((kept & ((want[:, 0] == 19) | (want[:, 1] == 19))).sum()),
             at_far_edge=int((kept & ((want[:, 0] == far_x) | (want[:, 1] == far_y))).sum()),
             past_far_edge=int((~kept & ((want[:, 0] == far_x + 1) | (want[:, 1] == far_y + 1))).sum()),
             below_19=int((~kept & (want == np.float32(18.999)).any(axis=1)).sum()),
             half_even=min(int((kept & frac & even[:, 0]).sum()), int((kept & frac & even[:, 1]).sum())),
             half_odd=min(int((kept & frac & ~even[:, 0]).sum()), int((kept & frac & ~even[:, 1]).sum())),
             not_corner=int((inside & ~kept).sum()),
             every_octave=min(int((kept & (kin["octave"] == o)).sum()) for o in range(prm["nlevels"]) if rows[o] > 38 and cols[o] > 38),
             desc_dropped_all=int(len(ok) == 0 and inside.sum() > 0))
    print("\nreach %-24s %s" % (name, r))
    for claim in case["claims"]:
        assert r[claim] > 0, (name, claim)
    assert ((want[:, 0] == far_x + 1) & kept).sum() == 0 and ((want == np.float32(18.999)).any(axis=1) & kept).sum() == 0
