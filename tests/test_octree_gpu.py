"""GPU: k_octree (ssvio_amd/csrc/octree.hip) on the made candidate sets of tests/octree_cases.py, through the tap
ssx_orb_debug_octree (include/ssx_test_hooks.h): no image, the kernel's four builds, every (image, level) workgroup of a batch with a
problem of its own.

Per case and (image, level) the tap's selection -- (x, y, response) in list order -- equals, element for element and in order, the
sequential oracle (po.octree, oracle/liboracle.so) run on the candidates as ssx_orb_stage_candidates returns them for that level, with
the level's box and budget; lvl_ncand is the set's size; status is 0, but bit 0 exactly where a set is larger than the capacity, and
there the oracle gets the first `cap` candidates.  All comparisons are exact integers.

The capacities are 16384 candidates per (image, level) with the keys in LDS and 65535 with the keys in global scratch (a node's
count is a 16-bit word: 65536 candidates in the single root of a square level came back as one keypoint when the capacity was 65536)."""
import numpy as np
import pytest

import octree_cases as oc
import ssvio_amd.orb as sorb
from ssvio_amd import _lib

pytestmark = pytest.mark.gpu


def extractor(ctx, k):
    return sorb.ORBextractor(ctx, nfeatures=k["nfeatures"], scaleFactor=k["scale"], nlevels=k["nlevels"])


def run(ctx, k, cand):
    return extractor(ctx, k).debug_octree(k["rows"], k["cols"], cand, images=k["images"], detect_only=k["detect_only"])


@pytest.mark.parametrize("name", oc.NAMES)
def test_kernel_selects_what_the_oracle_selects(ctx, po, name):
    case, g, sets = oc.build(name)
    k = case["key"]
    ex = extractor(ctx, k)
    out = ex.debug_octree(k["rows"], k["cols"], oc.candidates(sets), images=k["images"], detect_only=k["detect_only"])
    assert out["lvl_ncand"].shape == (k["images"], g["L"])
    for i in range(k["images"]):
        over = False
        for l in range(g["L"]):
            xy, r = sets.get((i, l), (np.zeros((0, 2), np.int64), np.zeros(0, np.int64)))
            staged = ex.stage_candidates(l, image=i)
            # the reference order comes from the library; the case was made in it
            assert len(staged) == len(xy)
            assert np.array_equal(staged["x"].astype(np.int64), xy[:, 0]) and np.array_equal(staged["y"].astype(np.int64), xy[:, 1])
            assert np.array_equal(staged["response"].astype(np.int64), r)
            assert out["lvl_ncand"][i, l] == len(xy)
            over |= len(xy) > g["cap"]
            sx = np.stack([staged["x"], staged["y"]], axis=1).astype(np.int64)
            want = oc.oracle_select(po, g, l, sx, staged["response"].astype(np.int64)) if len(xy) else np.zeros((0, 3), np.int32)
            got = out["sel"][i][l]
            print(name, "image", i, "level", l, "M", len(xy), "N", g["feat"][l], "oracle", len(want), "kernel", out["sel_count"][i, l])
            assert out["sel_count"][i, l] == len(want)
            assert got.shape == want.shape and np.array_equal(got, want)
        assert out["status"][i] == (1 if over else 0)


def test_tap_refuses_what_fast_cannot_have_left(ctx):
    """nothing is launched for a candidate outside every cell, a cell over its 256, a coordinate above 4095, a response outside 1..255,
    an image or level out of range; the next good call is served"""
    k = oc.key(240, 400, 300)
    g = oc.geometry(k)
    x0, x1, y0, y1 = g["cells"][0][0]
    good = [0, 0, x0 + 1, y0 + 1, 30]
    full = [[0, 0, x0 + (j % 20), y0 + j // 20, 30] for j in range(oc.CELL_CAP + 1)]
    assert x0 + 20 <= x1 and y0 + (oc.CELL_CAP + 1) // 20 < y1
    for bad, text in (([[0, 0, 0, y0, 30]], "lies in no grid cell"), ([[0, 0, x0, 1, 30]], "lies in no grid cell"),
                      ([[0, 0, g["cols"][0], y0, 30]], "lies in no grid cell"), (full, "more than 256 candidates in cell"),
                      ([[0, 0, 4096, y0, 30]], "outside 0..4095"), ([[0, 0, x0, -1, 30]], "outside 0..4095"),
                      ([[0, 0, x0, y0, 0]], "response 0 outside 1..255"), ([[0, 0, x0, y0, 256]], "response 256 outside 1..255"),
                      ([[1, 0, x0, y0, 30]], "out of range"), ([[-1, 0, x0, y0, 30]], "out of range"),
                      ([[0, 1, x0, y0, 30]], "out of range"), ([[0, -1, x0, y0, 30]], "out of range")):
        with pytest.raises(_lib.SsxError) as e:
            run(ctx, k, [good] + bad)
        assert e.value.status == _lib.SSX_ERR_INVALID_ARG and text in str(e.value), (bad[-1], str(e.value))
    assert len(full[:-1]) == oc.CELL_CAP
    out = run(ctx, k, full[:-1])                                   # exactly 256 in a cell is served
    assert out["status"][0] == 0 and out["lvl_ncand"][0, 0] == oc.CELL_CAP and out["sel_count"][0, 0] >= 1
    out = run(ctx, k, [good])
    assert out["status"][0] == 0 and out["lvl_ncand"][0, 0] == 1 and out["sel"][0][0].tolist() == [good[2:]]
    out = run(ctx, k, np.zeros((0, 5), np.int32))                  # no candidates at all: an empty selection, written
    assert out["status"][0] == 0 and out["lvl_ncand"][0, 0] == 0 and out["sel_count"][0, 0] == 0
