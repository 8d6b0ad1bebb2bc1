"""CPU: the made candidate sets of tests/octree_cases.py.  Every set goes through the sequential oracle (po.octree) and through the
data-parallel model the kernel follows (tools/octree_model.py), byte-equal as in tests/test_octree_model.py; the numpy restatement of
the plan's geometry is held against ssx_orb_debug_plan, which also shows the build of k_octree a key selects; and every case's
self-checks run, so that no case goes quietly trivial: its M, its nIni, the number of distinct responses, for phase-2 cases an oracle
output of N .. N + 2 < M keypoints, for the block exactly one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import octree_cases as oc  # noqa: E402
from octree_model import octree_parallel  # noqa: E402

from ssvio_amd import _lib  # noqa: E402
from tools.orb_plan_ab import case as plan_case, plan_info  # noqa: E402

DISTINCT = dict(equal=lambda M: 1, rising=lambda M: min(M, 255), few=lambda M: None, varied=lambda M: None)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", oc.NAMES)
def test_geometry_and_build_of_the_key(lib, name):
    """levels, budgets and cell counts as the plan has them; the bytes of the octree scratch buffer (buffer 8 of the arena) are
    256 for keys and tables in LDS, else images x levels x the stride of [keys | tables]: they name the build"""
    case = oc.CASES[name]
    k, g = case["key"], oc.geometry(case["key"])
    p = plan_info(lib, plan_case(k["rows"], k["cols"], I=k["images"], detect=int(k["detect_only"]), nfeatures=k["nfeatures"], nlevels=k["nlevels"], scale=k["scale"]))
    assert p.status == _lib.SSX_OK, p.error
    assert p.nlevels == g["L"]
    for l in range(g["L"]):
        assert (p.lvl_rows[l], p.lvl_cols[l], p.feat[l]) == (g["rows"][l], g["cols"][l], g["feat"][l])
        assert p.lvl_cell0[l + 1] - p.lvl_cell0[l] == len(g["cells"][l])
    assert (g["global_tab"], g["global_keys"]) == case["builds"]
    assert p.buf_bytes[8] == g["scratch_bytes"]
    assert g["n_ini"][0] == case["n_ini"]


@pytest.mark.parametrize("name", oc.NAMES)
def test_sets_through_oracle_and_model(po, name):
    case, g, sets = oc.build(name)
    assert sorted(sets) == sorted(case["sets"])
    for (i, l), (xy, r) in sets.items():
        spec = case["sets"][(i, l)]
        M, N, cap = len(xy), g["feat"][l], g["cap"]
        assert M == spec["M"] and r.min() >= 1 and r.max() <= 255 and xy.min() >= 0 and xy.max() <= 4095
        want = DISTINCT[spec["kind"]](M)
        assert want is None or len(np.unique(r)) == want
        if spec["kind"] in ("few", "varied") and M > 100:
            assert len(np.unique(r)) > 1
        if spec["kind"] == "rising":
            assert (np.diff(r) >= 0).all() and (M < 2 or r[-1] > r[0])
        assert len(oc.order(g["cells"][l], xy)) == M and (oc.order(g["cells"][l], xy) == xy).all()     # reference order, and a valid cell fill
        kp = oc.keypoints(po, xy[:cap], r[:cap])
        box = (oc.BORDER, g["cols"][l] - oc.BORDER, oc.BORDER, g["rows"][l] - oc.BORDER)
        ref = po.octree(kp, *box, N)
        sel = octree_parallel(kp["x"].copy(), kp["y"].copy(), kp["response"].copy(), *box, N)
        got = kp[sel] if len(sel) else kp[:0]
        assert len(got) == len(ref) and got.tobytes() == ref.tobytes()
        assert len(ref) >= 1 and len(ref) <= oc.SEL_CAP
        if case["checks"].get("phase2"):
            assert N < min(M, cap) and N <= len(ref) <= N + 2, (N, M, len(ref))
        if case["checks"].get("block"):
            assert len(ref) == 1


def test_named_properties_of_the_cases():
    """what the names promise"""
    _, g, sets = oc.build("K/right_root")
    assert g["n_ini"][0] == 4 and sets[(0, 0)][0][:, 0].min() >= 3 * (g["cols"][0] - 2 * oc.BORDER) // 4 + 1
    for name, roots in (("A/per_root", 2), ("K/per_root", 4), ("C1/per_root", 2)):
        _, g, sets = oc.build(name)
        xy = sets[(0, 0)][0]
        hx = np.float32(g["cols"][0] - 2 * oc.BORDER) / np.float32(roots)
        assert sorted((xy[:, 0].astype(np.float32) / hx).astype(int)) == list(range(roots))
    assert {len(oc.build("A/M%d" % M)[2][(0, 0)][0]) for M in (16383, 16384, 16385)} == {oc.CAND_CAP - 1, oc.CAND_CAP, oc.CAND_CAP + 1}
    assert {len(oc.build("C2/M%d/N1000" % M)[2][(0, 0)][0]) for M in (65535, 65536, 65537)} == {oc.CAND_CAP_BIG, oc.CAND_CAP_BIG + 1, oc.CAND_CAP_BIG + 2}
    for name in ("D/small/n1000", "D/small/n4088", "D/big/n3000"):
        case, g, sets = oc.build(name)
        L = g["L"]
        counts = [len(sets[(i, l)][0]) if (i, l) in sets else 0 for i in range(3) for l in range(L)]
        nonzero = [c for c in counts if c]
        assert 0 in counts and len(set(nonzero)) == len(nonzero)          # some levels empty, no two workgroups the same count
