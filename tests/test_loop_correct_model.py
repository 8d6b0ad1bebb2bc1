"""CPU: tools/loop_correct_model.py, the contract of ssx_loop_correct -- against the 60-digit fixture
(tests/golden/loop_correct_hp.npz, every entry of every case), its invariants, the whole chain with the CPU oracle's optimiser in
the middle, and the ABI of the call (declared, exported, mirrored)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import loop_correct_cases as lcc
from tools import loop_correct_model as lcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = np.load(os.path.join(os.path.dirname(__file__), "golden", "loop_correct_hp.npz"))
CASE = {n: lcc.make(n) for n in lcc.NAMES}


def test_fixture_covers_the_cases_and_the_required_point_counts():
    assert list(HP["names"]) == lcc.NAMES and float(HP["factor"]) == 4.0
    for n in ("lc12", "lc60", "lc200", "only_cur", "all_fixed", "no_edges", "far", "half_turn", "no_change"):
        assert n in CASE
    assert {0, 1, 63, 64, 65, 255, 257} <= {pr["N"] for pr in CASE.values()}
    assert (CASE["lc12"]["P"], CASE["lc60"]["P"], CASE["lc200"]["P"]) == (12, 60, 200)
    assert CASE["only_cur"]["kf_active"].sum() == 1 and CASE["all_fixed"]["kf_active"].all() and CASE["no_edges"]["E"] == 0
    assert np.abs(CASE["far"]["poses"][:, 4:]).max() > 3000 and CASE["half_turn"]["corrected_pose"][3] == 0.0
    assert np.array_equal(CASE["no_change"]["corrected_pose"], CASE["no_change"]["poses"][CASE["no_change"]["cur_kf"]])
    free_keep = [n for n, pr in CASE.items() if pr["keep_kf"] >= 0 and not lcm.fixed_set(pr)[pr["keep_kf"]]]
    assert free_keep == ["lc60"] and CASE["lc12"]["kf_active"][CASE["lc12"]["keep_kf"]]
    for n in ("lc12", "lc60", "lc200", "far", "half_turn", "no_change"):      # the mix loop_correct_cases lists
        pr = CASE[n]
        act, anc, pact = pr["kf_active"] != 0, pr["point_anchor"], pr["point_active"] != 0
        fixed = lcm.fixed_set(pr) != 0
        assert (pact & (anc < 0)).any() and (~pact & (anc < 0)).any() and (pact & (anc >= 0) & ~act[np.maximum(anc, 0)]).any()
        assert (~pact & (anc >= 0) & fixed[np.maximum(anc, 0)]).any() and (~pact & (anc >= 0) & ~fixed[np.maximum(anc, 0)]).any()
        assert (pact & (anc == pr["cur_kf"])).any()


@pytest.mark.parametrize("name", lcc.NAMES)
def test_model_against_60_digits(name):
    """every pose and every point of every case.  Bar: the chain to a stage-3 point is six SE3 operations (inverse, two products,
    inverse, two actions), each about eight roundings of terms up to 2 M, M the case's largest number: 6 x 8 x 2 M x eps / 2 = 48 M eps,
    stated as 64 spacing(M); and never more than the distance the fixture recorded for the model, which the kernel's bar is built on."""
    pr = CASE[name]
    k = lcc.NAMES.index(name)
    s1, p1, _ = lcm.stage1(pr)
    assert np.array_equal(s1, HP[f"{name}_s3_s1_poses"]) and np.array_equal(p1, HP[f"{name}_s3_in_points"])
    opt = lcc.stated_opt_poses(pr, s1)
    assert np.array_equal(opt, HP[f"{name}_s3_opt_poses"])
    _, p3, _ = lcm.stage3(pr, s1, opt, p1)
    m0 = lcm.loop_correct(pr, None, iters=0)
    other = pr["point_active"] == 0
    got = dict(s1_poses=lcc.pose_distance(s1, HP[f"{name}_s1_poses"]), s1_points=lcc.point_distance(p1, HP[f"{name}_s1_points"]),
               identity=lcc.point_distance(m0["points"][other], HP[f"{name}_s1_points"][other]),
               s3_points=lcc.point_distance(p3, HP[f"{name}_s3_points"]))
    bar = 64 * np.spacing(lcc.magnitude(pr, HP[f"{name}_s1_poses"], HP[f"{name}_s3_points"]))
    print(name, {q: f"{v:.2e}" for q, v in got.items()}, f"bar {bar:.2e}")
    for q, v in got.items():
        assert v <= bar and v <= HP[f"model_{q}"][k], (q, v, bar, HP[f"model_{q}"][k])
    assert np.array_equal(m0["stage1_poses"], s1) and np.array_equal(m0["points"][~other], p1[~other])


@pytest.mark.parametrize("name", lcc.NAMES)
def test_model_invariants(name):
    pr = CASE[name]
    s1, p1, _ = lcm.stage1(pr)
    opt = lcc.stated_opt_poses(pr, s1)
    out = lcm.loop_correct(pr, lambda flat, iters: dict(poses=lcc.stated_opt_poses(pr, flat["poses"])))
    if out["pg"] is None:
        opt = s1
    lcc.check_invariants(pr, s1, opt, out["poses"], out["points"], out["stage1_points"])
    for key, v in lcc.expected_counts(pr).items():
        assert out[key] == v, key
    assert np.array_equal(pr["poses"], CASE[name]["poses"])                # the inputs are not modified


@pytest.mark.parametrize("name", ["lc12", "lc60", "only_cur", "all_fixed", "no_edges", "far"])
def test_full_chain_with_the_oracle_optimiser(po, name):
    pr = CASE[name]
    seen = []

    def optimiser(flat, iters):
        seen.append(flat)
        return po.pose_graph_opt(flat, "oracle", iters)
    out = lcm.loop_correct(pr, optimiser)
    fixed = lcm.fixed_set(pr) != 0
    if name in ("all_fixed", "no_edges"):
        assert out["pg"] is None and not seen and np.array_equal(out["opt_poses"], out["stage1_poses"])
    else:
        assert len(seen) == 1 and np.array_equal(seen[0]["poses"], out["stage1_poses"]) and np.array_equal(seen[0]["fixed"] != 0, fixed)
        pg = out["pg"]
        assert pg["n_iters"] >= 1 and pg["chi2"][-1] < pg["chi2"][0]
        assert np.array_equal(out["opt_poses"][fixed], out["stage1_poses"][fixed])             # fixed vertices keep the stage-1 bits
        assert not np.array_equal(out["opt_poses"][~fixed], out["stage1_poses"][~fixed])
    lcc.check_invariants(pr, out["stage1_poses"], out["opt_poses"], out["poses"], out["points"], out["stage1_points"])


def test_loop_correct_abi():
    """ssx_loop_correct is declared in ssx.h and exported by the built library, the ctypes mirrors have the C sizes, and the ABI version
    did not move"""
    import re
    hdr = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert re.search(r"SSX_API\s+ssx_status\s+ssx_loop_correct\s*\(", hdr)
    from ssvio_amd import build
    build.build()
    import ssvio_amd
    from ssvio_amd import _lib, loop
    lib = ssvio_amd.load()
    assert hasattr(lib, "ssx_loop_correct")
    assert lib.ssx_version() == _lib.SSX_VERSION == 120
    names = {"ssx_loop_correct_problem": loop.LoopCorrectProblem, "ssx_loop_correct_result": loop.LoopCorrectResult}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "ssx.h"\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + \
        'printf("points %zu\\n", offsetof(ssx_loop_correct_problem, points));printf("n_active_kf %zu\\n", offsetof(ssx_loop_correct_result, n_active_kf));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert sizes[n] == C.sizeof(cls), (n, sizes[n], C.sizeof(cls))
    assert sizes["points"] == loop.LoopCorrectProblem.points.offset and sizes["n_active_kf"] == loop.LoopCorrectResult.n_active_kf.offset
