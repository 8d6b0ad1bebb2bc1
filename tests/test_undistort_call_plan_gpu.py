"""GPU: every case of tests/undistort_call_cases.py that real memory can state -- pageable arrays, an ssx_host_alloc arena, pinned
blocks allocated one by one, device memory -- through its real entry point.  The counters of the call are the ones
ssx_undistort_debug_plan predicts for the pointers the call was given and the facts the memory really has (so the plan the CPU test
holds to its rules is the call that is issued), and the output is the model's bytes (tools/undistort_model.py)."""
import numpy as np
import pytest

import undistort_call_cases as cc
from ssvio_amd import undistort as ud
from tools import undistort_model as um

pytestmark = pytest.mark.gpu

SETS = [((38.0, 41.0, 30.2, 20.7), (-0.28, 0.07, 0.004, -0.003, 0.01)), ((39.0, 40.0, 31.0, 21.5), (0.2, -0.05, -0.002, 0.003, 0.0))]


@pytest.fixture(scope="module")
def made():
    """eight images, two parameter sets, and the model's result of every image under either set, computed once"""
    rng = np.random.default_rng(77)
    imgs = [rng.integers(1, 256, size=(cc.ROWS, cc.COLS), dtype=np.uint8) for _ in range(8)]
    want = {(i, s): um.undistort(imgs[i], *SETS[s]) for i in range(8) for s in range(2)}
    for a in imgs + list(want.values()):
        a.setflags(write=False)
    assert not np.array_equal(want[(0, 0)], want[(0, 1)])
    return imgs, want


@pytest.fixture(scope="module")
def plan2(ctx):
    with ud.UndistortPlan(ctx, cc.ROWS, cc.COLS) as plan:
        assert [plan.add(ud.make_params(*s)) for s in SETS] == [0, 1]
        yield plan


@pytest.mark.parametrize("name", [n for n, c in cc.CASES.items() if c["gpu"]])
def test_the_call_issues_what_the_plan_says_and_writes_the_models_bytes(ctx, plan2, made, name):
    imgs, want = made
    case = cc.CASES[name]
    outs, stats, facts = cc.run(ctx, plan2, case, imgs, [ud.make_params(*s) for s in SETS])
    said = ud.debug_plan(case["entry"], cc.ROWS, cc.COLS, facts, case["on_device"], cc.N_MAPS, case["src_facts"], case["dst_facts"])
    assert said["status"] == 0, said["error"]
    assert (said["src_intake"], said["dst_intake"]) == (case["src_intake"], case["dst_intake"])
    assert stats == {k: said["stats"][k] for k in stats}, (stats, said["stats"])          # (ssx_undistort reports four of the six)
    if case["entry"] == ud.ENTRY_PLAN_APPLY:
        assert (stats["copies_up"], stats["copies_down"]) == (case["copies_up"], case["copies_down"])
    for k, got in enumerate(outs):
        assert np.array_equal(got, want[(k % 8, k % cc.N_MAPS)]), k
