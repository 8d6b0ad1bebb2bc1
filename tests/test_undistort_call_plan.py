"""CPU: the call of ssx_undistort / ssx_undistort_lens / ssx_undistort_plan_apply as a plain value (csrc/undistort.hip: ud_check, ud_build
-> UdCall), shown by ssx_undistort_debug_plan without a device.  Every case of tests/undistort_call_cases.py is held to the rules the
comments of undistort.hip state, restated here; the refusals of both entry points are held to their status, their text and their order."""
import pytest

import undistort_call_cases as cc
from ssvio_amd import _lib
from ssvio_amd import undistort as ud

ROWS, COLS, IMG = cc.ROWS, cc.COLS, cc.IMG
DPITCH = 68                          # cols rounded up to a dword
ENTRY_BYTES = {ud.ENTRY_UNDISTORT: 184, ud.ENTRY_LENS: 184, ud.ENTRY_PLAN_APPLY: 40}     # sizeof(UdJob), sizeof(UdRemapJob)


def _up256(v):
    return (v + 255) & ~255


def _extent(stride):
    return (ROWS - 1) * stride + COLS


@pytest.mark.parametrize("name", list(cc.CASES))
def test_the_plan_of_every_case_keeps_the_stated_rules(name):
    case = cc.CASES[name]
    jobs, n, stored = case["jobs"], len(case["jobs"]), case["entry"] == ud.ENTRY_PLAN_APPLY
    p = cc.plan_of(case)
    assert p["status"] == _lib.SSX_OK and p["error"] == "", p["error"]
    assert p["grid"] == (1, 12, n) and p["block"] == (64, 4, 1)          # ceil(67 / 256), ceil(45 / 4), one z per job
    assert (p["src_intake"], p["dst_intake"]) == (case["src_intake"], case["dst_intake"])
    # the block: [job table | sources] | results -- disjoint, in order, each at a multiple of 256
    (t_off, t_n), (s_off, s_n), (r_off, r_n) = p["spans"]
    assert t_off == 0 and t_n == n * ENTRY_BYTES[case["entry"]]
    assert t_off + t_n <= s_off and s_off + s_n == p["up_bytes"] == r_off and r_off + r_n == p["arena_bytes"]
    assert all(v % 256 == 0 for v in (t_off, s_off, r_off, p["up_bytes"], p["arena_bytes"]))
    # everything sent lies in front of up_bytes, everything that comes back behind it
    for u in p["up"]:
        assert 0 <= u["off"] and u["off"] + u["bytes"] <= p["up_bytes"], u
    for d in p["down"]:
        assert p["up_bytes"] <= d["off"] and d["off"] + (d["height"] - 1) * d["dev_pitch"] + d["width"] <= p["arena_bytes"], d
    # the table goes up first, from staging; with staged images it is the one copy and carries them
    staged = case["src_intake"] == ud.STAGED
    assert p["up"][0]["off"] == 0 and p["up"][0]["host_off"] == ud.STAGING and p["up"][0]["images"] == (1 if staged else 0)
    assert p["up"][0]["bytes"] == (p["up_bytes"] if staged or not stored else t_n)
    assert p["stage_bytes"] == (p["arena_bytes"] if staged or not stored else t_n)
    image_ups, k_up, k_down = p["up"][1:], 0, 0
    slot = (lambda b: _up256(b)) if stored else (lambda b: b)
    for k, (so, ss, do, ds, _) in enumerate(jobs):
        j = p["jobs"][k]
        # sources
        if case["src_intake"] == ud.STAGED:                              # packed at a pitch of cols; a plan's slots are rounded to 256
            assert j["src_off"] == s_off + k * slot(IMG) and j["src_stride"] == COLS
        elif case["src_intake"] == ud.RANGE:                             # the host layout: base + (src_k - src_0), at its own stride, in ONE copy
            assert j["src_off"] == s_off + (so - jobs[0][0]) and j["src_stride"] == ss
            assert j["src_off"] + _extent(ss) <= p["up_bytes"]
        elif case["src_intake"] == ud.EACH and case["src_facts"][1][k] == ud.PINNED:
            u = image_ups[k_up]; k_up += 1
            assert (u["off"], u["host_off"], u["bytes"], u["images"]) == (j["src_off"], so, _extent(ss), 1) and j["src_stride"] == ss
            assert j["src_off"] % 256 == 0 and s_off <= j["src_off"]
        else:
            assert j["src_off"] == ud.WHERE_IT_LIES and j["src_stride"] == ss
        # results
        if case["dst_intake"] == ud.STAGED:                              # a staged result's pitch is cols rounded up to 4
            assert j["dst_off"] == r_off + k * slot(ROWS * DPITCH) and j["dst_stride"] == DPITCH
        elif case["dst_intake"] == ud.RANGE:                             # images of rows * cols bytes at a stride of cols, slots rounded to 256
            assert j["dst_off"] == r_off + k * _up256(IMG) and j["dst_stride"] == COLS
        elif case["dst_intake"] == ud.EACH and case["dst_facts"][1][k] == ud.PINNED:
            d = p["down"][k_down]; k_down += 1
            assert (d["host_off"], d["host_pitch"], d["off"], d["dev_pitch"], d["width"], d["height"]) == (do, ds, j["dst_off"], DPITCH, COLS, ROWS)
            assert j["dst_off"] % 256 == 0 and j["dst_stride"] == DPITCH
        else:
            assert j["dst_off"] == ud.WHERE_IT_LIES and j["dst_stride"] == ds
    if case["src_intake"] == ud.RANGE:
        range_bytes = jobs[-1][0] - jobs[0][0] + _extent(jobs[-1][1])
        assert len(image_ups) == 1 and (image_ups[0]["off"], image_ups[0]["host_off"], image_ups[0]["bytes"]) == (s_off, jobs[0][0], range_bytes)
    elif case["src_intake"] == ud.EACH:
        assert k_up == len(image_ups)
    else:
        assert not image_ups
    if case["dst_intake"] == ud.STAGED:                                  # one linear copy into staging
        assert p["down"] == [dict(host_off=ud.STAGING, host_pitch=0, off=r_off, dev_pitch=0, width=n * slot(ROWS * DPITCH), height=1)]
    elif case["dst_intake"] == ud.RANGE:                                 # one 2-D copy: a row of it is an image, nothing between the images is written
        assert p["down"] == [dict(host_off=jobs[0][2], host_pitch=jobs[1][2] - jobs[0][2], off=r_off, dev_pitch=_up256(IMG), width=IMG, height=n)]
    elif case["dst_intake"] == ud.EACH:
        assert k_down == len(p["down"])
    else:
        assert not p["down"]
    # the counters are the sums of the copies
    st = p["stats"]
    assert st["launches"] == 1 and st["syncs"] == 1
    assert st["bytes_up"] == sum(u["bytes"] for u in p["up"]) and st["copies_up"] == sum(u["images"] for u in p["up"]) == case["copies_up"]
    assert st["bytes_down"] == sum(d["width"] * d["height"] for d in p["down"]) and st["copies_down"] == len(p["down"]) == case["copies_down"]
    # ... and the values the GPU tests assert for these shapes
    if staged and stored:
        assert n * ROWS * DPITCH <= st["bytes_down"] <= n * (ROWS * DPITCH + 256)
        assert n * IMG <= st["bytes_up"] <= n * (IMG + 256 + 256) + 256
    if staged and not stored:
        assert st["bytes_down"] == n * ROWS * DPITCH
        assert n * IMG <= st["bytes_up"] <= n * (IMG + 256 + 256) + 256
    if case["dst_intake"] == ud.RANGE:
        assert st["bytes_down"] == n * IMG
    if case["dst_intake"] == ud.IN_PLACE:
        assert st["bytes_down"] == 0


def test_the_cases_the_issue_names_are_all_there():
    names = set(cc.CASES)
    assert {f"apply staged n={n} stride={s}" for n in (1, 2, 8) for s in (67, 80)} <= names
    assert {f"undistort {how} n={n}" for how in ("staged", "in place") for n in (1, 2, cc.MAX_JOBS)} <= names
    assert cc.MAX_JOBS == _lib.SSX_UNDISTORT_MAX_JOBS


def test_the_runtimes_answer_decides_between_one_copy_and_a_copy_each():
    """the same pointers: one pinned allocation -> RANGE, several -> EACH, one device allocation -> IN_PLACE"""
    jobs = cc.CASES["apply arena n=8"]["jobs"]
    intakes = {}
    for what, facts in (("one pinned", (True, [ud.PINNED] * 8)), ("several pinned", (False, [ud.PINNED] * 8)), ("one device", (True, [ud.DEVICE] * 8)),
                        ("mixed", (False, [ud.PINNED, ud.DEVICE] * 4))):
        p = ud.debug_plan(ud.ENTRY_PLAN_APPLY, ROWS, COLS, jobs, True, cc.N_MAPS, facts, facts)
        intakes[what] = (p["src_intake"], p["dst_intake"], p["stats"]["copies_up"], p["stats"]["copies_down"])
    assert intakes == {"one pinned": (ud.RANGE, ud.RANGE, 1, 1), "several pinned": (ud.EACH, ud.EACH, 8, 8), "one device": (ud.IN_PLACE, ud.IN_PLACE, 0, 0),
                       "mixed": (ud.EACH, ud.EACH, 4, 4)}


# ---- the refusals: status, text, order -------------------------------------------------------------------------------------------
GOOD = (0, COLS, 2 * IMG, COLS, 0)
OTHER = (IMG, COLS, 3 * IMG, COLS, 1)


def _refused(entry, jobs, rows=ROWS, cols=COLS, **kw):
    p = ud.debug_plan(entry, rows, cols, jobs, kw.pop("on_device", False), kw.pop("n_maps", 4), **kw)
    assert set(p) == {"status", "error"}
    return p["status"], p["error"]


# the lists of tests/test_undistort_gpu.py and tests/test_undistort_plan_gpu.py, and what the entry points add to them
COMMON = {
    "n < 0": (dict(jobs=[GOOD], n=-1), "n = -1 outside [0, 1024]"),
    "n above the limit": (dict(jobs=[GOOD], n=1025), "n = 1025 outside [0, 1024]"),
    "null table": (dict(jobs=[GOOD], null_table=True), "jobs is null"),
    "null src": (dict(jobs=[(None, COLS, 2 * IMG, COLS, 0)]), "job 0 has a null src"),
    "null dst": (dict(jobs=[(0, COLS, None, COLS, 0)]), "job 0 has a null dst"),
    "null dst of the second job": (dict(jobs=[GOOD, (IMG, COLS, None, COLS, 1)]), "job 1 has a null dst"),
    "src stride": (dict(jobs=[(0, COLS - 1, 2 * IMG, COLS, 0)]), "job 0 has a stride (src 66, dst 67) smaller than cols = 67"),
    "dst stride": (dict(jobs=[(0, COLS, 2 * IMG, COLS - 1, 0)]), "job 0 has a stride (src 67, dst 66) smaller than cols = 67"),
    "in place": (dict(jobs=[(0, COLS, 0, COLS, 0)]), "the dst of job 0 overlaps the src of job 0 (there is no in-place form)"),
    "overlap by one byte": (dict(jobs=[(0, COLS, IMG - 1, COLS, 0)]), "the dst of job 0 overlaps the src of job 0 (there is no in-place form)"),
    "dst on another job's src": (dict(jobs=[GOOD, (IMG, COLS, 0, COLS, 1)]), "the dst of job 1 overlaps the src of job 0 (there is no in-place form)"),
}
INLINE = {
    "rows": (dict(jobs=[GOOD], rows=0), "rows = 0, cols = 67 (both must be >= 1)"),
    "cols": (dict(jobs=[GOOD], cols=0), "rows = 45, cols = 0 (both must be >= 1)"),
    "negative rows": (dict(jobs=[GOOD], rows=-3), "rows = -3, cols = 67 (both must be >= 1)"),
    "lens model": (dict(jobs=[GOOD, (IMG, COLS, 3 * IMG, COLS, 2)]), "job 1 names lens model 2 (SSX_LENS_RADTAN = 0, SSX_LENS_KB4 = 1)"),
}
STORED = {
    "map the plan does not hold": (dict(jobs=[(0, COLS, 2 * IMG, COLS, 4)]), "job 0 names map 4, the plan holds 4"),
    "negative map": (dict(jobs=[GOOD, (IMG, COLS, 3 * IMG, COLS, -1)]), "job 1 names map -1, the plan holds 4"),
    "pageable src as device memory": (dict(jobs=[GOOD], on_device=True, src_facts=(False, [ud.NEITHER]), dst_facts=(False, [ud.NEITHER])),
                                      "the src of job 0 is neither device memory nor pinned host memory (images_on_device = 1)"),
    "pageable dst as device memory": (dict(jobs=[GOOD, OTHER], on_device=True, src_facts=(False, [ud.PINNED, ud.DEVICE]), dst_facts=(False, [ud.DEVICE, ud.NEITHER])),
                                      "the dst of job 1 is neither device memory nor pinned host memory (images_on_device = 1)"),
}


@pytest.mark.parametrize("entry, who, extra", [(ud.ENTRY_UNDISTORT, "ssx_undistort", INLINE), (ud.ENTRY_LENS, "ssx_undistort_lens", INLINE),
                                               (ud.ENTRY_PLAN_APPLY, "ssx_undistort_plan_apply", STORED)])
def test_every_rejection_has_its_status_and_its_text(entry, who, extra):
    for name, (kw, what) in {**COMMON, **extra}.items():
        st, msg = _refused(entry, **kw)
        assert (st, msg) == (_lib.SSX_ERR_INVALID_ARG, f"{who}: {what}"), name
    # no jobs: nothing to do; neighbours that do not overlap are accepted
    assert _refused(entry, [], null_table=True) == (_lib.SSX_OK, "")
    assert ud.debug_plan(entry, ROWS, COLS, [(0, COLS, IMG, COLS, 0)], n_maps=4)["status"] == _lib.SSX_OK


def test_a_side_above_the_limit_is_unsupported_and_comes_after_the_overlap():
    big = 32769
    far = (0, big, 1 << 38, big, 0)
    assert _refused(ud.ENTRY_UNDISTORT, [far], rows=4, cols=big) == (_lib.SSX_ERR_UNSUPPORTED, "ssx_undistort: 4 x 32769 is above 32768 a side")
    assert _refused(ud.ENTRY_UNDISTORT, [far], rows=big, cols=4)[0] == _lib.SSX_ERR_UNSUPPORTED
    assert _refused(ud.ENTRY_UNDISTORT, [(0, big, 0, big, 0)], rows=4, cols=big)[1].endswith("(there is no in-place form)")
    assert ud.debug_plan(ud.ENTRY_PLAN_APPLY, 4, big, [far], n_maps=1)["status"] == _lib.SSX_OK      # (a plan's size is its creation's to refuse)


def test_the_refusals_come_in_the_stated_order():
    """each call has two faults: the earlier check speaks"""
    bad_stride_then_null = [(0, COLS - 1, 2 * IMG, COLS, 0), (None, COLS, 3 * IMG, COLS, 0)]
    for entry in (ud.ENTRY_UNDISTORT, ud.ENTRY_PLAN_APPLY):
        assert "n = -1" in _refused(entry, [GOOD], n=-1, null_table=True)[1]                       # the count before the table
        assert "job 0 has a stride" in _refused(entry, bad_stride_then_null)[1]                    # job by job, not check by check
        assert "null src" in _refused(entry, [(None, COLS - 1, 0, COLS, 9)])[1]                    # a job's pointers, then its strides, then its tag
        assert "stride" in _refused(entry, [(0, COLS - 1, 0, COLS, 9)])[1]
        assert "names" in _refused(entry, [(0, COLS, 0, COLS, 9)])[1]                              # the tag before the overlap
    assert "rows = 0" in _refused(ud.ENTRY_UNDISTORT, [GOOD], rows=0, null_table=True)[1]          # ssx_undistort: the size before the table ...
    assert "n = 1025" in _refused(ud.ENTRY_UNDISTORT, [GOOD], rows=0, n=1025)[1]                   # ... and behind the count
    # the overlap before the kind of memory; the sources before the results; a one-allocation range of unknown kind names job 0
    neither = dict(on_device=True, src_facts=(False, [ud.PINNED, ud.NEITHER]), dst_facts=(False, [ud.NEITHER, ud.NEITHER]))
    assert "overlaps" in _refused(ud.ENTRY_PLAN_APPLY, [GOOD, (IMG, COLS, 0, COLS, 1)], **neither)[1]
    assert "the src of job 1" in _refused(ud.ENTRY_PLAN_APPLY, [GOOD, OTHER], **neither)[1]
    one = dict(on_device=True, src_facts=(True, [ud.NEITHER, ud.PINNED]), dst_facts=(True, [ud.PINNED, ud.PINNED]))
    assert "the src of job 0" in _refused(ud.ENTRY_PLAN_APPLY, [GOOD, OTHER], **one)[1]
    # ssx_undistort asks nothing about the memory: images_on_device is the caller's word
    assert ud.debug_plan(ud.ENTRY_UNDISTORT, ROWS, COLS, [GOOD], True, src_facts=(False, [ud.NEITHER]), dst_facts=(False, [ud.NEITHER]))["status"] == _lib.SSX_OK
