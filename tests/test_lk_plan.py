"""The LK host side without a GPU (ssx_lk_debug_plan, include/ssx_test_hooks.h): the geometry of a key, and per call of
tests/lk_call_cases.py the io block, the launch list, the image intake and the slots' flags afterwards -- each against a restatement of
the rule in ssvio_amd/csrc/lk.hip's comments -- and the refusals with their order (statuses and texts as the entry points have always
reported them: job checks, job by job, before the parameters, before the image size)."""
import pytest

import lk_call_cases as cc
from ssvio_amd import _lib, lk

FUSED_MAX_LEVELS, FUSED_MAX_JOBS, FT, JOB_BYTES = 4, 16, 8, 64
HAVE_NEXT, HAVE_NEXT_DERIV = 1, 2
INVALID = _lib.SSX_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def r256(n):
    return (n + 255) & ~255


@pytest.mark.parametrize("h,w,win,max_level", cc.GEOMETRIES)
def test_geometry(lib, h, w, win, max_level):
    p = lk.debug_plan(lib, h, w, [dict(slot=0, fresh=True, n=1)], win=win, max_level=max_level)
    assert p.status == _lib.SSX_OK, p.error
    rows, cols = [h], [w]                                               # buildOpticalFlowPyramid: a level not larger than the window ends the pyramid
    while len(rows) <= max_level and (rows[-1] + 1) // 2 > win and (cols[-1] + 1) // 2 > win:
        rows.append((rows[-1] + 1) // 2); cols.append((cols[-1] + 1) // 2)
    L = len(rows)
    assert p.levels == L and list(p.rows[:L]) == rows and list(p.cols[:L]) == cols and p.win == win and p.pad == win + 1
    end = 0
    for l in range(L):
        assert p.pitch[l] % 64 == 0 and p.pitch[l] >= cols[l] + 2 * p.pad
        assert p.off[l] >= end and p.doff[l] >= end                     # level spans disjoint, in order, inside a pyramid
        end = p.off[l] + p.pitch[l] * (rows[l] + 2 * p.pad)
        assert p.doff[l] + p.pitch[l] * (rows[l] + 2 * p.pad) <= p.deriv_words
    assert end <= p.pyr_bytes
    assert bool(p.fused_ok) == (L <= FUSED_MAX_LEVELS and min(rows[-1], cols[-1]) >= p.pad + 2)


def check_io(p, c, k):
    nj, npts = len(k["slots"]), max(sum(k["n"]), 1)
    span = dict(zip(lk.SPANS, zip(p.span_off, p.span_bytes)))
    order = [span[s] for s in lk.SPANS]
    for (a, na), (b, _) in zip(order, order[1:]):                      # memory order: disjoint when each ends before the next begins
        assert a + na <= b
    assert all(off % 256 == 0 for off, _ in order)
    assert span["tab"] == (0, JOB_BYTES * nj) and span["prev_pts"][1] == span["next_pts"][1] == 8 * npts
    assert span["status"][1] == npts and span["err"][1] == 4 * npts
    staged = sum(r256(c["h"] * c["w"]) * (2 if f else 1) for f in k["fresh"]) if p.intake == cc.STAGED else 0
    assert span["images"][1] == staged
    for s in ("tab", "images", "prev_pts", "next_pts"):                 # everything that is sent lies in front of in_bytes
        assert span[s][0] + span[s][1] <= p.in_bytes
    # what comes back is one run: next points, status, error, up to host_end
    assert span["next_pts"][0] + r256(8 * npts) == p.in_bytes == span["status"][0]
    assert span["status"][0] + r256(npts) == span["err"][0] and span["err"][0] + r256(4 * npts) == p.host_end
    off, nbytes = span["dev_images"]
    assert (nbytes > 0) == (p.intake in (cc.IN_ARENA, cc.EACH)) and off >= p.host_end and off + nbytes <= p.io_bytes
    if p.intake == cc.IN_ARENA:
        assert nbytes == p.arena_bytes + 16 and p.arena_bytes == max(cc.next_offsets(c, k)) + c["h"] * c["w"]


def check_launches(p, k, flags_before):
    nj, L, pad = len(k["slots"]), p.levels, p.pad
    got = [(lk.KERNELS[l.kernel], tuple(l.grid), l.which, l.level) for l in p.launch[:p.n_launches]]
    level_grid = lambda l: ((p.cols[l] + 2 * pad + 255) // 256, p.rows[l] + 2 * pad, nj)
    want = []
    assert bool(p.use_fused) == (bool(p.fused_ok) and nj <= FUSED_MAX_JOBS)
    if p.use_fused:                                                     # one launch for all images: z = job x {previous, next}
        want.append(("k_lk_pyramid", ((p.cols[L - 1] + 2 * pad + FT - 1) // FT, (p.rows[L - 1] + 2 * pad + FT - 1) // FT, 2 * nj), -1, -1))
    else:                                                               # per image set: the previous images only if a job is fresh
        for which in range(0 if any(k["fresh"]) else 1, 2):
            want.append(("k_lk_pad_level0", level_grid(0), which, 0))
            want += [("k_lk_pyr_down", level_grid(l), which, l) for l in range(1, L)]
    scharr = not p.use_fused or any(not f and not fl & HAVE_NEXT_DERIV for f, fl in zip(k["fresh"], flags_before))
    assert bool(p.scharr_now) == scharr
    if scharr:
        want += [("k_lk_scharr", level_grid(l), -1, l) for l in range(L)]
    if sum(k["n"]) > 0:                                                 # one wave per point, four points a workgroup
        want.append(("k_lk_track", ((max(k["n"]) + 3) // 4, nj, 1), -1, -1))
    assert got == want


def expected_intake(c, k, jobs, on_device, next0_is_host, use_fused, one_allocation=True):
    if not on_device:
        return cc.STAGED
    span, offs = c["h"] * c["w"], [j["next_off"] for j in jobs]         # (every case's stride is the image width)
    arena = len(jobs) >= 2 and all(b > a and b - a >= span for a, b in zip(offs, offs[1:])) and offs[-1] - offs[0] + span <= 2 * len(jobs) * span
    if arena and one_allocation:                                        # the copy of an arena is ONE copy: it may not leave the allocation
        return cc.IN_ARENA
    return cc.EACH if use_fused and next0_is_host else cc.IN_PLACE


def plan_case(lib, c, one_allocation=None):
    """every call of a case, the slots' flags carried from call to call as the context carries them; one_allocation: what the runtime
    answers when it is asked whether the `next` images lie in one allocation (None: what the case's layout says) -> the intakes"""
    flags, intakes = {}, []
    for k in c["calls"]:
        jobs, on_device, next0_is_host, one = cc.facts(c, k)
        one = one if one_allocation is None else int(one_allocation)
        before = [flags.get(s, 0) for s in k["slots"]]
        p = lk.debug_plan(lib, c["h"], c["w"], jobs, before, c["win"], c["max_level"], None, on_device, next0_is_host, one)
        assert p.status == _lib.SSX_OK, p.error
        check_io(p, c, k)
        check_launches(p, k, before)
        assert p.intake == expected_intake(c, k, jobs, on_device, next0_is_host, p.use_fused, one)
        assert (p.arena_bytes > 0) == (p.intake == cc.IN_ARENA)
        if c["intake"] is not None and one_allocation is None:
            assert (p.intake, bool(p.use_fused)) == (c["intake"], c["use_fused"])
        assert p.n_jobs == len(jobs)
        for j, s in enumerate(k["slots"]):                              # have_next, and the kept derivative images only after k_lk_pyramid
            assert p.slot_flags[j] & 3 == HAVE_NEXT | (HAVE_NEXT_DERIV if p.use_fused else 0)
            # a chained job turns the slot's two buffers over; the table names both of each kind
            assert bool(p.slot_flags[j] & 4) == (not k["fresh"][j] and not before[j] & 4)
            assert p.job_roles[j] in (0b1010, 0b0101) and bool(p.job_roles[j] & 1) == bool(p.slot_flags[j] & 4)
            flags[s] = p.slot_flags[j]
        intakes.append(p.intake)
    return intakes


@pytest.mark.parametrize("c", cc.CASES, ids=cc.name)
def test_calls(lib, c):
    plan_case(lib, c)


@pytest.mark.parametrize("c", cc.ALLOCATION_CASES, ids=cc.name)
def test_an_arena_is_one_allocation(lib, c):
    """Pointers that ascend at equal distances within 2 x jobs images are an arena only if the runtime confirms that they lie in ONE
    allocation: the arena's images cross in one copy over the whole range.  The same pointers planned with both answers: "several"
    is never LK_ARENA -- a copy per image in front of k_lk_pyramid when they are host memory, else read where they lie -- and "one"
    is the arena of before, with the same arena_bytes (check_io)."""
    host = c["calls"][0]["layout"] != cc.ADJACENT_DEVICE
    assert plan_case(lib, c) == [c["intake"]] * 2 == [cc.EACH if c["use_fused"] and host else cc.IN_PLACE] * 2
    assert plan_case(lib, c, one_allocation=False) == [c["intake"]] * 2
    assert plan_case(lib, c, one_allocation=True) == [cc.IN_ARENA] * 2


def test_the_allocation_question_decides_nothing_else(lib):
    """where the arithmetic already says "no arena" (or the images are staged) the answer is not looked at"""
    for c in cc.CASES:
        if c["intake"] not in (None, cc.IN_ARENA):
            assert plan_case(lib, c, one_allocation=False) == plan_case(lib, c, one_allocation=True) == [c["intake"]] * len(c["calls"]), c["name"]


def test_arena_rule_at_its_edges(lib):
    """unequal strides, a gap below one image, a range beyond 2 x jobs images: no arena"""
    h, w = 120, 168
    job = lambda j, off, stride=w: dict(slot=j, fresh=True, n=4, next_off=off, next_stride=stride)
    plan = lambda jobs, one=1: lk.debug_plan(lib, h, w, jobs, images_on_device=1, next0_is_host=1, one_allocation=one).intake
    span = h * w
    assert plan([job(0, 0), job(1, span)]) == cc.IN_ARENA
    assert plan([job(0, 0), job(1, span)], one=0) == cc.EACH             # two allocations back to back
    assert plan([job(0, 0), job(1, 3 * span)], one=0) == cc.EACH
    assert plan([job(0, 0), job(1, span - 1)]) == cc.EACH
    assert plan([job(0, 0), job(1, 3 * span)]) == cc.IN_ARENA          # range 4 spans = 2 x 2 jobs
    assert plan([job(0, 0), job(1, 3 * span + 1)]) == cc.EACH
    assert plan([job(0, 0), job(1, 2 * span, w + 8)]) == cc.EACH
    assert plan([job(0, 0), job(1, 2 * span), job(2, span)]) == cc.EACH  # not ascending


TEXT = {"stride": "ssx_lk: stride smaller than the image width", "slot": "ssx_lk: slot 4096 outside 0..4095",
        "twice": "ssx_lk_track_batch: slot 1 twice in one call",
        "chain": "ssx_lk_track_next: no previous ssx_lk_track call with the same image size, window and max_level on this context (slot 5)",
        "even": "ssx_lk: unsupported window 10 (odd, 3..15) or max_level 3 (0..7)", "win17": "ssx_lk: unsupported window 17 (odd, 3..15) or max_level 3 (0..7)",
        "level8": "ssx_lk: unsupported window 11 (odd, 3..15) or max_level 8 (0..7)", "one_row": "ssx_lk: image 160x1 outside the supported range",
        "wide": "ssx_lk: image 8193x100 outside the supported range"}
GOOD = dict(slot=0, fresh=True, n=4)
# name -> (arguments of lk.debug_plan that differ from a good 100 x 160 call, the text that wins)
REFUSALS = {
    "stride": (dict(jobs=[dict(GOOD, next_stride=159)]), "stride"),
    "prev-stride": (dict(jobs=[dict(GOOD, prev_stride=100)]), "stride"),
    "slot-4096": (dict(jobs=[dict(GOOD, slot=4096)]), "slot"),
    "slot-twice": (dict(jobs=[GOOD, dict(GOOD, slot=1), dict(GOOD, slot=1)]), "twice"),
    "no-chain": (dict(jobs=[dict(slot=5, fresh=False, n=4)], slot_flags=[0]), "chain"),
    "key-change": (dict(jobs=[dict(slot=5, fresh=False, n=4)], slot_flags=[3], planned_key=(100, 160, 7, 3)), "chain"),
    "size-change": (dict(jobs=[dict(slot=5, fresh=False, n=4)], slot_flags=[3], planned_key=(101, 160, 11, 3)), "chain"),
    "even-window": (dict(win=10), "even"),
    "window-17": (dict(win=17), "win17"),
    "max-level-8": (dict(max_level=8), "level8"),
    "one-row": (dict(rows=1), "one_row"),
    "8193-columns": (dict(cols=8193), "wide"),
    # two at once: job checks before parameter checks before the image range, and the jobs one after the other
    "stride+even-window": (dict(jobs=[dict(GOOD, next_stride=159)], win=10), "stride"),
    "slot-twice+one-row": (dict(jobs=[GOOD, dict(GOOD, slot=1), dict(GOOD, slot=1)], rows=1), "twice"),
    "no-chain+even-window": (dict(jobs=[dict(slot=5, fresh=False, n=4)], slot_flags=[0], win=10), "chain"),
    "even-window+one-row": (dict(win=10, rows=1), "even"),
    "stride+slot-on-one-job": (dict(jobs=[dict(GOOD, slot=4096, next_stride=159)]), "stride"),
    "slot-then-stride": (dict(jobs=[dict(GOOD, slot=4096), dict(GOOD, slot=1, next_stride=159)]), "slot"),
    "stride-then-slot": (dict(jobs=[dict(GOOD, next_stride=159), dict(GOOD, slot=4096)]), "stride"),
    "twice-before-chain": (dict(jobs=[dict(GOOD, slot=1), dict(slot=1, fresh=False, n=4)], slot_flags=[0, 0]), "twice"),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusals_and_their_order(lib, which):
    kw, text = REFUSALS[which]
    kw = dict(dict(rows=100, cols=160, jobs=[GOOD]), **kw)
    p = lk.debug_plan(lib, kw.pop("rows"), kw.pop("cols"), kw.pop("jobs"), **kw)
    assert p.status == INVALID and p.error.decode() == TEXT[text], (p.status, p.error)
    assert p.levels == 0 and p.n_launches == 0 and p.io_bytes == 0


def test_a_negative_point_count_is_refused_without_a_text(lib):
    p = lk.debug_plan(lib, 100, 160, [dict(GOOD, n=-1)])
    assert p.status == INVALID and p.error == b""
    assert lk.debug_plan(lib, 100, 160, [GOOD]).status == _lib.SSX_OK    # the good call beside them
