"""The host side of the pose-only and loop-pose calls without a GPU (ssx_po_debug_plan, include/ssx_test_hooks.h): what
ssx_pose_only_opt_batch / ssx_pose_only_debug_trace would do with a batch, and the one block of ssx_pnp_ransac / ssx_loop_pose_opt /
ssx_loop_compute_pose -- each against a restatement of the rules in the comments of ssvio_amd/csrc/pose_only.hpp (PoProblem, po_class),
pose_only.hip (PoBatchPlan, pose_only_generic) and pnp.hip (PnpBlock)."""
import itertools

import pytest

from ssvio_amd import _lib, ba

K2, K6, GENERIC, EMPTY = 0, 1, 2, 3
DESC_BYTES, TRACE_BYTES, RESULT_BYTES, HDR_BYTES = 144, 32, 72, 72      # sizeof PoDev, PoTrace, PoResult, PnpHdr
MS = (0, 1, 511, 512, 513, 1535, 1536, 1537, 4000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def r256(n):
    return (n + 255) & ~255


def cls_of(M):
    return EMPTY if M == 0 else K2 if M <= 512 else K6 if M <= 1536 else GENERIC


def problem_bytes(M):
    """xyz, uv, pose in (8 doubles), the generic kernel's err and level, the result record with its M flags"""
    scratch = M if M > 1536 else 0
    return dict(xyz=24 * M, uv=16 * M, pose_in=64, err=16 * scratch, level=scratch, result=RESULT_BYTES + M)


def check_spans(spans, block_bytes):
    """spans: (offset, bytes) in memory order: 256-aligned, inside the block, disjoint (each ends before the next begins)"""
    assert all(off % 256 == 0 for off, _ in spans)
    for (a, na), (b, _) in zip(spans, spans[1:]):
        assert a + na <= b
    assert spans[-1][0] + spans[-1][1] <= block_bytes
    full = [s for s in spans if s[1]]
    assert all(a + na <= b or b + nb <= a for (a, na), (b, nb) in itertools.combinations(full, 2))


def check_batch(lib, Ms, traced):
    p, _ = ba.po_debug_plan(lib, list(Ms), traced)
    assert p.n_jobs == len(Ms)
    jobs = [dict(cls=j.cls, block=j.block, **{s: (j.span_off[k], j.span_bytes[k]) for k, s in enumerate(ba.PO_SPANS)}) for j in p.job[:len(Ms)]]
    assert [j["cls"] for j in jobs] == [cls_of(M) for M in Ms]
    # descriptors: class 0 first, then class 1, job order inside a class; the generic jobs follow in job order, a block each
    reg = [i for c in (K2, K6) for i, M in enumerate(Ms) if cls_of(M) == c]
    gen = [i for i, M in enumerate(Ms) if cls_of(M) == GENERIC]
    n2 = sum(cls_of(M) == K2 for M in Ms)
    first_gen = 1 if reg else 0
    assert p.n_blocks == first_gen + len(gen)
    want = ([(K2, n2, 0, 0)] if n2 else []) + ([(K6, len(reg) - n2, 0, n2)] if len(reg) > n2 else []) + [(GENERIC, 1, first_gen + k, -1) for k in range(len(gen))]
    assert [(l.cls, l.grid, l.block, l.first_desc) for l in p.launch[:p.n_launches]] == want
    assert len([l for l in want if l[0] != GENERIC]) <= 2
    for i, M in enumerate(Ms):
        j = jobs[i]
        if cls_of(M) == EMPTY:
            assert j["block"] == -1 and all(j[s] == (0, 0) for s in ba.PO_SPANS)
            continue
        assert {s: j[s][1] for s in ba.PO_SPANS} == problem_bytes(M)
        assert (j["err"][1] > 0) == (j["level"][1] > 0) == (M > 1536)
    if reg:
        b = p.block[0]
        assert all(jobs[i]["block"] == 0 for i in reg)
        assert (b.desc_off, b.desc_bytes) == (0, DESC_BYTES * len(reg))
        assert b.trace_bytes == (TRACE_BYTES * len(reg) if traced else 0)      # the shipped entry points' block carries no record table
        spans = [(b.desc_off, b.desc_bytes)] + [jobs[i][s] for i in reg for s in ba.PO_SPANS] + [(b.trace_off, b.trace_bytes)]
        check_spans(spans, b.bytes)
        assert b.bytes == sum(r256(n) for _, n in spans)
        assert (b.sent, b.ret_off, b.ret_bytes) == (0, 0, 0)                 # pinned, read and written in place: no copy
    for k, i in enumerate(gen):
        b, j = p.block[first_gen + k], jobs[i]
        assert j["block"] == first_gen + k
        assert (b.desc_bytes, b.trace_bytes) == (0, 0)                        # descriptor and record go over by value
        spans = [j[s] for s in ba.PO_SPANS]
        check_spans(spans, b.bytes)
        assert b.bytes == sum(r256(n) for _, n in spans)
        for s in ("xyz", "uv", "pose_in"):                                    # what is sent lies inside the prefix, and nothing else does
            assert j[s][0] + j[s][1] <= b.sent
        assert b.sent == j["pose_in"][0] + r256(64) == j["err"][0]
        assert (b.ret_off, b.ret_bytes) == j["result"]                        # what comes back is the record and its flags, exactly


@pytest.mark.parametrize("traced", [False, True])
def test_mixed_batch(lib, traced):
    check_batch(lib, MS, traced)
    check_batch(lib, MS[::-1], traced)
    check_batch(lib, (600, 3, 2000, 0, 700, 5, 1537), traced)                # classes interleaved: job order inside each


@pytest.mark.parametrize("traced", [False, True])
@pytest.mark.parametrize("M", MS)
def test_single_job(lib, M, traced):
    check_batch(lib, (M,), traced)


def test_empty_batches(lib):
    for Ms in ((), (0,), (0, 0)):
        p, _ = ba.po_debug_plan(lib, list(Ms), False)
        assert (p.n_blocks, p.n_launches) == (0, 0)


@pytest.mark.parametrize("tap", [0, 1])
@pytest.mark.parametrize("H", [1, 256])
@pytest.mark.parametrize("M", [3, 10, 1536, 1537])
def test_pnp_plan(lib, M, H, tap):
    _, p = ba.po_debug_plan(lib, pnp=(M, H, tap))
    span = {s: (p.span_off[k], p.span_bytes[k]) for k, s in enumerate(ba.PNP_SPANS)}
    assert p.refine_cls == cls_of(M)
    want = dict(problem_bytes(M), best=16, header=HDR_BYTES, mask=M, counts=4 * H if tap else 0, descriptor=DESC_BYTES)
    assert {s: n for s, (_, n) in span.items()} == want
    assert (span["counts"][1] > 0) == bool(tap) and (span["err"][1] > 0) == (span["level"][1] > 0) == (M > 1536)
    order = [span[s] for s in ba.PNP_SPANS]
    check_spans(order, p.bytes)                                               # (the descriptor slot among them: disjoint from everything)
    assert p.bytes == sum(r256(n) for _, n in order) and span["best"][0] == 0
    for s in ("best", "xyz", "uv", "pose_in"):                                # one copy up: everything that is sent, and nothing else
        assert span[s][0] + span[s][1] <= p.sent
    assert p.sent == span["pose_in"][0] + r256(64)
    for s in ("err", "level", "result", "header", "mask", "counts", "descriptor"):
        assert span[s][0] >= p.sent
    # one copy down: the refinement's record with its flags, the RANSAC's header and its mask -- one run, nothing else in it
    assert p.ret_off == span["result"][0] and p.ret_off + p.ret_bytes == span["mask"][0] + M
    assert span["result"][0] + r256(RESULT_BYTES + M) == span["header"][0] and span["header"][0] + r256(HDR_BYTES) == span["mask"][0]
    for s in ("best", "xyz", "uv", "pose_in", "err", "level", "counts", "descriptor"):
        assert span[s][0] + span[s][1] <= p.ret_off or span[s][0] >= p.ret_off + p.ret_bytes


def test_refusals(lib):
    for Ms in ([-1], [1] * 17):
        with pytest.raises(ValueError):
            ba.po_debug_plan(lib, Ms)
    with pytest.raises(ValueError):
        ba.po_debug_plan(lib, pnp=(-1, 1, 0))
