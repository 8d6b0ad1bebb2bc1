"""LK calls as data: the geometries and call sequences that tests/test_lk_plan.py plans without a GPU (ssx_lk_debug_plan), that
tests/test_lk_gpu.py::test_every_image_intake_gives_the_same_bits runs, and that tools/lk_call_trace.py replays under a profiler to
compare the launches and copies of two builds of the library.

A CASE is one context's life: an image size, a window, a max_level and a list of calls.  A CALL names the slots of its jobs, which of
them are fresh (both images given) and which chained (prev = NULL), the points per job, and the LAYOUT of its images:

    HOST           ordinary host arrays, images_on_device = 0
    ARENA          one pinned block, the jobs' `next` images sliced from it at a constant distance, ascending
    ARENA_SKIP     the same block with slice 1 left out (a stream that sits the call out)
    SEPARATE_HOST  a pinned block per image, the jobs listed in DESCENDING address order
    DEVICE         a device buffer per image, likewise descending
    ADJACENT_HOST  a pinned block per image which the allocator happened to lay out like an arena: ascending, at a constant distance,
                   close together -- pointer arithmetic cannot tell it from ARENA, only the runtime can (several allocations)
    ADJACENT_HOST_SKIP, ADJACENT_DEVICE   the same with slice 1 left out; the same in device memory

facts() turns a call into what ssx_lk_debug_plan is told: per job (slot, fresh, n, strides, next_off) + images_on_device + whether
jobs[0].next is host memory + whether the `next` images lie in ONE allocation."""

HOST, ARENA, ARENA_SKIP, SEPARATE_HOST, DEVICE = "host", "arena", "arena_skip", "separate_host", "device"
ADJACENT_HOST, ADJACENT_HOST_SKIP, ADJACENT_DEVICE = "adjacent_host", "adjacent_host_skip", "adjacent_device"
ADJACENT = (ADJACENT_HOST, ADJACENT_HOST_SKIP, ADJACENT_DEVICE)
STAGED, IN_ARENA, EACH, IN_PLACE = range(4)                       # ssx_lk_call_info.intake (include/ssx_test_hooks.h)

# (h, w, win, max_level): the nine of test_lk_gpu.py::test_pyramids_borders_and_chains_over_sizes_and_windows, the default parameters on a
# KITTI frame, and a five-level pyramid (more than k_lk_pyramid holds: the per-level kernels)
GEOMETRIES = [(120, 160, 11, 3), (121, 163, 11, 3), (97, 250, 7, 3), (113, 113, 15, 2), (200, 333, 5, 3), (64, 90, 11, 3), (111, 112, 11, 1),
              (130, 97, 13, 3), (376, 1241, 11, 2), (376, 1241, 11, 3), (240, 400, 11, 4)]


def call(slots, fresh, layout=HOST, n=20):
    slots = list(slots)
    return dict(slots=slots, fresh=[fresh] * len(slots) if isinstance(fresh, bool) else list(fresh), layout=layout,
                n=[n] * len(slots) if isinstance(n, int) else list(n))


def case(name, h, w, calls, win=11, max_level=3, intake=None, use_fused=None):
    return dict(name=name, h=h, w=w, win=win, max_level=max_level, calls=calls, intake=intake, use_fused=use_fused)


def _intake_cases():
    """every layout at the two sizes and job counts of the intake test: 3 jobs (k_lk_pyramid where the geometry allows) and 17 (above
    FUSED_MAX_JOBS); about 50 points a job, job 1 without points; a fresh call, then a chained one through the same layout"""
    out = []
    for h, w, ml in ((120, 168, 3), (240, 400, 4)):
        for nj in (3, 17):
            fused = ml == 3 and nj <= 16
            n = [0 if j == 1 else 47 + j for j in range(nj)]
            for layout in (HOST, ARENA, ARENA_SKIP, SEPARATE_HOST, DEVICE):
                want = {HOST: STAGED, ARENA: IN_ARENA, ARENA_SKIP: IN_ARENA, SEPARATE_HOST: EACH if fused else IN_PLACE, DEVICE: IN_PLACE}[layout]
                out.append(case(f"intake-{h}x{w}-{nj}jobs-{layout}", h, w, [call(range(nj), True, layout, n), call(range(nj), False, layout, n)],
                                max_level=ml, intake=want, use_fused=fused))
    return out


WIDE, FEW = 20, 4
CASES = [case(f"geom-{h}x{w}-win{win}-ml{ml}", h, w, [call([0], True), call([0], False)], win=win, max_level=ml) for h, w, win, ml in GEOMETRIES] + [
    # test_lk_gpu.py::test_wide_and_narrow_calls_interleave: wide -> narrow -> narrow -> wide -> narrow for other slots
    case("interleave", 120, 168, [call(range(WIDE), True, n=12), call(range(FEW), False, n=12), call(range(FEW), False, n=12),
                                  call(range(WIDE), False, n=12), call(range(FEW, 2 * FEW), False, n=12)]),
    # fresh and chained jobs in one call, listed in another order than their slots; one job without points
    case("mixed", 240, 400, [call([3, 0, 5], True, n=[30, 0, 41]), call([5, 3, 0], [False, True, False], n=[41, 30, 0])]),
    case("no-points", 120, 160, [call([0], True, n=0), call([0], False, n=0)]),
    # one job with images_on_device: never an arena; a pinned image in front of k_lk_pyramid comes over by a copy of its own
    case("single-pinned", 120, 168, [call([0], True, SEPARATE_HOST), call([0], False, SEPARATE_HOST)], intake=EACH, use_fused=True),
    case("single-device", 120, 168, [call([0], True, DEVICE), call([0], False, DEVICE)], intake=IN_PLACE, use_fused=True),
] + _intake_cases()


def _allocation_cases():
    """The layouts whose pointers pass the arena's arithmetic although every image is an allocation of its own (a cohort of two image
    sizes hands ssx_lk_track_batch exactly this: host/stream_batcher.cpp gives the streams of the larger size buffers of their own).
    2 and 3 jobs (k_lk_pyramid), 17 (the per-level kernels), a left-out slice; a fresh call, then a chained one.  `intake` is what
    the call takes when the runtime answers "several allocations"; with the answer "one" it is IN_ARENA (tests/test_lk_plan.py plans
    both).  These cases are planned only: tools/lk_call_trace.py cannot ask an allocator for such a layout."""
    out = []
    for nj in (2, 3, 17):
        fused = nj <= 16
        n = [0 if j == 1 else 47 + j for j in range(nj)]
        for layout in ADJACENT if nj > 2 else (ADJACENT_HOST, ADJACENT_DEVICE):
            out.append(case(f"allocations-120x168-{nj}jobs-{layout}", 120, 168, [call(range(nj), True, layout, n), call(range(nj), False, layout, n)],
                            intake=EACH if fused and layout != ADJACENT_DEVICE else IN_PLACE, use_fused=fused))
    return out


ALLOCATION_CASES = _allocation_cases()


def name(c):
    return c["name"]


def slice_bytes(c):
    """distance of two slices of an arena: one image, rounded up to 256 bytes"""
    return (c["h"] * c["w"] + 255) & ~255


def next_offsets(c, k):
    """the `next` pointers of a call's jobs relative to job 0's, as its layout places them"""
    nj, d = len(k["slots"]), slice_bytes(c)
    if k["layout"] == ARENA_SKIP:
        return [(j if j < 1 else j + 1) * d for j in range(nj)]
    if k["layout"] in ADJACENT:                                         # (a page of the allocator's own between two images)
        return [(j + 1 if j >= 1 and k["layout"] == ADJACENT_HOST_SKIP else j) * (d + 4096) for j in range(nj)]
    if k["layout"] in (SEPARATE_HOST, DEVICE):
        return [-j * (d + 4096) for j in range(nj)]                     # allocations of their own, descending
    return [j * d for j in range(nj)]


def facts(c, k):
    """-> (jobs for ssvio_amd.lk.debug_plan, images_on_device, next0_is_host, one_allocation)"""
    jobs = [dict(slot=s, fresh=f, n=n, next_off=o) for s, f, n, o in zip(k["slots"], k["fresh"], k["n"], next_offsets(c, k))]
    return jobs, int(k["layout"] != HOST), int(k["layout"] not in (DEVICE, ADJACENT_DEVICE)), int(k["layout"] not in ADJACENT)
