"""GPU: the undistortion plan (csrc/undistort.hip: k_undistort_map, k_undistort_remap, ssx_undistort_plan_*) writes the bytes of its
contract, tools/undistort_model.py -- array_equal, no tolerance.  Expected bytes come from the model (um.undistort, um.pack_map), never
from the library; that ssx_undistort gives the same bytes is asserted beside it.

The shapes are the smallest at which the kernels can go wrong: more than one workgroup in rows (48 > 4), a row that is no multiple of a
thread's four pixels (67), an image narrower than two threads (5 x 7: the row tail only), pitches that leave rows dword-unaligned
(dst 73: the byte stores), every border path (all taps inside / some / none / all positions clamped), one full-size pair for more than
one wavefront per row (1241 > 256)."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import undistort as ud
from tools import undistort_model as um

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
K_A = (40.0, 40.0, 31.5, 23.5)
K_T = (38.0, 41.0, 30.2, 20.7)
TANGENTIAL = (-0.28, 0.07, 0.004, -0.003, 0.01)
PINCUSHION = (0.25, 0.05, 0.0, 0.0, 0.0)
# name: (rows, cols, K, dist, kind of iR)
MAPS = {
    "barrel": (48, 64, K_A, (-0.3, 0.1, 0.0, 0.0, 0.0), None),
    "pincushion": (48, 64, K_A, PINCUSHION, None),
    "tangential with k3": (45, 67, K_T, TANGENTIAL, None),
    "rotated": (48, 64, K_A, PINCUSHION, "rotated"),
    "far outside": (48, 64, K_A, (50.0, 0.0, 0.0, 0.0, 0.0), None),
    "nan": (48, 64, K_A, (np.nan, 0, 0, 0, 0), None),
    "inf": (48, 64, K_A, (np.inf, 0, 0, 0, 0), None),
    "1e300": (48, 64, K_A, (1e300, 1e300, 0, 0, 1e300), None),
    "-1e12": (48, 64, K_A, (-1e12, 0, 0, 0, 0), None),
    "W = 0": (48, 64, K_A, ZERO, "w0"),
    "5 x 7": (5, 7, (6.0, 6.0, 3.0, 2.0), (-0.2, 0.05, 0.001, -0.001, 0.0), None),
}


def _iR(K, kind):
    if kind == "rotated":
        return um.rotated_iR(K, *np.deg2rad([2.0, 2.0, 2.0]))
    if kind == "w0":
        iR = um.default_iR(K).copy()
        iR[8] = 0.0
        return iR
    return None


def _image(rows, cols, seed, stride=None):
    """a textured image (never 0, so a border pixel is told from a sampled one) as the [rows, cols] view of a [rows, stride] buffer"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(1, 256, size=(rows, cols if stride is None else stride), dtype=np.uint8)
    return buf[:, :cols]


@pytest.mark.parametrize("name", list(MAPS))
def test_the_stored_map_and_its_image_equal_the_model(ctx, name):
    rows, cols, K, dist, kind = MAPS[name]
    iR = _iR(K, kind)
    prm = ud.make_params(K, dist, iR)
    img = _image(rows, cols, 11)
    with ud.UndistortPlan(ctx, rows, cols) as plan:
        m = plan.add(prm)
        assert m == 0 and plan.size() == (rows, cols, 1)
        assert plan.last_call() == dict(launches=1, syncs=1, bytes_up=0, bytes_down=0, copies_up=0, copies_down=0)
        want_map = um.pack_map(rows, cols, *um.undistort_map(rows, cols, K, dist, iR))
        for got, want, plane in zip(plan.packed_map(m), want_map, ("xs", "ys", "ab")):
            assert np.array_equal(got, want), plane
        want = um.undistort(img, K, dist, iR)
        got = plan.apply([img], [m])[0]
        assert np.array_equal(got, want)
        assert np.array_equal(got, ud.undistort(ctx, [img], [prm])[0])          # the inline form on the same inputs
    if name == "far outside":
        assert (want == 0).mean() > 0.9 and want.any()
    if name == "barrel":
        assert want.all()


@pytest.mark.parametrize("rows, cols", [(48, 64), (45, 67), (5, 7)])
def test_zero_coefficients_copy_the_image(ctx, rows, cols):
    img = _image(rows, cols, 15)
    with ud.UndistortPlan(ctx, rows, cols) as plan:
        assert np.array_equal(plan.apply([img], [plan.add(ud.make_params(K_A, ZERO))])[0], img)


def test_unaligned_pitches_take_byte_stores_and_leave_the_pitch_bytes(ctx):
    """src stride 81, dst stride 73 at 45 x 67: three rows of four start off a dword boundary"""
    rows, cols = 45, 67
    img = _image(rows, cols, 12, 81)
    want = um.undistort(img, K_T, TANGENTIAL)
    with ud.UndistortPlan(ctx, rows, cols) as plan:
        m = plan.add(ud.make_params(K_T, TANGENTIAL))
        assert np.array_equal(plan.apply([img], [m], dst_stride=73)[0], want)
        buf = np.full((rows, 73), 0xCD, np.uint8)
        plan.apply_ptrs([(img.ctypes.data, 81, buf.ctypes.data, 73, m)], images_on_device=False)
        assert np.array_equal(buf[:, :cols], want) and (buf[:, cols:] == 0xCD).all()


@pytest.fixture(scope="module")
def three():
    """45 x 67: four parameter sets (the third is shown to the plan and never used), eight images, and the model's result of every
    image under every used set, computed once"""
    rng = np.random.default_rng(21)
    sets = []
    for k in range(4):
        dist = (rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004), rng.uniform(-0.02, 0.02))
        Kk = tuple(np.array(K_T) + rng.uniform(-2, 2, 4))
        iR = um.rotated_iR(Kk, *np.deg2rad(rng.uniform(-2, 2, 3))) if k % 2 else None
        sets.append((Kk, dist, iR))
    imgs = [_image(45, 67, 30 + k) for k in range(8)]
    used = (0, 1, 3)
    want = {(i, s): um.undistort(imgs[i], *sets[s]) for i in range(8) for s in used}
    for a in list(want.values()) + imgs:
        a.setflags(write=False)
    assert not np.array_equal(want[(0, 0)], want[(0, 1)]) and not np.array_equal(want[(0, 1)], want[(0, 3)])   # the maps are told apart
    return sets, imgs, used, want


@pytest.fixture()
def plan3(ctx, three):
    sets = three[0]
    with ud.UndistortPlan(ctx, 45, 67) as plan:
        assert [plan.add(ud.make_params(*s)) for s in sets] == [0, 1, 2, 3]
        yield plan


def _assign(n, used, seed):
    """job k: (image, map) -- the maps in permuted order, several jobs sharing one"""
    rng = np.random.default_rng(seed)
    return [(k % 8, int(used[rng.integers(0, len(used))]) if n > 2 else used[(k + 1) % 3]) for k in range(n)]


def test_jobs_over_three_maps_and_the_counts_do_not_depend_on_n(ctx, three, plan3):
    sets, imgs, used, want = three
    stats = {}
    for n in (1, 2, 8, 64):
        jm = _assign(n, used, n)
        got = plan3.apply([imgs[i] for i, _ in jm], [m for _, m in jm])
        stats[n] = plan3.last_call()
        for k, (i, m) in enumerate(jm):
            assert np.array_equal(got[k], want[(i, m)]), (n, k)
        if n >= 8:
            assert len({m for _, m in jm}) == 3 and 2 not in {m for _, m in jm}
    prm = [ud.make_params(*s) for s in sets]
    jm = _assign(8, used, 8)
    single = ud.undistort(ctx, [imgs[i] for i, _ in jm], [prm[m] for _, m in jm])
    assert all(np.array_equal(single[k], want[(i, m)]) for k, (i, m) in enumerate(jm))
    for n, s in stats.items():
        assert s["launches"] == 1 and s["syncs"] == 1 and s["copies_up"] == 1 and s["copies_down"] == 1, (n, s)
        assert n * 45 * 68 <= s["bytes_down"] <= n * (45 * 68 + 256)          # the results at a dword pitch, each block rounded to 256
        assert n * 45 * 67 <= s["bytes_up"] <= n * (45 * 67 + 256 + 256) + 256
    assert plan3.size() == (45, 67, 4)


def test_equal_parameter_bytes_share_a_map_and_launch_nothing(ctx, three, plan3):
    sets = three[0]
    before = [np.array(p) for p in plan3.packed_map(1)]
    assert plan3.add(ud.make_params(*sets[1])) == 1
    assert plan3.last_call() == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0, copies_up=0, copies_down=0)
    assert plan3.add(ud.make_params(*sets[3])) == 3 and plan3.size() == (45, 67, 4)
    other = list(sets[1][1]); other[4] = np.nextafter(other[4], 1.0)        # one bit of k3: a new set
    assert plan3.add(ud.make_params(sets[1][0], tuple(other), sets[1][2])) == 4
    assert plan3.last_call()["launches"] == 1 and plan3.size() == (45, 67, 5)
    assert all(np.array_equal(a, b) for a, b in zip(before, plan3.packed_map(1)))


def test_more_maps_than_the_limit_are_refused(ctx):
    with ud.UndistortPlan(ctx, 5, 7) as plan:
        for k in range(_lib.SSX_UNDISTORT_PLAN_MAX_MAPS):
            assert plan.add(ud.make_params(K_A, (0.001 * k, 0, 0, 0, 0))) == k
        m = C.c_int32(-7)
        st = plan.lib.ssx_undistort_plan_add(plan.handle, C.byref(ud.make_params(K_A, (0.5, 0, 0, 0, 0))), C.byref(m))
        msg = plan.lib.ssx_last_error(ctx.handle).decode()
        assert st == _lib.SSX_ERR_CAPACITY and msg.startswith("ssx_undistort_plan_add:") and "64" in msg and m.value == -7
        assert plan.size() == (5, 7, _lib.SSX_UNDISTORT_PLAN_MAX_MAPS)
        assert plan.add(ud.make_params(K_A, (0.003, 0, 0, 0, 0))) == 3         # a set the plan holds is still found


def _host_alloc(lib, nbytes):
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    p = lib.ssx_host_alloc(nbytes)
    assert p
    return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))


def test_an_arena_goes_in_one_copy_each_way_and_nothing_between_the_images_is_written(ctx, three, plan3):
    """ssx_host_alloc arena, images_on_device = 1: the sources in slices of 3072 bytes (45 * 67 = 3015: 57 bytes between two images), the
    destinations behind them likewise; the bytes between the destinations keep what they held"""
    sets, imgs, used, want = three
    rows, cols, slice_ = 45, 67, 3072
    for n in (2, 8):
        jm = _assign(n, used, 50 + n)
        p, arena = _host_alloc(ctx.lib, 2 * n * slice_)
        try:
            arena[:] = 0xAB
            for k, (i, _) in enumerate(jm):
                arena[k * slice_:k * slice_ + rows * cols] = imgs[i].reshape(-1)
            plan3.apply_ptrs([(p + k * slice_, cols, p + (n + k) * slice_, cols, m) for k, (_, m) in enumerate(jm)], images_on_device=True)
            st = plan3.last_call()
            assert st["launches"] == 1 and st["syncs"] == 1 and st["copies_up"] == 1 and st["copies_down"] == 1, st
            assert st["bytes_down"] == n * rows * cols
            for k, (i, m) in enumerate(jm):
                d = arena[(n + k) * slice_:(n + k + 1) * slice_]
                assert np.array_equal(d[:rows * cols].reshape(rows, cols), want[(i, m)]), (n, k)
                assert (d[rows * cols:] == 0xAB).all()
                s = arena[k * slice_:(k + 1) * slice_]
                assert np.array_equal(s[:rows * cols].reshape(rows, cols), imgs[i]) and (s[rows * cols:] == 0xAB).all()
        finally:
            ctx.lib.ssx_host_free(p)


def test_pitched_or_unevenly_spaced_arena_images_go_one_by_one_with_the_same_bytes(ctx, three, plan3):
    """destinations at a pitch of 73 (their pitch bytes must stay) and at uneven distances: no single copy down; the sources still form a
    range"""
    sets, imgs, used, want = three
    rows, cols, ss, ds, n = 45, 67, 80, 73, 3
    jm = _assign(8, used, 61)[:n]
    src_off = [0, rows * ss, 2 * rows * ss + 128]
    dst_off = [4 * rows * ss, 4 * rows * ss + rows * ds + 64, 4 * rows * ss + 3 * rows * ds]
    p, arena = _host_alloc(ctx.lib, dst_off[-1] + rows * ds)
    try:
        arena[:] = 0xAB
        for k, (i, _) in enumerate(jm):
            arena[src_off[k]:src_off[k] + rows * ss].reshape(rows, ss)[:, :cols] = imgs[i]
        plan3.apply_ptrs([(p + src_off[k], ss, p + dst_off[k], ds, m) for k, (_, m) in enumerate(jm)], images_on_device=True)
        st = plan3.last_call()
        assert st["launches"] == 1 and st["syncs"] == 1 and st["copies_up"] == 1 and st["copies_down"] == n, st
        for k, (i, m) in enumerate(jm):
            d = arena[dst_off[k]:dst_off[k] + rows * ds].reshape(rows, ds)
            assert np.array_equal(d[:, :cols], want[(i, m)]), k
            assert (d[:, cols:] == 0xAB).all()
        assert (arena[dst_off[0] + rows * ds:dst_off[1]] == 0xAB).all()
    finally:
        ctx.lib.ssx_host_free(p)


def test_separately_allocated_pinned_images_and_device_images(ctx, three, plan3):
    """pinned images allocated one by one are copied one by one, however they stand (no copy may cross from one allocation into the
    next); device images are used where they lie and nothing is copied"""
    import torch
    sets, imgs, used, want = three
    rows, cols, n = 45, 67, 4
    jm = _assign(8, used, 71)[:n]
    bufs = [_host_alloc(ctx.lib, rows * cols) for _ in range(2 * n)]
    try:
        order = sorted(range(n), key=lambda k: bufs[k][0])                   # ascending, as an arena's slices would stand
        src = [bufs[k] for k in order]
        dst = sorted(bufs[n:], key=lambda b: b[0])
        for k, (i, _) in enumerate(jm):
            src[k][1][:] = imgs[i].reshape(-1)
            dst[k][1][:] = 0
        plan3.apply_ptrs([(src[k][0], cols, dst[k][0], cols, m) for k, (_, m) in enumerate(jm)], images_on_device=True)
        st = plan3.last_call()
        assert st["launches"] == 1 and st["syncs"] == 1 and st["copies_up"] == n and st["copies_down"] == n, st
        for k, (i, m) in enumerate(jm):
            assert np.array_equal(dst[k][1].reshape(rows, cols), want[(i, m)]), k
    finally:
        for p, _ in bufs:
            ctx.lib.ssx_host_free(p)
    # device memory: one allocation for the sources, one for the results
    d_src = torch.from_numpy(np.stack([imgs[i] for i, _ in jm])).to("cuda:0")
    d_dst = torch.zeros((n, rows, cols), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    plan3.apply_ptrs([(d_src.data_ptr() + k * rows * cols, cols, d_dst.data_ptr() + k * rows * cols, cols, m) for k, (_, m) in enumerate(jm)], images_on_device=True)
    st = plan3.last_call()
    assert st["launches"] == 1 and st["syncs"] == 1 and st["copies_up"] == 0 and st["copies_down"] == 0 and st["bytes_down"] == 0, st
    got = d_dst.cpu().numpy()
    for k, (i, m) in enumerate(jm):
        assert np.array_equal(got[k], want[(i, m)]), k
    # one device image to a pinned destination: one copy down, none up
    p, out = _host_alloc(ctx.lib, rows * cols)
    try:
        out[:] = 0
        plan3.apply_ptrs([(d_src.data_ptr(), cols, p, cols, jm[0][1])], images_on_device=True)
        st = plan3.last_call()
        assert st["copies_up"] == 0 and st["copies_down"] == 1 and st["syncs"] == 1
        assert np.array_equal(out.reshape(rows, cols), want[jm[0]])
    finally:
        ctx.lib.ssx_host_free(p)


@pytest.mark.parametrize("stride", [1_000_000_000, 2_000_000_000])
def test_source_offsets_past_2_31_and_past_2_32(ctx, stride):
    """a tap's byte offset is 64-bit: four rows at a pitch of 1e9 (the last row begins past 2^31) and of 2e9 (past 2^32), in device memory
    that is allocated and, but for the four rows, never touched.  Barrel coefficients: every pixel samples, and the last rows are read."""
    import torch
    rows, cols = 4, 64
    K, dist = (40.0, 40.0, 31.5, 1.5), (-0.3, 0.1, 0.0, 0.0, 0.0)
    img = _image(rows, cols, 91)
    want = um.undistort(img, K, dist)
    assert want[rows - 1].all() and not np.array_equal(want, img)
    src = torch.empty((rows - 1) * stride + cols, dtype=torch.uint8, device="cuda:0")
    for r in range(rows):
        src[r * stride:r * stride + cols] = torch.from_numpy(np.ascontiguousarray(img[r])).to("cuda:0")
    dst = torch.zeros((rows, cols), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with ud.UndistortPlan(ctx, rows, cols) as plan:
        plan.apply_ptrs([(src.data_ptr(), stride, dst.data_ptr(), cols, plan.add(ud.make_params(K, dist)))], images_on_device=True)
        assert np.array_equal(dst.cpu().numpy(), want)
    del src
    torch.cuda.empty_cache()


def test_every_rejection_has_a_message_and_touches_nothing(ctx, three, plan3):
    sets, imgs, used, want = three
    lib = plan3.lib
    rows, cols = 45, 67
    src = np.ascontiguousarray(imgs[0])
    other = np.ascontiguousarray(imgs[1])
    dst = np.full((rows, cols), 0x5A, np.uint8)
    both = np.full((2 * rows, cols), 0x5A, np.uint8)
    maps_before = [[np.array(p) for p in plan3.packed_map(m)] for m in range(4)]

    def call(n, jobs, null_table=False, on_device=0):
        arr = (_lib.UndistortPlanJob * max(len(jobs), 1))()
        for k, (s, ss, d, ds, m) in enumerate(jobs):
            arr[k].src = s; arr[k].src_stride = ss; arr[k].dst = d; arr[k].dst_stride = ds; arr[k].map = m
        st = lib.ssx_undistort_plan_apply(plan3.handle, n, None if null_table else arr, on_device)
        return st, lib.ssx_last_error(ctx.handle).decode()

    good = (src.ctypes.data, cols, dst.ctypes.data, cols, 0)
    cases = {
        "n < 0": (call(-1, [good]), "n = -1"),
        "n above the limit": (call(_lib.SSX_UNDISTORT_MAX_JOBS + 1, [good]), "n = 1025"),
        "null table": (call(1, [good], null_table=True), "jobs is null"),
        "null src": (call(1, [(None, cols, dst.ctypes.data, cols, 0)]), "job 0 has a null src"),
        "null dst": (call(1, [(src.ctypes.data, cols, None, cols, 0)]), "job 0 has a null dst"),
        "null dst of the second job": (call(2, [good, (other.ctypes.data, cols, None, cols, 1)]), "job 1 has a null dst"),
        "src stride": (call(1, [(src.ctypes.data, cols - 1, dst.ctypes.data, cols, 0)]), "stride (src 66, dst 67)"),
        "dst stride": (call(1, [(src.ctypes.data, cols, dst.ctypes.data, cols - 1, 0)]), "stride (src 67, dst 66)"),
        "map the plan does not hold": (call(1, [(src.ctypes.data, cols, dst.ctypes.data, cols, 4)]), "job 0 names map 4, the plan holds 4"),
        "negative map": (call(2, [good, (other.ctypes.data, cols, both.ctypes.data, cols, -1)]), "job 1 names map -1"),
        "in place": (call(1, [(dst.ctypes.data, cols, dst.ctypes.data, cols, 0)]), "dst of job 0 overlaps the src of job 0"),
        "overlap by one byte": (call(1, [(both.ctypes.data, cols, both.ctypes.data + rows * cols - 1, cols, 0)]), "dst of job 0 overlaps the src of job 0"),
        "dst on another job's src": (call(2, [good, (other.ctypes.data, cols, src.ctypes.data, cols, 1)]), "dst of job 1 overlaps the src of job 0"),
        "pageable memory as device memory": (call(1, [good], on_device=1), "src of job 0 is neither device memory nor pinned host memory"),
    }
    for name, ((st, msg), what) in cases.items():
        assert st == _lib.SSX_ERR_INVALID_ARG and msg.startswith("ssx_undistort_plan_apply:") and what in msg, (name, st, msg)
        assert plan3.last_call() == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0, copies_up=0, copies_down=0), name
    assert lib.ssx_undistort_plan_apply(plan3.handle, 0, None, 0) == _lib.SSX_OK     # no jobs: nothing to do
    assert (dst == 0x5A).all() and (both == 0x5A).all()
    assert np.array_equal(src, imgs[0]) and np.array_equal(other, imgs[1])
    assert plan3.size() == (45, 67, 4)
    for m in range(4):
        assert all(np.array_equal(a, b) for a, b in zip(maps_before[m], plan3.packed_map(m)))
    # a plan is refused for a side above 65533 (unsupported) and for an empty image (invalid), both with a message
    for shape, status, what in (((65534, 4), _lib.SSX_ERR_UNSUPPORTED, "65533"), ((4, 65534), _lib.SSX_ERR_UNSUPPORTED, "65533"), ((0, 4), _lib.SSX_ERR_INVALID_ARG, "rows = 0")):
        h = C.c_void_p()
        assert lib.ssx_undistort_plan_create(ctx.handle, shape[0], shape[1], C.byref(h)) == status and not h.value
        msg = lib.ssx_last_error(ctx.handle).decode()
        assert msg.startswith("ssx_undistort_plan_create:") and what in msg, msg
    # neighbours in one allocation that do not overlap are accepted: the destination begins where the source ends
    both[:rows] = src
    st, _ = call(1, [(both.ctypes.data, cols, both.ctypes.data + rows * cols, cols, 0)])
    assert st == _lib.SSX_OK and np.array_equal(both[rows:], want[(0, 0)])


def test_two_plans_of_two_sizes_on_one_context_stay_independent(ctx, three):
    sets, imgs, used, want = three
    small = _image(5, 7, 81)
    K_S, D_S = (6.0, 6.0, 3.0, 2.0), (-0.2, 0.05, 0.001, -0.001, 0.0)
    with ud.UndistortPlan(ctx, 45, 67) as a, ud.UndistortPlan(ctx, 5, 7) as b:
        ma = a.add(ud.make_params(*sets[1]))
        mb = b.add(ud.make_params(K_S, D_S))
        assert (ma, mb) == (0, 0) and a.size() == (45, 67, 1) and b.size() == (5, 7, 1)
        for _ in range(2):                                                   # alternating: neither call disturbs the other plan
            assert np.array_equal(a.apply([imgs[2]], [ma])[0], want[(2, 1)])
            assert np.array_equal(b.apply([small], [mb])[0], um.undistort(small, K_S, D_S))
        assert a.add(ud.make_params(*sets[3])) == 1 and b.size() == (5, 7, 1)
        assert np.array_equal(a.apply([imgs[2], imgs[4]], [1, 0]), [want[(2, 3)], want[(4, 1)]])
        with pytest.raises(ValueError):
            b.apply([imgs[2]], [mb])                                        # an image of the other plan's size


@pytest.fixture(scope="module")
def full_pair():
    """376 x 1241 at KITTI's intrinsics read as float, left and right with different coefficients; the model's result, computed once"""
    from tools.synth import KITTI00_SETTINGS
    K = tuple(float(np.float32(KITTI00_SETTINGS["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))
    dists = [tuple(float(np.float32(v)) for v in d) + (0.0,) for d in ((-0.20, 0.03, 0.001, -0.0005), (-0.18, 0.02, -0.0008, 0.0004))]
    imgs = [_image(376, 1241, 16), _image(376, 1241, 17)]
    want = [um.undistort(im, K, d) for im, d in zip(imgs, dists)]
    return K, dists, imgs, want


def test_full_size_pair(ctx, full_pair):
    K, dists, imgs, want = full_pair
    with ud.UndistortPlan(ctx, 376, 1241) as plan:
        maps = [plan.add(ud.make_params(K, d)) for d in dists]
        assert maps == [0, 1]
        got = plan.apply(imgs, maps)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        swapped = plan.apply(imgs, maps[::-1])
        assert not np.array_equal(swapped[0], want[0])                      # the two maps are told apart
        # the pair in a pinned arena, slices rounded to 256 bytes as a cohort's are: one copy each way
        nb, sl = 376 * 1241, (376 * 1241 + 255) & ~255
        p, arena = _host_alloc(ctx.lib, 4 * sl)
        try:
            arena[:] = 0xAB
            for k in (0, 1):
                arena[k * sl:k * sl + nb] = imgs[k].reshape(-1)
            plan.apply_ptrs([(p + k * sl, 1241, p + (2 + k) * sl, 1241, maps[k]) for k in (0, 1)], images_on_device=True)
            st = plan.last_call()
            assert st["copies_up"] == 1 and st["copies_down"] == 1 and st["launches"] == 1 and st["syncs"] == 1
            for k in (0, 1):
                assert np.array_equal(arena[(2 + k) * sl:(2 + k) * sl + nb].reshape(376, 1241), want[k])
                assert (arena[(2 + k) * sl + nb:(3 + k) * sl] == 0xAB).all()
        finally:
            ctx.lib.ssx_host_free(p)
