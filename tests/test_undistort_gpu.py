"""GPU: ssx_undistort (csrc/undistort.hip: k_undistort) writes the bytes of its contract, tools/undistort_model.py -- array_equal, no
tolerance: the map is f64 operation by operation and everything behind its quantisation is integer.

The shapes are the smallest at which the kernel can go wrong: more than one workgroup in rows (48 > 4) and a row that is no multiple
of a thread's four pixels (67) or ends inside a wavefront's 256; a pitch that leaves rows dword-unaligned (dst stride 73: the byte-store
path) beside an aligned one (72); every border path (all taps inside / some / none); W != 1; one full-size pair for more than one
wavefront per row (1241 > 256)."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import undistort as ud
from tools import undistort_model as um

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)
K_A = (40.0, 40.0, 31.5, 23.5)
PINCUSHION = (0.25, 0.05, 0.0, 0.0, 0.0)
# name: (rows, cols, K, dist, src stride, dst stride, rotated)
CASES = {
    "barrel": (48, 64, K_A, (-0.3, 0.1, 0.0, 0.0, 0.0), None, None, False),
    "pincushion": (48, 64, K_A, PINCUSHION, None, None, False),
    "tangential": (45, 67, (38.0, 41.0, 30.2, 20.7), (-0.28, 0.07, 0.004, -0.003, 0.01), 80, 72, False),
    "small_third": (60, 80, (48.0, 48.0, 40.3, 29.6), (0.1, -0.2, 0.001, 0.0005, 0.05), None, None, False),
    "rotated": (48, 64, K_A, PINCUSHION, None, None, True),
}


def _image(rows, cols, seed, stride=None):
    """a textured image (never 0, so a border pixel is told from a sampled one) as the [rows, cols] view of a [rows, stride] buffer"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(1, 256, size=(rows, cols if stride is None else stride), dtype=np.uint8)
    return buf[:, :cols]


def _iR(K, rotated):
    return um.rotated_iR(K, *np.deg2rad([2.0, 2.0, 2.0])) if rotated else None


def _one(ctx, img, K, dist, iR=None, dst_stride=None):
    return ud.undistort(ctx, [img], [ud.make_params(K, dist, iR)], dst_stride=dst_stride)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_model(ctx, name):
    rows, cols, K, dist, ss, ds, rotated = CASES[name]
    img = _image(rows, cols, 11, ss)
    iR = _iR(K, rotated)
    want = um.undistort(img, K, dist, iR)
    got = _one(ctx, img, K, dist, iR, dst_stride=ds)
    assert np.array_equal(got, want)
    # the case is what its name says
    iu, iv = um.undistort_map(rows, cols, K, dist, iR)
    inside = um.all_taps_inside(rows, cols, iu, iv)
    X0, Y0 = iu >> 5, iv >> 5
    none = (X0 < -1) | (X0 >= cols) | (Y0 < -1) | (Y0 >= rows)
    if name == "barrel":
        assert inside.all()
    if name == "pincushion":
        assert 0.70 < inside.mean() < 0.80 and 0.15 < none.mean() < 0.25 and 0.02 < (~inside & ~none).mean() < 0.08
        assert not want[none].any() and want[inside].all()
    if name == "rotated":
        W = np.arange(cols)[None, :] * iR[6] + np.arange(rows)[:, None] * iR[7] + iR[8]
        assert np.ptp(W) > 0.05 and not np.array_equal(want, um.undistort(img, K, dist))


def test_an_unaligned_pitch_takes_byte_stores(ctx):
    """dst stride 73: three rows of four start off a dword boundary; src stride 81"""
    rows, cols, K, dist = 45, 67, (38.0, 41.0, 30.2, 20.7), (-0.28, 0.07, 0.004, -0.003, 0.01)
    img = _image(rows, cols, 12, 81)
    assert np.array_equal(_one(ctx, img, K, dist, dst_stride=73), um.undistort(img, K, dist))


def test_far_outside_but_finite(ctx):
    rows, cols = 48, 64
    img = _image(rows, cols, 13)
    dist = (50.0, 0.0, 0.0, 0.0, 0.0)
    want = um.undistort(img, K_A, dist)
    assert np.array_equal(_one(ctx, img, K_A, dist), want)
    assert (want == 0).mean() > 0.9 and want.any()


@pytest.mark.parametrize("dist", [(np.nan, 0, 0, 0, 0), (np.inf, 0, 0, 0, 0), (1e300, 1e300, 0, 0, 1e300), (-1e12, 0, 0, 0, 0)])
def test_non_finite_positions_are_ordinary(ctx, dist):
    """q's NaN case and clamp are the code's own: the kernel equals the model and nothing faults"""
    img = _image(48, 64, 14)
    assert np.array_equal(_one(ctx, img, K_A, dist), um.undistort(img, K_A, dist))
    iR = um.default_iR(K_A).copy(); iR[8] = 0.0                         # W = 0
    assert np.array_equal(_one(ctx, img, K_A, ZERO, iR), um.undistort(img, K_A, ZERO, iR))


@pytest.mark.parametrize("rows, cols", [(48, 64), (45, 67)])
def test_zero_coefficients_copy_the_image(ctx, rows, cols):
    img = _image(rows, cols, 15)
    assert np.array_equal(_one(ctx, img, K_A, ZERO), img)


@pytest.fixture(scope="module")
def full_pair():
    """376 x 1241 at KITTI's intrinsics read as float, left and right with different coefficients; the model's result, computed once"""
    from tools.synth import KITTI00_SETTINGS
    K = tuple(float(np.float32(KITTI00_SETTINGS["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))
    dists = [tuple(float(np.float32(v)) for v in d) + (0.0,) for d in ((-0.20, 0.03, 0.001, -0.0005), (-0.18, 0.02, -0.0008, 0.0004))]
    imgs = [_image(376, 1241, 16), _image(376, 1241, 17)]
    want = [um.undistort(im, K, d) for im, d in zip(imgs, dists)]
    for a, b in zip(imgs, want):
        a.setflags(write=False); b.setflags(write=False)
    return K, dists, imgs, want


def test_full_size_pair(ctx, full_pair):
    K, dists, imgs, want = full_pair
    got = ud.undistort(ctx, imgs, [ud.make_params(K, d) for d in dists])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(want[0], um.undistort(imgs[0], K, dists[1]))   # the two parameter sets are told apart


@pytest.fixture(scope="module")
def eight():
    """eight jobs of 45 x 67 with different images and parameters, and the model's results"""
    rng = np.random.default_rng(21)
    K = (38.0, 41.0, 30.2, 20.7)
    jobs = []
    for k in range(8):
        dist = (rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004), rng.uniform(-0.02, 0.02))
        Kk = tuple(np.array(K) + rng.uniform(-2, 2, 4))
        iR = um.rotated_iR(Kk, *np.deg2rad(rng.uniform(-2, 2, 3))) if k % 2 else None
        img = _image(45, 67, 30 + k)
        jobs.append((img, Kk, dist, iR, um.undistort(img, Kk, dist, iR)))
    return jobs


@pytest.mark.parametrize("n", [1, 2, 8])
def test_jobs_in_one_call_equal_the_single_calls(ctx, eight, n):
    jobs = eight[:n]
    prm = [ud.make_params(K, d, iR) for _, K, d, iR, _ in jobs]
    got = ud.undistort(ctx, [j[0] for j in jobs], prm)
    for k, j in enumerate(jobs):
        assert np.array_equal(got[k], j[4]), k                                        # the model
        assert np.array_equal(got[k], ud.undistort(ctx, [j[0]], [prm[k]])[0]), k      # the single call
    perm = np.random.default_rng(n).permutation(n)
    got_p = ud.undistort(ctx, [jobs[p][0] for p in perm], [prm[p] for p in perm])
    for k, p in enumerate(perm):
        assert np.array_equal(got_p[k], got[p])


def _host_alloc(lib, nbytes):
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    p = lib.ssx_host_alloc(nbytes)
    assert p
    return p, np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))


def test_pinned_buffers_read_and_written_in_place(ctx, eight):
    """ssx_host_alloc buffers with images_on_device = 1: the same bytes, written where the destination lies, pitch bytes untouched"""
    rows, cols, ss, ds = 45, 67, 80, 72
    n = 2
    p, arena = _host_alloc(ctx.lib, n * rows * (ss + ds))
    try:
        arena[:] = 0xAB
        jobs = []
        for k in range(n):
            src = arena[k * rows * ss:(k + 1) * rows * ss].reshape(rows, ss)
            src[:, :cols] = eight[k][0]
            off = n * rows * ss + k * rows * ds
            jobs.append((p + k * rows * ss, ss, p + off, ds, ud.make_params(*eight[k][1:4])))
        ud.undistort_ptrs(ctx, jobs, rows, cols, images_on_device=True)
        st = ud.last_call(ctx)
        assert st["bytes_down"] == 0 and st["launches"] == 1 and st["syncs"] == 1
        for k in range(n):
            dst = arena[n * rows * ss + k * rows * ds:n * rows * ss + (k + 1) * rows * ds].reshape(rows, ds)
            assert np.array_equal(dst[:, :cols], eight[k][4]), k
            assert (dst[:, cols:] == 0xAB).all()
            src = arena[k * rows * ss:(k + 1) * rows * ss].reshape(rows, ss)
            assert np.array_equal(src[:, :cols], eight[k][0]) and (src[:, cols:] == 0xAB).all()
    finally:
        ctx.lib.ssx_host_free(p)


def test_pitch_bytes_of_a_host_destination_are_untouched(ctx, eight):
    img, K, dist, iR, want = eight[1]
    rows, cols = img.shape
    buf = np.full((rows, 72), 0xCD, np.uint8)
    ud.undistort_ptrs(ctx, [(np.ascontiguousarray(img).ctypes.data, cols, buf.ctypes.data, 72, ud.make_params(K, dist, iR))], rows, cols, images_on_device=False)
    assert np.array_equal(buf[:, :cols], want) and (buf[:, cols:] == 0xCD).all()


def test_every_rejection_has_a_message_and_touches_nothing(ctx, eight):
    lib = ud._fns(ctx.lib)
    rows, cols = 45, 67
    src = np.ascontiguousarray(eight[0][0])
    other = np.ascontiguousarray(eight[1][0])
    dst = np.full((rows, cols), 0x5A, np.uint8)
    both = np.full((2 * rows, cols), 0x5A, np.uint8)                     # a source and a destination that overlap in their last / first row
    prm = ud.make_params(*eight[0][1:4])

    def call(n, jobs, r=rows, c=cols, null_table=False):
        arr = (_lib.UndistortJob * max(len(jobs), 1))()
        for k, (s, ss, d, ds) in enumerate(jobs):
            arr[k].src = s; arr[k].src_stride = ss; arr[k].dst = d; arr[k].dst_stride = ds; arr[k].prm = prm
        st = lib.ssx_undistort(ctx.handle, n, None if null_table else arr, r, c, 0)
        return st, lib.ssx_last_error(ctx.handle).decode()

    good = (src.ctypes.data, cols, dst.ctypes.data, cols)
    # name: (the call, what its message names)
    cases = {
        "n < 0": (call(-1, [good]), "n = -1"),
        "null table": (call(1, [good], null_table=True), "jobs is null"),
        "null src": (call(1, [(None, cols, dst.ctypes.data, cols)]), "job 0 has a null src"),
        "null dst": (call(1, [(src.ctypes.data, cols, None, cols)]), "job 0 has a null dst"),
        "null dst of the second job": (call(2, [good, (other.ctypes.data, cols, None, cols)]), "job 1 has a null dst"),
        "src stride": (call(1, [(src.ctypes.data, cols - 1, dst.ctypes.data, cols)]), "stride (src 66, dst 67)"),
        "dst stride": (call(1, [(src.ctypes.data, cols, dst.ctypes.data, cols - 1)]), "stride (src 67, dst 66)"),
        "rows": (call(1, [good], r=0), "rows = 0"),
        "cols": (call(1, [good], c=0), "cols = 0"),
        "negative rows": (call(1, [good], r=-3), "rows = -3"),
        "in place": (call(1, [(dst.ctypes.data, cols, dst.ctypes.data, cols)]), "dst of job 0 overlaps the src of job 0"),
        "overlap by one byte": (call(1, [(both.ctypes.data, cols, both.ctypes.data + rows * cols - 1, cols)]), "dst of job 0 overlaps the src of job 0"),
        "dst on another job's src": (call(2, [good, (other.ctypes.data, cols, src.ctypes.data, cols)]), "dst of job 1 overlaps the src of job 0"),
    }
    for name, ((st, msg), what) in cases.items():
        assert st == _lib.SSX_ERR_INVALID_ARG and msg.startswith("ssx_undistort:") and what in msg, (name, st, msg)
    assert lib.ssx_undistort(ctx.handle, 0, None, 1, 1, 0) == _lib.SSX_OK    # no jobs: nothing to do
    assert (dst == 0x5A).all() and (both == 0x5A).all()
    assert np.array_equal(src, eight[0][0]) and np.array_equal(other, eight[1][0])
    assert ud.last_call(ctx) == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0)
    # neighbours in one allocation that do not overlap are accepted: the destination begins where the source ends
    both[:rows] = src
    st, _ = call(1, [(both.ctypes.data, cols, both.ctypes.data + rows * cols, cols)])
    assert st == _lib.SSX_OK and np.array_equal(both[rows:], eight[0][4])


def test_launches_and_synchronisations_do_not_depend_on_n(ctx, eight):
    """one launch, one synchronisation, one copy each way, whatever n is (ssx_undistort_debug_last_call)"""
    stats = {}
    for n in (1, 2, 8, 64):
        jobs = [eight[k % 8] for k in range(n)]
        got = ud.undistort(ctx, [j[0] for j in jobs], [ud.make_params(*j[1:4]) for j in jobs])
        stats[n] = ud.last_call(ctx)
        assert all(np.array_equal(g, j[4]) for g, j in zip(got, jobs))
    for n, s in stats.items():
        assert s["launches"] == 1 and s["syncs"] == 1, (n, s)
        assert s["bytes_down"] == n * 45 * 68                            # the results at a dword pitch
        assert n * 45 * 67 <= s["bytes_up"] <= n * (45 * 67 + 256 + 256) + 256   # the sources and the job table, each block rounded to 256


def test_a_pinned_result_goes_straight_into_the_batched_tracker():
    """an ssx_host_alloc buffer filled by ssx_undistort (images_on_device = 1) is the input of ssx_lk_track_batch (images_on_device = 1):
    the tracks are those of the model's undistorted images handed over as ordinary host arrays.  (A context of its own: the LK call
    re-plans the context it runs on.)"""
    import ssvio_amd
    from ssvio_amd import lk
    from tools.synth import make_stereo_pair
    rows, cols = 200, 320
    L, R, _ = make_stereo_pair(seed=3, h=rows, w=cols, n_blobs=400)
    K, dist = (300.0, 300.0, 159.5, 99.5), (-0.1, 0.02, 0.0005, -0.0005, 0.0)
    want = [um.undistort(L, K, dist), um.undistort(R, K, dist)]
    xs, ys = np.meshgrid(np.arange(30, cols - 30, 20), np.arange(30, rows - 30, 20))
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    nb = rows * cols
    own = ssvio_amd.Context(0)
    p, arena = _host_alloc(own.lib, 4 * nb)
    try:
        arena[:nb] = L.reshape(-1); arena[nb:2 * nb] = R.reshape(-1)
        prm = ud.make_params(K, dist)
        ud.undistort_ptrs(own, [(p, cols, p + 2 * nb, cols, prm), (p + nb, cols, p + 3 * nb, cols, prm)], rows, cols, images_on_device=True)
        assert np.array_equal(arena[2 * nb:3 * nb].reshape(rows, cols), want[0]) and np.array_equal(arena[3 * nb:].reshape(rows, cols), want[1])
        got = lk.track_batch_ptrs(own, [dict(slot=0, prev=p + 2 * nb, next=p + 3 * nb, stride=cols, prev_pts=pts, next_pts=None)], rows, cols)[0]
        ref = lk.track_batch(own, [dict(slot=0, prev=want[0], next=want[1], prev_pts=pts, next_pts=None)])[0]
        assert ref[1].sum() > len(pts) // 2                               # the pair is trackable
        for g, r in zip(got, ref):
            assert g.tobytes() == r.tobytes()
    finally:
        own.lib.ssx_host_free(p)
        own.close()
