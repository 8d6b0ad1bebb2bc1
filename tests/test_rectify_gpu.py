"""GPU: ssx_undistort_lens (csrc/undistort.hip: k_undistort with a lens model per job) writes the bytes of its contract,
tools/rectify_model.py -- array_equal, no tolerance: the map is f64 operation by operation, atan_c included, and everything behind its
quantisation is integer.  The device's atan_c and sqrt are compared bit for bit on their own through ssx_lens_debug_atan.

The shapes are those tests/test_undistort_gpu.py argues for: more than one workgroup in rows (48 > 4), a row that is no multiple of a
thread's four pixels (67), a pitch that leaves rows dword-unaligned (dst stride 73) beside an aligned one (72), every border path (all
taps inside / some / none), more than one wavefront a row (300 > 256); and what the KB4 lens adds: rays behind the camera (W <= 0)
and non-finite coefficients.  iR is rectify()'s of a rig rotated by (1.5, -2, 1) degrees, so W != 1 everywhere."""
import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import undistort as ud
from tools import rectify_model as rm
from tools import undistort_model as um

pytestmark = pytest.mark.gpu

K_L, K_R = (40.0, 40.0, 31.5, 23.5), (41.0, 39.5, 32.2, 22.9)
KB_L, KB_R = (-0.02, 0.005, -0.001, 0.0002), (0.03, -0.01, 0.002, -0.0003)
RT = (-0.28, 0.07, 0.004, -0.003, 0.01)
K_PITCH = (22.0, 22.0, 31.5, 23.5)


def _rig(f):
    return rm.rectify(dict(cam=[dict(model=rm.KB4, K=K_L, coeffs=KB_L), dict(model=rm.KB4, K=K_R, coeffs=KB_R)],
                           R=rm.rot(*np.deg2rad([1.5, -2.0, 1.0])), t=(-0.11, 0.004, -0.003), f=f))


@pytest.fixture(scope="module")
def rigs():
    return {22: _rig(22.0), 30: _rig(30.0)}


def _image(rows, cols, seed, stride=None):
    """a textured image (never 0, so a border pixel is told from a sampled one) as the [rows, cols] view of a [rows, stride] buffer"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(1, 256, size=(rows, cols if stride is None else stride), dtype=np.uint8)
    return buf[:, :cols]


def _one(ctx, img, model, K, coeffs, iR, dst_stride=None):
    return ud.undistort_lens(ctx, [img], [ud.make_lens_params(model, K, coeffs, iR)], dst_stride=dst_stride)[0]


def test_device_atan_and_sqrt_are_the_models_bits(ctx):
    r = rm.atan_sweep()
    a, s = ud.lens_atan(ctx, r)
    want_a = rm.atan_c(r)
    with np.errstate(invalid="ignore"):
        want_s = np.sqrt(r)
    nan = np.isnan(r)
    assert nan.sum() == 1 and np.array_equal(np.isnan(a), nan) and np.array_equal(np.isnan(s), nan)
    assert np.array_equal(a[~nan].view(np.uint64), want_a[~nan].view(np.uint64))
    assert np.array_equal(s[~nan].view(np.uint64), want_s[~nan].view(np.uint64))


# name: (side, rows, cols, f, src stride, dst stride, the shares (inside, none, partial) the case claims or None)
CASES = {
    "left_f22": (0, 48, 64, 22, None, None, (0.52, 0.41, 0.07)),
    "left_f30": (0, 48, 64, 30, None, None, (0.90, 0.05, 0.05)),
    "right_strided": (1, 45, 67, 22, 80, 72, None),
    "right_byte_stores": (1, 45, 67, 22, 81, 73, None),
    "wide": (0, 12, 300, 22, None, None, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kb4_equals_the_model(ctx, rigs, name):
    side, rows, cols, f, ss, ds, shares = CASES[name]
    K, co = (K_L, KB_L) if side == 0 else (K_R, KB_R)
    iR = rigs[f]["iR_l" if side == 0 else "iR_r"]
    img = _image(rows, cols, 41 + side, ss)
    iu, iv = rm.lens_map(rows, cols, rm.KB4, K, co, iR)
    want = um.remap(img, iu, iv)
    got = _one(ctx, img, rm.KB4, K, co, iR, dst_stride=ds)
    assert np.array_equal(got, want)
    # the case is what it claims
    got_shares = rm.rig_share(rows, cols, iu, iv)
    if shares is not None:
        assert all(abs(g - s) <= 0.05 for g, s in zip(got_shares, shares)), got_shares
    else:
        assert min(got_shares) > 0.03, got_shares                            # every border path is taken
    W = np.arange(cols)[None, :] * iR[6] + np.arange(rows)[:, None] * iR[7] + iR[8]
    assert np.ptp(W) > 0.01                                                  # a rectifying rotation: W != 1
    assert not np.array_equal(want, um.remap(img, *rm.lens_map(rows, cols, rm.RADTAN, K, co + (0.0,), iR)))   # and the lens is told from radtan


def test_rays_behind_the_camera_are_zero(ctx):
    """a 50 degree pitch: the rows with W <= 0, 12.5 % of the pixels, read nothing"""
    iR = um.rotated_iR(K_PITCH, np.deg2rad(50.0), 0.0, 0.0)
    img = _image(48, 64, 43)
    want = rm.rectify_image(img, rm.KB4, K_PITCH, KB_L, iR)
    assert np.array_equal(_one(ctx, img, rm.KB4, K_PITCH, KB_L, iR), want)
    W = (np.arange(64.0)[None, :] * iR[6] + np.arange(48.0)[:, None] * iR[7]) + iR[8]
    behind = ~(W > 0)
    assert abs(behind.mean() - 0.125) <= 0.05 and not want[behind].any() and want[~behind].any()


@pytest.mark.parametrize("coeffs", [(np.nan, 0, 0, 0), (0, np.inf, 0, 0), (1e300, 1e300, 1e300, 1e300), (0, 0, 0, -1e300)])
def test_non_finite_positions_are_ordinary(ctx, rigs, coeffs):
    """q's NaN case and clamp are the code's own: the kernel equals the model and nothing faults"""
    img = _image(48, 64, 44)
    coeffs = tuple(float(c) for c in coeffs)
    iR = rigs[22]["iR_l"]
    assert np.array_equal(_one(ctx, img, rm.KB4, K_L, coeffs, iR), rm.rectify_image(img, rm.KB4, K_L, coeffs, iR))
    bad = um.default_iR(K_L).copy(); bad[8] = 0.0                            # W = 0 everywhere
    want = rm.rectify_image(img, rm.KB4, K_L, KB_L, bad)
    assert np.array_equal(_one(ctx, img, rm.KB4, K_L, KB_L, bad), want) and not want.any()
    bad[8] = np.nan
    assert np.array_equal(_one(ctx, img, rm.KB4, K_L, KB_L, bad), rm.rectify_image(img, rm.KB4, K_L, KB_L, bad))


def test_a_radtan_lens_job_is_ssx_undistort(ctx, rigs):
    img = _image(45, 67, 45, 80)
    iR = rigs[30]["iR_r"]
    via_lens = _one(ctx, img, rm.RADTAN, K_R, RT, iR, dst_stride=72)
    plain = ud.undistort(ctx, [img], [ud.make_params(K_R, RT, iR)], dst_stride=72)[0]
    assert np.array_equal(via_lens, plain) and np.array_equal(plain, um.undistort(img, K_R, RT, iR))
    assert via_lens.any()


@pytest.fixture(scope="module")
def eight(rigs):
    """eight jobs of 45 x 67, the two lens models alternating, with different images and parameters, and the model's results"""
    rng = np.random.default_rng(46)
    jobs = []
    for k in range(8):
        model = rm.KB4 if k % 2 == 0 else rm.RADTAN
        K = tuple(np.array(K_R) + rng.uniform(-2, 2, 4))
        co = tuple(rng.uniform(-0.03, 0.03, 4) * [1, 0.3, 0.1, 0.01]) if model == rm.KB4 else (rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), rng.uniform(-0.004, 0.004),
                                                                                                  rng.uniform(-0.004, 0.004), rng.uniform(-0.02, 0.02))
        iR = rigs[22 if k < 4 else 30]["iR_l" if k % 4 < 2 else "iR_r"]
        img = _image(45, 67, 50 + k)
        jobs.append((img, model, K, co, iR, rm.rectify_image(img, model, K, co, iR)))
    return jobs


def test_mixed_models_in_one_call_equal_the_single_calls_in_one_launch(ctx, eight):
    prm = [ud.make_lens_params(*j[1:5]) for j in eight]
    got = ud.undistort_lens(ctx, [j[0] for j in eight], prm)
    st = ud.last_call(ctx)
    assert st["launches"] == 1 and st["syncs"] == 1, st
    for k, j in enumerate(eight):
        assert np.array_equal(got[k], j[5]), k                                            # the model
        assert np.array_equal(got[k], ud.undistort_lens(ctx, [j[0]], [prm[k]])[0]), k     # the single call
    assert len({p.model for p in prm}) == 2


def test_every_rejection_has_a_message_and_touches_nothing(ctx, eight):
    lib = ud._fns(ctx.lib)
    rows, cols = 45, 67
    src = np.ascontiguousarray(eight[0][0])
    other = np.ascontiguousarray(eight[1][0])
    dst = np.full((rows, cols), 0x5A, np.uint8)
    good_prm = ud.make_lens_params(*eight[0][1:5])

    def call(n, jobs, r=rows, c=cols, null_table=False, models=None):
        arr = (_lib.LensJob * max(len(jobs), 1))()
        for k, (s, ss, d, ds) in enumerate(jobs):
            arr[k].src = s; arr[k].src_stride = ss; arr[k].dst = d; arr[k].dst_stride = ds; arr[k].prm = good_prm
            if models is not None:
                arr[k].prm.model = models[k]
        st = lib.ssx_undistort_lens(ctx.handle, n, None if null_table else arr, r, c, 0)
        return st, lib.ssx_last_error(ctx.handle).decode()

    good = (src.ctypes.data, cols, dst.ctypes.data, cols)
    second = (other.ctypes.data, cols, dst.ctypes.data, cols)
    cases = {
        "n < 0": (call(-1, [good]), "n = -1"),
        "n above the limit": (call(_lib.SSX_UNDISTORT_MAX_JOBS + 1, [good]), "n = 1025"),
        "null table": (call(1, [good], null_table=True), "jobs is null"),
        "null src": (call(1, [(None, cols, dst.ctypes.data, cols)]), "job 0 has a null src"),
        "null dst": (call(1, [(src.ctypes.data, cols, None, cols)]), "job 0 has a null dst"),
        "src stride": (call(1, [(src.ctypes.data, cols - 1, dst.ctypes.data, cols)]), "stride (src 66, dst 67)"),
        "dst stride": (call(1, [(src.ctypes.data, cols, dst.ctypes.data, cols - 1)]), "stride (src 67, dst 66)"),
        "rows": (call(1, [good], r=0), "rows = 0"),
        "cols": (call(1, [good], c=-2), "cols = -2"),
        "in place": (call(1, [(dst.ctypes.data, cols, dst.ctypes.data, cols)]), "dst of job 0 overlaps the src of job 0"),
        "unknown model": (call(1, [good], models=[2]), "job 0 names lens model 2"),
        "negative model": (call(1, [good], models=[-1]), "job 0 names lens model -1"),
        "unknown model of the second job": (call(2, [good, second], models=[1, 7]), "job 1 names lens model 7"),
    }
    for name, ((st, msg), what) in cases.items():
        assert st == _lib.SSX_ERR_INVALID_ARG and msg.startswith("ssx_undistort_lens:") and what in msg, (name, st, msg)
    assert lib.ssx_undistort_lens(ctx.handle, 0, None, 1, 1, 0) == _lib.SSX_OK    # no jobs: nothing to do
    assert (dst == 0x5A).all() and np.array_equal(src, eight[0][0]) and np.array_equal(other, eight[1][0])
    assert ud.last_call(ctx) == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0)
    st, _ = call(1, [good])
    assert st == _lib.SSX_OK and np.array_equal(dst, eight[0][5])
