"""GPU: ssx_stereo_dense_post (csrc/dense_post.inc) -- the launches of ssx_stereo_dense followed by the speckle filter and the samples
-- equals tools/dense_model.py's disparity followed by tools/dense_post_model.py's postprocess, array_equal, on the synthetic pair of
test_dense_gpu.py; with everything off it writes the bytes of ssx_stereo_dense."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import dense as dn
from tools import dense_model as dm
from tools import dense_post_model as pm
from tools.synth import make_stereo_pair

pytestmark = pytest.mark.gpu

ROWS, COLS = 96, 320
CASES = [(200.0, 64, 4), (200.0, 64, 8), (386.0, 128, 8)]
_pairs, _want = {}, {}


def _pair(bf, seed=1, rows=ROWS, cols=COLS, blobs=263):
    k = (bf, seed, rows, cols)
    if k not in _pairs:
        L, R, _ = make_stereo_pair(seed=seed, h=rows, w=cols, n_blobs=blobs, bf=bf)
        L.setflags(write=False); R.setflags(write=False)
        _pairs[k] = (L, R)
    return _pairs[k]


def _model_map(bf, D, paths, **kw):
    k = (bf, D, paths, tuple(sorted(kw.items())))
    if k not in _want:
        L, R = _pair(bf, **kw)
        out = dm.disparity(L, R, dm.DenseParams(disparities=D, paths=paths))
        out.setflags(write=False)
        _want[k] = out
    return _want[k]


@pytest.mark.parametrize("bf,D,paths", CASES)
def test_equals_the_models_chain(ctx, bf, D, paths):
    L, R = _pair(bf)
    raw = _model_map(bf, D, paths)
    bar = pm.min_disp16(bf, 40.0)
    mpost = pm.DensePost(speckle_size=100, speckle_range=16, cloud_stride=4, cloud_min_disp16=bar)
    want_map, want_smp = pm.postprocess(raw, L, mpost)
    assert (want_map != raw).sum() > 50 and 0 < len(want_smp) < (raw[::4, ::4] > 0).sum()           # the filter and the bar both bite
    prm = dn.DenseParams(disparities=D, paths=paths)
    post = dn.DensePost(speckle_size=100, speckle_range=16, cloud_stride=4, cloud_min_disp16=bar)
    got_map, got_smp = dn.dense_disparity(ctx, L, R, prm, post=post)
    st = dn.last_call(ctx)
    assert st["syncs"] == 1 and st["groups"] == 1 and st["launches"] == 12
    assert st["bytes_down"] <= 2 * ROWS * COLS + 8 * 24 * 80 + 3 * 256
    assert np.array_equal(got_map, want_map), int((got_map != want_map).sum())
    assert np.array_equal(dn.samples_table(got_smp), want_smp)
    # the filter alone: a map, no samples
    only = dn.dense_disparity(ctx, L, R, prm, post=dn.DensePost(speckle_size=100, speckle_range=16))
    assert np.array_equal(only, want_map) and dn.last_call(ctx)["launches"] == 10
    # samples alone, and no map asked for: the samples of the unfiltered map, and no map comes down
    spost = dn.DensePost(cloud_stride=4, cloud_min_disp16=bar)
    maps, smp = dn.dense_disparity_batch(ctx, [(L, R)], prm, post=spost, want_maps=False)
    st = dn.last_call(ctx)
    assert maps is None and st["launches"] == 8 and st["bytes_down"] <= 8 * 24 * 80 + 2 * 256
    assert np.array_equal(dn.samples_table(smp[0]), pm.samples(raw, L, 4, bar))


@pytest.mark.parametrize("bf,D,paths", CASES)
def test_everything_off_gives_the_bytes_of_ssx_stereo_dense(ctx, bf, D, paths):
    L, R = _pair(bf)
    prm = dn.DenseParams(disparities=D, paths=paths)
    plain = dn.dense_disparity_batch(ctx, [(L, R)], prm, disp_stride=COLS + 5)[0]
    a = dn.last_call(ctx)
    off = dn.dense_disparity_batch(ctx, [(L, R)], prm, disp_stride=COLS + 5, post=dn.default_post())[0]
    b = dn.last_call(ctx)
    assert plain.base.tobytes() == off.base.tobytes()                          # the pitch elements included
    assert np.array_equal(off, _model_map(bf, D, paths))
    assert a["launches"] == b["launches"] == 6 and a["syncs"] == b["syncs"] == 1


def _three(rows=41, cols=67):
    return [_pair(bf, seed=seed, rows=rows, cols=cols, blobs=30) for seed, bf in ((4, 90.0), (5, 40.0), (6, 200.0))]


def test_three_jobs_equal_three_single_calls_on_host_and_device_memory(ctx):
    import torch
    pairs = _three()
    prm = dn.DenseParams(disparities=64)
    post = dn.DensePost(speckle_size=30, speckle_range=16, cloud_stride=3, cloud_min_disp16=40)
    singles = [dn.dense_disparity(ctx, L, R, prm, post=post) for L, R in pairs]
    for k, (L, R) in enumerate(pairs):                                          # each single call is the model's chain
        m, s = pm.postprocess(dm.disparity(L, R, dm.DenseParams(disparities=64)), L, pm.DensePost(30, 16, 3, 40))
        assert np.array_equal(singles[k][0], m) and np.array_equal(dn.samples_table(singles[k][1]), s), k
    maps, smp = dn.dense_disparity_batch(ctx, pairs, prm, post=post)
    st = dn.last_call(ctx)
    assert st["syncs"] == 1 and st["groups"] == 1 and st["launches"] == 12
    for k in range(3):
        assert np.array_equal(maps[k], singles[k][0]) and smp[k].tobytes() == singles[k][1].tobytes(), k
    assert len({len(s) for s in smp}) > 1                                       # the counts differ: each job has its own
    dev = [(torch.from_numpy(L.copy()).cuda(), torch.from_numpy(R.copy()).cuda()) for L, R in pairs]
    dmaps, dsmp = dn.dense_disparity_batch(ctx, dev, prm, on_device=True, post=post)
    st = dn.last_call(ctx)
    assert st["syncs"] == 1 and st["launches"] == 12 and st["bytes_down"] <= 256
    for k in range(3):
        assert np.array_equal(dmaps[k].cpu().numpy(), singles[k][0]) and dsmp[k].tobytes() == singles[k][1].tobytes(), k
    # device images and no map asked for: the call keeps a map of its own
    _, nsmp = dn.dense_disparity_batch(ctx, dev, prm, on_device=True, post=post, want_maps=False)
    for k in range(3):
        assert nsmp[k].tobytes() == singles[k][1].tobytes(), k


def _raw(ctx, left, right, disp, cloud, prm, post, n=1, rows=40, cols=48, strides=(48, 48, 48), jobs_null=False, prm_null=False, post_null=False, clouds_null=False):
    lib = dn._fns(ctx.lib)
    arr = (_lib.DenseJob * 1)(_lib.DenseJob(left, strides[0], right, strides[1], disp, strides[2]))
    cl = (_lib.DenseCloud * 1)(_lib.DenseCloud(*cloud)) if cloud is not None else None
    return lib.ssx_stereo_dense_post(ctx.handle, n, None if jobs_null else arr, None if clouds_null else cl, rows, cols, None if prm_null else C.byref(prm),
                                     None if post_null else C.byref(post), 0)


def test_every_refusal_is_invalid_arg_with_a_message_and_untouched_memory(ctx):
    rows, cols = 40, 48
    L, R = _pair(60.0, seed=2, rows=rows, cols=cols, blobs=20)
    disp = np.full((rows, cols), 0x5a5a, dtype=np.int16)
    post4 = dn.DensePost(speckle_size=10, cloud_stride=4)
    cap = dn.sample_capacity(rows, cols, post4)
    smp = dn.samples_buffers(1, rows, cols, post4)[0]
    l, r, d, sp = L.ctypes.data, R.ctypes.data, disp.ctypes.data, smp.ctypes.data
    ok = dn.DenseParams(disparities=64)
    bad_prm = dn.DenseParams(disparities=96)
    res_prm = dn.DenseParams(disparities=64)
    res_prm.reserved[1] = 1
    res_post = dn.DensePost(speckle_size=10, cloud_stride=4)
    res_post.reserved[2] = 1
    cases = {
        "disparities 96": dict(prm=bad_prm),
        "reserved of prm": dict(prm=res_prm),
        "null prm": dict(prm_null=True),
        "null post": dict(post_null=True),
        "speckle_size -1": dict(post=dn.DensePost(speckle_size=-1, cloud_stride=4)),
        "speckle_size above the pixels": dict(post=dn.DensePost(speckle_size=rows * cols + 1, cloud_stride=4)),
        "speckle_range 32768": dict(post=dn.DensePost(speckle_range=32768, cloud_stride=4)),
        "cloud_stride 4001": dict(post=dn.DensePost(cloud_stride=4001)),
        "cloud_min_disp16 0": dict(post=dn.DensePost(cloud_stride=4, cloud_min_disp16=0)),
        "cloud_min_disp16 32769": dict(post=dn.DensePost(cloud_stride=4, cloud_min_disp16=32769)),
        "reserved of post": dict(post=res_post),
        "null jobs": dict(jobs_null=True),
        "null left": dict(left=None),
        "null right": dict(right=None),
        "null disp without clouds": dict(disp=None, post=dn.DensePost(speckle_size=10), clouds_null=True),
        "null clouds with a stride": dict(clouds_null=True),
        "clouds without a stride": dict(post=dn.DensePost(speckle_size=10)),
        "null samples": dict(cloud=(None, cap, 0)),
        "a capacity one short": dict(cloud=(sp, cap - 1, 0)),
        "left stride": dict(strides=(47, 48, 48)),
        "right stride": dict(strides=(48, 47, 48)),
        "disp stride": dict(strides=(48, 48, 47)),
        "n -1": dict(n=-1),
        "n above the limit": dict(n=_lib.SSX_DENSE_MAX_JOBS + 1),
        "rows 39": dict(rows=39),
        "cols 4001": dict(cols=4001, strides=(4001, 4001, 4001)),
    }
    for name, kw in cases.items():
        args = dict(left=l, right=r, disp=d, cloud=(sp, cap, 0), prm=ok, post=post4)
        args.update(kw)
        st = _raw(ctx, args.pop("left"), args.pop("right"), args.pop("disp"), args.pop("cloud"), args.pop("prm"), args.pop("post"), **args)
        assert st == _lib.SSX_ERR_INVALID_ARG, name
        msg = ctx.lib.ssx_last_error(ctx.handle).decode()
        assert msg.startswith("ssx_stereo_dense_post:") and len(msg) > 30, (name, msg)
        assert np.all(disp == 0x5a5a) and np.all(smp.view(np.uint8) == 0xA5), name
        assert dn.last_call(ctx) == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0, groups=0), name
    assert dn._fns(ctx.lib).ssx_stereo_dense_post(None, 0, None, None, rows, cols, None, None, 0) == _lib.SSX_ERR_INVALID_ARG
    # a null disp WITH clouds is a valid call, and a valid call right after the refusals gives the model's bytes
    assert _raw(ctx, l, r, None, (sp, cap, 0), ok, post4, strides=(48, 48, 0)) == _lib.SSX_OK
    assert _raw(ctx, l, r, d, (sp, cap, 0), ok, post4) == _lib.SSX_OK
    want_map, _ = pm.postprocess(dm.disparity(L, R, dm.DenseParams(disparities=64)), L, pm.DensePost(10, 16, 4, 1))
    assert np.array_equal(disp, want_map)
    assert _raw(ctx, l, r, d, (sp, cap, 0), ok, post4, n=0) == _lib.SSX_OK
