"""GPU: ssx_dense_postprocess and the components tap (csrc/dense_post.inc) write the bits of their contract, tools/dense_post_model.py
-- array_equal, no tolerance: every value is an integer and the partition into components does not depend on the order of the unions.

The labelling tile is 64 columns x 16 rows (DP_TW x DP_TH).  Shapes: the smallest legal map (40 x 48: less than one tile wide), an odd
one (41 x 67: one column past a tile), the synthetic pair's (96 x 320) and 50 x 150, which crosses a tile border three times down
(16, 32, 48) and twice across (64, 128).  The made maps are tests/dense_post_cases.py's."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import dense as dn
from dense_post_cases import made_maps, seam_maps
from tools import dense_post_model as pm

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16
SHAPES = [(40, 48), (41, 67), (96, 320), (50, 150)]
CASES = ["constant", "checkerboard", "serpentine", "comb", "ramp_at_range", "ramp_past_range", "no_wrap", "blobs", "extremes", "random"]
_maps, _comp, _left = {}, {}, {}


def _made(shape):
    if shape not in _maps:
        _maps[shape] = made_maps(*shape)
    return _maps[shape]


def _components(shape, name):
    """the model's (size, root), computed once per map"""
    if (shape, name) not in _comp:
        m, rng, _ = _made(shape)[name]
        size, root = pm.components(m, rng)
        size.setflags(write=False); root.setflags(write=False)
        _comp[(shape, name)] = (size, root)
    return _comp[(shape, name)]


def _filtered(shape, name, s):
    m, _, _ = _made(shape)[name]
    size, _ = _components(shape, name)
    return np.where((m > 0) & (size <= s), pm.INVALID, m).astype(np.int16) if s > 0 else m.copy()


def _image(shape):
    if shape not in _left:
        im = np.random.default_rng(shape[0] + shape[1]).integers(0, 256, size=shape).astype(np.uint8)
        im.setflags(write=False)
        _left[shape] = im
    return _left[shape]


def test_the_shapes_cross_the_tile():
    assert (50 - 1) // TILE_H >= 2 and (150 - 1) // TILE_W >= 2 and 48 < TILE_W and 67 == TILE_W + 3


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_components_and_filter_equal_the_model(ctx, shape, name):
    m, rng, sizes = _made(shape)[name]
    want_size, want_root = _components(shape, name)
    size, root = dn.components(ctx, m, rng)
    assert np.array_equal(root, want_root), f"{int((root != want_root).sum())} roots differ"
    assert np.array_equal(size, want_size), f"{int((size != want_size).sum())} sizes differ"
    for s in sizes:
        got = m.copy()
        dn.postprocess(ctx, [got], post=dn.DensePost(speckle_size=s, speckle_range=rng))
        assert np.array_equal(got, _filtered(shape, name, s)), (s, int((got != _filtered(shape, name, s)).sum()))
    if name == "constant":
        assert np.array_equal(_filtered(shape, name, sizes[0]), m) and np.all(_filtered(shape, name, sizes[1]) == pm.INVALID)


def test_speckle_size_0_changes_nothing_and_launches_nothing(ctx):
    m = _made((41, 67))["random"][0]
    got = m.copy()
    dn.postprocess(ctx, [got], post=dn.DensePost())
    assert np.array_equal(got, m)
    assert dn.last_call(ctx)["launches"] == 0 and dn.last_call(ctx)["syncs"] == 1


def test_three_jobs_have_no_seam(ctx):
    shape = (40, 48)
    maps = seam_maps(*shape)
    want = [pm.filter_speckles(m, shape[1], 16) for m in maps]                 # a row is a component of cols pixels: all of them go
    assert all(np.all(w == pm.INVALID) for w in want)
    got = [m.copy() for m in maps]
    dn.postprocess(ctx, got, post=dn.DensePost(speckle_size=shape[1], speckle_range=16))
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k
    keep = [m.copy() for m in maps]
    dn.postprocess(ctx, keep, post=dn.DensePost(speckle_size=shape[1] - 1, speckle_range=16))
    for k in range(3):
        assert np.array_equal(keep[k], maps[k]), k
    # and three different maps in one call are three single calls
    trio = [_made(shape)[n][0] for n in ("random", "comb", "blobs")]
    got = [m.copy() for m in trio]
    dn.postprocess(ctx, got, post=dn.DensePost(speckle_size=50, speckle_range=16))
    st = dn.last_call(ctx)
    assert st["syncs"] == 1 and st["groups"] == 1 and st["launches"] == 4
    for k, n in enumerate(("random", "comb", "blobs")):
        assert np.array_equal(got[k], _filtered(shape, n, 50)), n


def test_a_pitch_of_its_own(ctx):
    shape, name, s = (41, 67), "random", 20
    m, rng, _ = _made(shape)[name]
    buf = np.full((shape[0], 75), 0x5a5a, dtype=np.int16)
    buf[:, :67] = m
    view = buf[:, :67]
    limg = np.full((shape[0], 80), 0xAB, dtype=np.uint8)
    limg[:, :67] = _image(shape)
    post = dn.DensePost(speckle_size=s, speckle_range=rng, cloud_stride=3, cloud_min_disp16=105)
    _, smp = dn.postprocess(ctx, [view], [limg[:, :67]], post=post)
    assert np.all(buf[:, 67:] == 0x5a5a)                                        # the pitch elements stay untouched
    assert np.array_equal(view, _filtered(shape, name, s))
    assert np.array_equal(dn.samples_table(smp[0]), pm.samples(_filtered(shape, name, s), _image(shape), 3, 105))


@pytest.mark.parametrize("stride", [1, 3, 4, 7])
def test_samples_in_raster_order(ctx, stride):
    shape, name = (50, 150), "random"
    m, rng, _ = _made(shape)[name]
    left = _image(shape)
    for s, bar in ((0, 1), (20, 105), (0, 32768), (20, 111)):                   # both extremes of the bar: everything valid, nothing at all
        post = dn.DensePost(speckle_size=s, speckle_range=rng, cloud_stride=stride, cloud_min_disp16=bar)
        got = m.copy()
        bufs = dn.samples_buffers(1, *shape, post)
        cap = dn.sample_capacity(*shape, post)
        counts = dn.postprocess_ptrs(ctx, [(left.ctypes.data, left.strides[0], got.ctypes.data, shape[1])], [(bufs[0].ctypes.data, cap)], *shape, post, on_device=False)
        want = pm.samples(_filtered(shape, name, s), left, stride, bar)
        assert counts == [len(want)], (s, bar)
        assert np.array_equal(dn.samples_table(bufs[0][:counts[0]]), want), (s, bar)
        assert np.all(bufs[0]["reserved"][:counts[0]] == 0)
        assert np.all(bufs[0][counts[0]:].view(np.uint8) == 0xA5)               # nothing is written past the count
        order = want[:, 1] * shape[1] + want[:, 0]
        assert np.all(np.diff(order) > 0)
        if bar == 1:
            assert len(want) == (m[::stride, ::stride] > 0).sum() > 0
        if bar == 32768:
            assert len(want) == 0
        assert dn.last_call(ctx)["launches"] == (6 if s else 2) and dn.last_call(ctx)["syncs"] == 1


def _raw(ctx, disp, left, cloud, post, n=1, rows=40, cols=48, strides=(48, 48), jobs_null=False, post_null=False, clouds_null=False, on_device=0):
    lib = dn._fns(ctx.lib)
    arr = (_lib.DenseJob * 1)(_lib.DenseJob(left, strides[0], None, 0, disp, strides[1]))
    cl = (_lib.DenseCloud * 1)(_lib.DenseCloud(*cloud)) if cloud is not None else None
    return lib.ssx_dense_postprocess(ctx.handle, n, None if jobs_null else arr, None if clouds_null else cl, rows, cols, None if post_null else C.byref(post), on_device)


def test_every_refusal_is_invalid_arg_with_a_message_and_untouched_memory(ctx):
    rows, cols = 40, 48
    m = _made((rows, cols))["random"][0]
    disp = m.copy()
    left = _image((rows, cols))
    post4 = dn.DensePost(speckle_size=10, cloud_stride=4)
    cap = dn.sample_capacity(rows, cols, post4)
    assert cap == 10 * 12
    smp = dn.samples_buffers(1, rows, cols, post4)[0]
    d, l, sp = disp.ctypes.data, left.ctypes.data, smp.ctypes.data

    def post(**kw):
        r = kw.pop("reserved", None)
        p = dn.DensePost(**{**dict(speckle_size=10, cloud_stride=4), **kw})
        if r is not None:
            p.reserved[r] = 1
        return p

    cases = {
        "speckle_size -1": dict(post=post(speckle_size=-1)),
        "speckle_size above the pixels": dict(post=post(speckle_size=rows * cols + 1)),
        "speckle_range -1": dict(post=post(speckle_range=-1)),
        "speckle_range 32768": dict(post=post(speckle_range=32768)),
        "cloud_stride -1": dict(post=post(cloud_stride=-1)),
        "cloud_stride 4001": dict(post=post(cloud_stride=4001)),
        "cloud_min_disp16 0": dict(post=post(cloud_min_disp16=0)),
        "cloud_min_disp16 32769": dict(post=post(cloud_min_disp16=32769)),
        "reserved 0": dict(post=post(reserved=0)),
        "reserved 3": dict(post=post(reserved=3)),
        "null post": dict(post_null=True),
        "null jobs": dict(jobs_null=True),
        "null disp": dict(disp=None),
        "null left with samples": dict(left=None),
        "null clouds with a stride": dict(clouds_null=True),
        "clouds without a stride": dict(post=post(cloud_stride=0)),
        "null samples": dict(cloud=(None, cap, 0)),
        "a capacity one short": dict(cloud=(sp, cap - 1, 0)),
        "samples not aligned on the device": dict(cloud=(sp + 2, cap, 0), on_device=1),
        "disp stride": dict(strides=(48, 47)),
        "left stride": dict(strides=(47, 48)),
        "n -1": dict(n=-1),
        "n above the limit": dict(n=_lib.SSX_DENSE_MAX_JOBS + 1),
        "rows 39": dict(rows=39),
        "cols 4001": dict(cols=4001, strides=(4001, 4001)),
    }
    for name, kw in cases.items():
        args = dict(disp=d, left=l, cloud=(sp, cap, 0), post=post4)
        args.update(kw)
        st = _raw(ctx, args.pop("disp"), args.pop("left"), args.pop("cloud"), args.pop("post"), **args)
        assert st == _lib.SSX_ERR_INVALID_ARG, name
        msg = ctx.lib.ssx_last_error(ctx.handle).decode()
        assert msg.startswith("ssx_dense_postprocess:") and len(msg) > 30, (name, msg)
        assert np.array_equal(disp, m) and np.all(smp.view(np.uint8) == 0xA5), name
        assert dn.last_call(ctx) == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0, groups=0), name
    assert dn._fns(ctx.lib).ssx_dense_postprocess(None, 0, None, None, rows, cols, None, 0) == _lib.SSX_ERR_INVALID_ARG
    # a valid call right after: the model's bytes; a left image is not needed without samples; no map at all is no error
    dn.postprocess(ctx, [disp], post=dn.DensePost(speckle_size=10))
    assert np.array_equal(disp, _filtered((rows, cols), "random", 10))
    assert _raw(ctx, d, l, (sp, cap, 0), post4, n=0) == _lib.SSX_OK


def test_launches_do_not_depend_on_the_content_and_runs_repeat(ctx):
    shape = (50, 150)
    post = dn.DensePost(speckle_size=20, speckle_range=16, cloud_stride=4, cloud_min_disp16=105)
    stats, outs = {}, {}
    for name in ("constant", "random"):
        for run in range(2):
            got = _made(shape)[name][0].copy()
            _, smp = dn.postprocess(ctx, [got], [_image(shape)], post=post)
            stats[(name, run)] = dn.last_call(ctx)
            outs[(name, run)] = (got.tobytes(), smp[0].tobytes())
        assert outs[(name, 0)] == outs[(name, 1)], name
    assert stats[("constant", 0)] == stats[("random", 0)] == stats[("random", 1)]
    assert stats[("random", 0)]["launches"] == 6 and stats[("random", 0)]["syncs"] == 1 and stats[("random", 0)]["groups"] == 1


def test_device_tensors(ctx):
    import torch
    shape, name, s = (41, 67), "random", 20
    m, rng, _ = _made(shape)[name]
    post = dn.DensePost(speckle_size=s, speckle_range=rng, cloud_stride=3, cloud_min_disp16=105)
    buf = torch.full((shape[0], 75), 0x5a5a, dtype=torch.int16, device="cuda")
    buf[:, :67] = torch.from_numpy(m.copy()).cuda()
    left = torch.from_numpy(_image(shape).copy()).cuda()
    maps, smp = dn.postprocess(ctx, [buf[:, :67]], [left], post=post, on_device=True)
    st = dn.last_call(ctx)
    assert st["syncs"] == 1 and st["launches"] == 6 and st["bytes_down"] <= 256
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :67], _filtered(shape, name, s)) and np.all(host[:, 67:] == 0x5a5a)
    assert np.array_equal(dn.samples_table(smp[0]), pm.samples(_filtered(shape, name, s), _image(shape), 3, 105))


def test_pinned_host_memory(ctx):
    lib = ctx.lib
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    shape, name, s = (41, 67), "random", 20
    rows, cols = shape
    m, rng, _ = _made(shape)[name]
    post = dn.DensePost(speckle_size=s, speckle_range=rng, cloud_stride=3, cloud_min_disp16=105)
    cap = dn.sample_capacity(rows, cols, post)
    ds, ls = 70, 72
    o_left, o_smp = 2 * rows * ds, 2 * rows * ds + rows * ls
    o_smp = (o_smp + 7) // 8 * 8
    total = o_smp + 8 * cap
    p = lib.ssx_host_alloc(total)
    assert p
    try:
        arena = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(total,))
        arena[:] = 0xAB
        dmap = arena[:o_left].view(np.int16).reshape(rows, ds)
        dmap[:, :cols] = m
        arena[o_left:o_left + rows * ls].reshape(rows, ls)[:, :cols] = _image(shape)
        counts = dn.postprocess_ptrs(ctx, [(p + o_left, ls, p, ds)], [(p + o_smp, cap)], rows, cols, post, on_device=True)
        want = pm.samples(_filtered(shape, name, s), _image(shape), 3, 105)
        assert counts == [len(want)]
        assert np.array_equal(dmap[:, :cols], _filtered(shape, name, s)) and np.all(dmap[:, cols:].view(np.uint8) == 0xAB)
        got = arena[o_smp:o_smp + 8 * counts[0]].view(dn.SAMPLE_DTYPE)
        assert np.array_equal(dn.samples_table(got), want)
        assert np.all(arena[o_smp + 8 * counts[0]:] == 0xAB)
    finally:
        lib.ssx_host_free(p)
