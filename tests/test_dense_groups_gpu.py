"""GPU: the dense calls beyond their first group, on maps taller than wide, and at the limits of a side and of the job count.

ssx_stereo_dense, ssx_dense_postprocess and ssx_stereo_dense_post (csrc/dense.hip, csrc/dense_post.inc) work through their jobs in
groups whose workspace stays under a cap.  From the second group on a call depends on the table offsets of the group, the per-job
sample counts behind the flag of the result block, the workspace that every group refills (and, chained, the labels that lie on the
dead census words), the scratch maps of jobs without a map of their own, the one copy down over all groups and the launch count.  The
cap is SSX_DENSE_WORKSPACE_CAP (1 GiB); the tests hook ssx_dense_debug_set_workspace_cap lowers it, so that five small jobs make 5, 3
and 2 groups, and one test reaches the second group at the real cap.  Every case asserts the groups ssx_dense_debug_last_call reports.

Everything is integer and held to tools/dense_model.py and tools/dense_post_model.py with array_equal: there is no tolerance here."""
import contextlib

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import dense as dn
from dense_post_cases import made_maps, seam_maps
from test_dense_gpu import _first_differing_stage
from tools import dense_model as dm
from tools import dense_post_model as pm
from tools.synth import make_stereo_pair

pytestmark = pytest.mark.gpu

N = 5
SEEDS = (4, 5, 6, 7, 8)
BF = {4: 90.0, 5: 40.0, 6: 200.0, 7: 120.0, 8: 60.0}             # (4, 5, 6 at 41 x 67 are the pairs of test_dense_gpu.py's trio)
SHAPES = {"41x67_D64": (41, 67, 64), "48x96_D128": (48, 96, 128)}
GROUPS = (1, 2, 4)                                               # jobs a group -> 5, 3 and 2 groups of five jobs, the last of one job
FILTER, STRIDE, BAR = 20, 3, 40                                  # speckle_size, cloud_stride, cloud_min_disp16 of the grouped cases
PITCH = 5                                                        # elements past cols in a map with a pitch of its own
_pairs, _raw, _post = {}, {}, {}


def dense_job_bytes(rows, cols, D):
    """the workspace of one job of ssx_stereo_dense / ssx_stereo_dense_post (include/ssx_test_hooks.h)"""
    return rows * cols * (16 + 2 * D + 4) + 768


def post_job_bytes(rows, cols):
    """the workspace of one job of ssx_dense_postprocess (include/ssx_test_hooks.h)"""
    return rows * cols * 8 + rows * 4 + 768


def cap_for(group, job_bytes):
    """a cap under which exactly `group` jobs fit"""
    return group * job_bytes + job_bytes // 2


def n_groups(n, group):
    return -(-n // group)


@contextlib.contextmanager
def workspace_cap(ctx, nbytes):
    dn.set_workspace_cap(ctx, nbytes)
    try:
        yield
    finally:
        dn.set_workspace_cap(ctx, 0)


def _pair(seed, rows, cols, blobs=None, bf=None):
    k = (seed, rows, cols, blobs, bf)
    if k not in _pairs:
        L, R, _ = make_stereo_pair(seed=seed, h=rows, w=cols, n_blobs=blobs if blobs is not None else rows * cols // 90, bf=bf if bf is not None else BF[seed])
        L.setflags(write=False); R.setflags(write=False)
        _pairs[k] = (L, R)
    return _pairs[k]


def _model(pair_key, D, lr=1):
    """the model's raw map of a pair of _pair, computed once per module"""
    k = (pair_key, D, lr)
    if k not in _raw:
        L, R = _pair(*pair_key)
        out = dm.disparity(L, R, dm.DenseParams(disparities=D, lr_tolerance=lr))
        out.setflags(write=False)
        _raw[k] = out
    return _raw[k]


def _model_post(pair_key, D, speckle=FILTER, stride=STRIDE, bar=BAR):
    """the model's filtered map and sample table of a pair"""
    k = (pair_key, D, speckle, stride, bar)
    if k not in _post:
        L, _ = _pair(*pair_key)
        m = pm.filter_speckles(_model(pair_key, D), speckle, 16)
        s = pm.samples(m, L, stride, bar)
        m.setflags(write=False); s.setflags(write=False)
        _post[k] = (m, s)
    return _post[k]


def _five(shape):
    rows, cols, _ = SHAPES[shape]
    return [(seed, rows, cols, None, None) for seed in SEEDS]


def _on_device(arrays):
    import torch
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _untouched_past(buf, count):
    """nothing is written past a job's count: a host buffer keeps its 0xA5 bytes, a device buffer its 0xA5A5 words"""
    if isinstance(buf, np.ndarray):
        return bool(np.all(buf[count:].view(np.uint8) == 0xA5))
    return bool((buf[count:] == -23131).all().item())


def test_the_cases_are_what_they_claim():
    for rows, cols, D in SHAPES.values():
        for g in GROUPS:
            assert cap_for(g, dense_job_bytes(rows, cols, D)) // dense_job_bytes(rows, cols, D) == g
            assert cap_for(g, post_job_bytes(rows, cols)) // post_job_bytes(rows, cols) == g
    assert [n_groups(N, g) for g in GROUPS] == [5, 3, 2] and all(N % g == 1 or g == 1 for g in GROUPS)
    assert dense_job_bytes(96, 320, 128) == 8479488 and _lib.SSX_DENSE_WORKSPACE_CAP // 8479488 == 126
    assert dense_job_bytes(40, 48, 64) == 284928 and _lib.SSX_DENSE_WORKSPACE_CAP // 284928 >= _lib.SSX_DENSE_MAX_JOBS == 1024


# ---- ssx_stereo_dense ----
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stereo_dense_in_groups(ctx, shape, group):
    rows, cols, D = SHAPES[shape]
    keys = _five(shape)
    pairs = [_pair(*k) for k in keys]
    want = [_model(k, D) for k in keys]
    assert len({w.tobytes() for w in want}) == N                               # five different maps: a job that lands in another's place shows
    groups = n_groups(N, group)
    prm = dn.DenseParams(disparities=D)
    with workspace_cap(ctx, cap_for(group, dense_job_bytes(rows, cols, D))):
        got = dn.dense_disparity_batch(ctx, pairs, prm)
        st = dn.last_call(ctx)
        assert st["groups"] == groups and st["syncs"] == 1 and st["launches"] == 6 * groups, st
        assert st["bytes_down"] == N * 2 * rows * cols
        for k in range(N):
            assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
        # device tensors, a pitch of its own for the map
        dev = list(zip(_on_device([p[0] for p in pairs]), _on_device([p[1] for p in pairs])))
        dgot = dn.dense_disparity_batch(ctx, dev, prm, on_device=True, disp_stride=cols + PITCH)
        st = dn.last_call(ctx)
        assert st["groups"] == groups and st["syncs"] == 1 and st["launches"] == 6 * groups and st["bytes_down"] == 0, st
        for k in range(N):
            host = dgot[k].cpu().numpy()
            assert np.array_equal(host, want[k]), (k, int((host != want[k]).sum()))
            assert bool((dgot[k]._base[:, cols:] == 0x5a5a).all().item()), k    # the pitch elements stay untouched
        # without the left-right check: four launches a group
        off = dn.DenseParams(disparities=D, lr_tolerance=-1)
        got = dn.dense_disparity_batch(ctx, pairs, off)
        st = dn.last_call(ctx)
        assert st["groups"] == groups and st["syncs"] == 1 and st["launches"] == 4 * groups, st
        for k in range(N):
            w = _model(keys[k], D, lr=-1)
            assert np.array_equal(got[k], w), (k, int((got[k] != w).sum()))
    assert not np.array_equal(_model(keys[0], D, lr=-1), want[0])


# ---- ssx_dense_postprocess ----
def _postprocess(ctx, maps, lefts, post, on_device):
    """one ssx_dense_postprocess call on buffers of the test's own -> (the maps' buffers, the counts, the sample buffers)"""
    rows, cols = maps[0].shape
    cap = dn.sample_capacity(rows, cols, post)
    if on_device:
        import torch
        dmaps = []
        for m in maps:
            b = torch.full((rows, cols + PITCH), 0x5a5a, dtype=torch.int16, device="cuda")
            b[:, :cols] = torch.from_numpy(m.copy()).cuda()
            dmaps.append(b)
        dl = _on_device(lefts)
        bufs = dn.samples_buffers(len(maps), rows, cols, post, device=dl[0].device)
        torch.cuda.synchronize()
        jobs = [(l.data_ptr(), l.stride(0), b.data_ptr(), b.stride(0)) for l, b in zip(dl, dmaps)]
        counts = dn.postprocess_ptrs(ctx, jobs, [(b.data_ptr(), cap) for b in bufs], rows, cols, post, on_device=True)
        return [b.cpu().numpy() for b in dmaps], counts, bufs
    hmaps = []
    for m in maps:
        b = np.full((rows, cols + PITCH), 0x5a5a, dtype=np.int16)
        b[:, :cols] = m
        hmaps.append(b)
    bufs = dn.samples_buffers(len(maps), rows, cols, post)
    jobs = [(l.ctypes.data, l.strides[0], b.ctypes.data, cols + PITCH) for l, b in zip(lefts, hmaps)]
    counts = dn.postprocess_ptrs(ctx, jobs, [(b.ctypes.data, cap) for b in bufs], rows, cols, post, on_device=False)
    return hmaps, counts, bufs


@pytest.mark.parametrize("on_device", [False, True], ids=["staged", "device"])
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_postprocess_in_groups(ctx, shape, group, on_device):
    rows, cols, D = SHAPES[shape]
    keys = _five(shape)
    raw = [_model(k, D) for k in keys]
    lefts = [_pair(*k)[0] for k in keys]
    want = [_model_post(k, D) for k in keys]
    assert len({len(s) for _, s in want}) == N                                  # five different counts: count[k] is job k's and no other's
    assert all((m != r).any() for (m, _), r in zip(want, raw))                  # the filter bites in every job
    groups = n_groups(N, group)
    post = dn.DensePost(speckle_size=FILTER, speckle_range=16, cloud_stride=STRIDE, cloud_min_disp16=BAR)
    with workspace_cap(ctx, cap_for(group, post_job_bytes(rows, cols))):
        maps, counts, bufs = _postprocess(ctx, raw, lefts, post, on_device)
        st = dn.last_call(ctx)
    assert st["groups"] == groups and st["syncs"] == 1 and st["launches"] == 6 * groups, st
    assert counts == [len(s) for _, s in want]
    for k in range(N):
        wm, ws = want[k]
        assert np.array_equal(maps[k][:, :cols], wm), (k, int((maps[k][:, :cols] != wm).sum()))
        assert np.all(maps[k][:, cols:] == 0x5a5a), k
        assert np.array_equal(dn.samples_table(dn.samples_result([bufs[k]], [counts[k]])[0]), ws), k
        assert _untouched_past(bufs[k], counts[k]), k


@pytest.mark.parametrize("group", [1, 2])
def test_a_seam_between_two_groups_stays_a_seam(ctx, group):
    """jobs 0 | 1 (and, one job a group, 1 | 2) sit in different groups: their facing rows are equal, valid and not neighbours"""
    shape = (40, 48)
    maps = seam_maps(*shape)
    groups = n_groups(3, group)
    with workspace_cap(ctx, cap_for(group, post_job_bytes(*shape))):
        got = [m.copy() for m in maps]
        dn.postprocess(ctx, got, post=dn.DensePost(speckle_size=shape[1], speckle_range=16))
        st = dn.last_call(ctx)
        assert st["groups"] == groups and st["launches"] == 4 * groups and st["syncs"] == 1, st
        for k in range(3):
            assert np.all(got[k] == pm.INVALID), k                             # a row is a component of cols pixels: all of them go
        keep = [m.copy() for m in maps]
        dn.postprocess(ctx, keep, post=dn.DensePost(speckle_size=shape[1] - 1, speckle_range=16))
        assert dn.last_call(ctx)["groups"] == groups
        for k in range(3):
            assert np.array_equal(keep[k], maps[k]), k                         # ... and none of them one pixel below: no row is joined to another


# ---- ssx_stereo_dense_post ----
def _chain(ctx, pairs, prm, post, on_device, no_map=()):
    """one ssx_stereo_dense_post call on buffers of the test's own; the jobs of no_map pass disp == NULL -> (maps as host arrays with
    their pitch, None for a job without one; counts; sample buffers)"""
    rows, cols = pairs[0][0].shape
    cap = dn.sample_capacity(rows, cols, post)
    n = len(pairs)
    if on_device:
        import torch
        dl, dr = _on_device([p[0] for p in pairs]), _on_device([p[1] for p in pairs])
        dmaps = [None if k in no_map else torch.full((rows, cols + PITCH), 0x5a5a, dtype=torch.int16, device="cuda") for k in range(n)]
        bufs = dn.samples_buffers(n, rows, cols, post, device=dl[0].device)
        torch.cuda.synchronize()
        jobs = [(dl[k].data_ptr(), dl[k].stride(0), dr[k].data_ptr(), dr[k].stride(0), None if dmaps[k] is None else dmaps[k].data_ptr(),
                 0 if dmaps[k] is None else cols + PITCH) for k in range(n)]
        counts = dn.dense_post_ptrs(ctx, jobs, [(b.data_ptr(), cap) for b in bufs], rows, cols, prm, post, images_on_device=True)
        return [None if m is None else m.cpu().numpy() for m in dmaps], counts, bufs
    hmaps = [None if k in no_map else np.full((rows, cols + PITCH), 0x5a5a, dtype=np.int16) for k in range(n)]
    bufs = dn.samples_buffers(n, rows, cols, post)
    jobs = [(pairs[k][0].ctypes.data, pairs[k][0].strides[0], pairs[k][1].ctypes.data, pairs[k][1].strides[0],
             None if hmaps[k] is None else hmaps[k].ctypes.data, 0 if hmaps[k] is None else cols + PITCH) for k in range(n)]
    counts = dn.dense_post_ptrs(ctx, jobs, [(b.ctypes.data, cap) for b in bufs], rows, cols, prm, post, images_on_device=False)
    return hmaps, counts, bufs


def _check_chain(maps, counts, bufs, want, cols, no_map, what):
    for k, (wm, ws) in enumerate(want):
        if k in no_map:
            assert maps[k] is None
        else:
            assert np.array_equal(maps[k][:, :cols], wm), (what, k, int((maps[k][:, :cols] != wm).sum()))
            assert np.all(maps[k][:, cols:] == 0x5a5a), (what, k)
        assert counts[k] == len(ws), (what, k, counts[k], len(ws))
        assert np.array_equal(dn.samples_table(dn.samples_result([bufs[k]], [counts[k]])[0]), ws), (what, k)
        assert _untouched_past(bufs[k], counts[k]), (what, k)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stereo_dense_post_in_groups(ctx, shape, group):
    """the chained call: the labels of a group lie on the census words that the next group's census overwrites"""
    rows, cols, D = SHAPES[shape]
    keys = _five(shape)
    pairs = [_pair(*k) for k in keys]
    want = [_model_post(k, D) for k in keys]
    groups = n_groups(N, group)
    prm = dn.DenseParams(disparities=D)
    post = dn.DensePost(speckle_size=FILTER, speckle_range=16, cloud_stride=STRIDE, cloud_min_disp16=BAR)
    # the two calls, one after the other, on this context: the model's results too
    two = dn.dense_disparity_batch(ctx, pairs, prm)
    two, two_smp = dn.postprocess(ctx, two, [p[0] for p in pairs], post=post)
    for k in range(N):
        assert np.array_equal(two[k], want[k][0]) and np.array_equal(dn.samples_table(two_smp[k]), want[k][1]), k
    all_null = tuple(range(N))
    with workspace_cap(ctx, cap_for(group, dense_job_bytes(rows, cols, D))):
        for on_device in (False, True):
            for no_map in ((), all_null, (1, 3)):
                what = ("device" if on_device else "staged", no_map)
                maps, counts, bufs = _chain(ctx, pairs, prm, post, on_device, no_map)
                st = dn.last_call(ctx)
                assert st["groups"] == groups and st["syncs"] == 1 and st["launches"] == 12 * groups, (what, st)
                _check_chain(maps, counts, bufs, want, cols, no_map, what)
                for k in range(N):
                    if k not in no_map:
                        assert np.array_equal(maps[k][:, :cols], two[k]), (what, k)
                    assert dn.samples_result([bufs[k]], [counts[k]])[0].tobytes() == two_smp[k].tobytes(), (what, k)


def test_the_workspace_is_reused_across_calls_with_other_groups_and_D(ctx):
    """one context: one job a group at D = 128, the default cap at D = 64 (one group), two jobs a group at D = 128 -- the workspace is
    carved anew for every call from one buffer that only grows"""
    shape = "48x96_D128"
    rows, cols, _ = SHAPES[shape]
    keys = _five(shape)
    pairs = [_pair(*k) for k in keys]
    post = dn.DensePost(speckle_size=FILTER, speckle_range=16, cloud_stride=STRIDE, cloud_min_disp16=BAR)
    try:
        for group, D in ((1, 128), (None, 64), (2, 128)):
            dn.set_workspace_cap(ctx, 0 if group is None else cap_for(group, dense_job_bytes(rows, cols, D)))
            groups = 1 if group is None else n_groups(N, group)
            got = dn.dense_disparity_batch(ctx, pairs, dn.DenseParams(disparities=D))
            assert dn.last_call(ctx)["groups"] == groups, (group, D)
            for k in range(N):
                assert np.array_equal(got[k], _model(keys[k], D)), (group, D, k)
            maps, counts, bufs = _chain(ctx, pairs, dn.DenseParams(disparities=D), post, False)
            st = dn.last_call(ctx)
            assert st["groups"] == groups and st["launches"] == 12 * groups, (group, D, st)
            _check_chain(maps, counts, bufs, [_model_post(k, D) for k in keys], cols, (), (group, D))
            maps, counts, bufs = _postprocess(ctx, [_model(k, D) for k in keys], [p[0] for p in pairs], post, False)
            _check_chain(maps, counts, bufs, [_model_post(k, D) for k in keys], cols, (), (group, D, "postprocess"))
    finally:
        dn.set_workspace_cap(ctx, 0)


def test_two_groups_at_the_real_cap(ctx):
    """no hook: 127 pairs of 96 x 320 at D = 128 take 8 479 488 bytes each, 126 of them fit under 2^30 -- a group of 126, then one of 1"""
    import torch
    rows, cols, D, n = 96, 320, 128, 127
    keys = [(1, rows, cols, 263, 386.0), (2, rows, cols, 263, 386.0), (3, rows, cols, 263, 386.0)]     # the first is test_dense_gpu.py's "two_per_lane"
    want = [_model(k, D) for k in keys]
    assert len({w.tobytes() for w in want}) == 3
    dev = [tuple(_on_device(_pair(*k))) for k in keys]
    got = dn.dense_disparity_batch(ctx, [dev[k % 3] for k in range(n)], dn.DenseParams(disparities=D), on_device=True)
    st = dn.last_call(ctx)
    assert st["groups"] == 2 and st["syncs"] == 1 and st["launches"] == 12 and st["bytes_down"] == 0, st
    host = torch.stack(got).cpu().numpy()
    del got
    for k, what in ((125, "job 125, the last of the first group"), (126, "job 126, the one job of the second group and the last of the call")):
        assert np.array_equal(host[k], want[k % 3]), f"{what}: {int((host[k] != want[k % 3]).sum())} pixels differ from the model"
    for k in range(n):
        assert np.array_equal(host[k], want[k % 3]), f"job {k}: {int((host[k] != want[k % 3]).sum())} pixels differ from the model"


# ---- maps taller than wide ----
TALL = {"120x40_D64": (120, 40, 64), "120x40_D128": (120, 40, 128), "67x41_D64": (67, 41, 64)}
_made = {}


def _tall_key(rows, cols):
    return (3, rows, cols, rows * cols // 120, 90.0)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", list(TALL))
def test_tall_pairs_equal_the_model(ctx, name, paths):
    """rows > cols: most diagonals start on a column and the vertical paths are the long ones; at 40 columns x - d < 0 for most lanes of
    every pixel"""
    rows, cols, D = TALL[name]
    assert rows > cols
    L, R = _pair(*_tall_key(rows, cols))
    prm = dn.DenseParams(disparities=D, paths=paths)
    want = dm.disparity(L, R, dm.DenseParams(disparities=D, paths=paths)) if paths != 8 else _model(_tall_key(rows, cols), D)
    if paths == 8:
        assert (want > 0).mean() > 0.8, (want > 0).mean()
    got = dn.dense_disparity(ctx, L, R, prm)
    if not np.array_equal(got, want):
        pytest.fail(f"{name}, {paths} paths: {int((got != want).sum())} of {want.size} pixels differ from the model; first differing stage: "
                    f"{_first_differing_stage(ctx, L, R, prm)}")


@pytest.mark.parametrize("name", ["constant", "checkerboard", "serpentine", "comb", "ramp_at_range", "ramp_past_range", "no_wrap", "blobs", "extremes", "random"])
def test_tall_made_maps_components_and_filter(ctx, name):
    """120 x 40: seven horizontal tile borders (16, 32 .. 112) and no vertical one, so k_dense_label_merge runs with n_v = 0"""
    shape = (120, 40)
    assert shape[0] > shape[1] and (shape[0] - 1) // 16 == 7 and (shape[1] - 1) // 64 == 0
    if shape not in _made:
        _made[shape] = made_maps(*shape)
    m, rng, sizes = _made[shape][name]
    want_size, want_root = pm.components(m, rng)
    size, root = dn.components(ctx, m, rng)
    assert np.array_equal(root, want_root), f"{int((root != want_root).sum())} roots differ"
    assert np.array_equal(size, want_size), f"{int((size != want_size).sum())} sizes differ"
    for s in sizes:
        got = m.copy()
        dn.postprocess(ctx, [got], post=dn.DensePost(speckle_size=s, speckle_range=rng))
        want = np.where((m > 0) & (want_size <= s), pm.INVALID, m).astype(np.int16)
        assert np.array_equal(got, want), (s, int((got != want).sum()))


# ---- the largest sides ----
BIG = {"40x4000": (40, 4000), "4000x40": (4000, 40)}
_big = {}


def _big_case(name):
    """the pair, the model's map, its components and its filtered map, once per module"""
    if name not in _big:
        rows, cols = BIG[name]
        key = _tall_key(rows, cols)
        raw = _model(key, 64)
        size, root = pm.components(raw, 16)
        flt = np.where((raw > 0) & (size <= 50), pm.INVALID, raw).astype(np.int16)
        for a in (size, root, flt):
            a.setflags(write=False)
        _big[name] = (_pair(*key), raw, size, root, flt)
    return _big[name]


@pytest.mark.parametrize("name", list(BIG))
def test_the_largest_side_pair_equals_the_model(ctx, name):
    """paths of 4000 pixels: along the rows of 40 x 4000, down the columns of 4000 x 40"""
    (L, R), want, _, _, _ = _big_case(name)
    assert max(L.shape) == 4000 and min(L.shape) == 40 and (want > 0).mean() > 0.8
    prm = dn.DenseParams(disparities=64)
    got = dn.dense_disparity(ctx, L, R, prm)
    st = dn.last_call(ctx)
    assert st["groups"] == 1 and st["launches"] == 6
    if not np.array_equal(got, want):
        pytest.fail(f"{name}: {int((got != want).sum())} of {want.size} pixels differ from the model; first differing stage: {_first_differing_stage(ctx, L, R, prm)}")


@pytest.mark.parametrize("name", list(BIG))
def test_the_largest_side_components_filter_and_samples(ctx, name):
    (L, _), raw, want_size, want_root, flt = _big_case(name)
    rows, cols = raw.shape
    assert (flt != raw).sum() > 100                                             # the filter bites
    size, root = dn.components(ctx, raw, 16)
    assert np.array_equal(root, want_root), f"{int((root != want_root).sum())} roots differ"
    assert np.array_equal(size, want_size), f"{int((size != want_size).sum())} sizes differ"
    # the filter and every pixel as a sample: rows sample rows (4000 of them on the tall map, v up to 3999; u up to 3999 on the wide one)
    post = dn.DensePost(speckle_size=50, speckle_range=16, cloud_stride=1, cloud_min_disp16=1)
    assert dn.sample_capacity(rows, cols, post) == 160000
    got = raw.copy()
    bufs = dn.samples_buffers(1, rows, cols, post)
    counts = dn.postprocess_ptrs(ctx, [(L.ctypes.data, L.strides[0], got.ctypes.data, cols)], [(bufs[0].ctypes.data, 160000)], rows, cols, post, on_device=False)
    assert dn.last_call(ctx)["launches"] == 6
    assert np.array_equal(got, flt), int((got != flt).sum())
    want = pm.samples(flt, L, 1, 1)
    assert counts == [len(want)] and len(want) == (flt > 0).sum() > 100000
    assert np.array_equal(dn.samples_table(bufs[0][:counts[0]]), want)
    assert want[:, 0].max() >= cols - 2 and want[:, 1].max() == rows - 1         # the last sample row has samples: the scan over rows - 1 terms is used
    assert _untouched_past(bufs[0], counts[0])
    # the largest stride: one sample at (0, 0), or none
    post = dn.DensePost(cloud_stride=4000, cloud_min_disp16=1)
    assert dn.sample_capacity(rows, cols, post) == 1
    for first in (int(flt[0, 0]), 160):
        m = flt.copy()
        m[0, 0] = first
        _, smp = dn.postprocess(ctx, [m], [L], post=post)
        want = pm.samples(m, L, 4000, 1)
        assert len(want) == (1 if first > 0 else 0) and np.array_equal(dn.samples_table(smp[0]), want), first
    assert np.array_equal(want, [[0, 0, 160, int(L[0, 0])]])


# ---- the most jobs ----
def test_the_most_jobs_in_one_call(ctx):
    """n = SSX_DENSE_MAX_JOBS: a 1024-entry job table, a census grid 2048 deep; 284 928 bytes a job, so one group at the default cap"""
    n, rows, cols, D = _lib.SSX_DENSE_MAX_JOBS, 40, 48, 64
    assert n == 1024
    keys = [(seed, rows, cols, 20, bf) for seed, bf in ((2, 60.0), (4, 90.0), (5, 40.0), (6, 200.0))]   # the first is test_dense_gpu.py's smallest pair
    pairs = [_pair(*k) for k in keys]
    want = [_model(k, D) for k in keys]
    assert len({w.tobytes() for w in want}) == 4
    prm = dn.DenseParams(disparities=D)
    got = dn.dense_disparity_batch(ctx, [pairs[k % 4] for k in range(n)], prm)
    st = dn.last_call(ctx)
    assert st["groups"] == 1 and st["syncs"] == 1 and st["launches"] == 6 and st["bytes_down"] == n * 2 * rows * cols, st
    bad = [k for k in range(n) if not np.array_equal(got[k], want[k % 4])]
    assert not bad, f"{len(bad)} jobs differ from the model, the first: {bad[:8]}"
    # the same call chained, with the filter and the samples at stride 4
    post = dn.DensePost(speckle_size=FILTER, speckle_range=16, cloud_stride=4, cloud_min_disp16=1)
    wpost = [_model_post(k, D, stride=4, bar=1) for k in keys]
    assert len({len(s) for _, s in wpost}) == 4
    maps, smp = dn.dense_disparity_batch(ctx, [pairs[k % 4] for k in range(n)], prm, post=post)
    st = dn.last_call(ctx)
    assert st["groups"] == 1 and st["syncs"] == 1 and st["launches"] == 12, st
    assert [len(s) for s in smp] == [len(wpost[k % 4][1]) for k in range(n)]
    bad = [k for k in range(n) if not (np.array_equal(maps[k], wpost[k % 4][0]) and np.array_equal(dn.samples_table(smp[k]), wpost[k % 4][1]))]
    assert not bad, f"{len(bad)} jobs differ from the model, the first: {bad[:8]}"
