"""Dense stereo over ctypes: ssx_stereo_dense / ssx_dense_default_params (include/ssx.h; contract: tools/dense_model.py) -- a disparity
for every pixel of a rectified pair by census + semi-global matching, int16 in 1/16 pixel, -16 where a pixel is invalid -- and what
follows a map: ssx_dense_postprocess / ssx_stereo_dense_post (contract: tools/dense_post_model.py), the speckle filter and the samples
a keyframe keeps."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, DenseCloud, DenseJob, DenseParamsC, DensePostC, load

INVALID = -16


class DenseParams(DenseParamsC):
    """ssx_dense_params with ssx_dense_default_params' values: disparities 64 or 128, 1 <= p1 <= p2 <= 192, uniqueness 0..99 (percent),
    lr_tolerance in whole disparities (-1: off), paths 4 or 8"""

    def __init__(self, disparities=128, p1=7, p2=86, uniqueness=10, lr_tolerance=1, paths=8):
        super().__init__(int(disparities), int(p1), int(p2), int(uniqueness), int(lr_tolerance), int(paths))


def _fns(lib):
    if not getattr(lib, "_dense_ready", False):
        lib.ssx_dense_default_params.restype = None
        lib.ssx_dense_default_params.argtypes = [C.POINTER(DenseParamsC)]
        lib.ssx_stereo_dense.restype = C.c_int
        lib.ssx_stereo_dense.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DenseJob), C.c_int32, C.c_int32, C.POINTER(DenseParamsC), C.c_int32]
        lib.ssx_dense_default_post.restype = None
        lib.ssx_dense_default_post.argtypes = [C.POINTER(DensePostC)]
        lib.ssx_dense_min_disp16.restype = C.c_int32
        lib.ssx_dense_min_disp16.argtypes = [C.c_double, C.c_double]
        lib.ssx_dense_postprocess.restype = C.c_int
        lib.ssx_dense_postprocess.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DenseJob), C.POINTER(DenseCloud), C.c_int32, C.c_int32, C.POINTER(DensePostC), C.c_int32]
        lib.ssx_stereo_dense_post.restype = C.c_int
        lib.ssx_stereo_dense_post.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DenseJob), C.POINTER(DenseCloud), C.c_int32, C.c_int32, C.POINTER(DenseParamsC),
                                              C.POINTER(DensePostC), C.c_int32]
        if hasattr(lib, "ssx_dense_debug_components"):
            lib.ssx_dense_debug_components.restype = C.c_int
            lib.ssx_dense_debug_components.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        if hasattr(lib, "ssx_dense_debug_last_call"):           # include/ssx_test_hooks.h: absent from a product build
            i32_p, i64_p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
            lib.ssx_dense_debug_last_call.restype = C.c_int
            lib.ssx_dense_debug_last_call.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p, i32_p]
            lib.ssx_dense_debug_stages.restype = C.c_int
            lib.ssx_dense_debug_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DenseParamsC),
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.ssx_dense_debug_set_workspace_cap.restype = C.c_int
            lib.ssx_dense_debug_set_workspace_cap.argtypes = [C.c_void_p, C.c_uint64]
        lib._dense_ready = True
    return lib


def default_params() -> DenseParams:
    """ssx_dense_default_params.  Needs no device."""
    lib = _fns(load())
    p = DenseParams()
    lib.ssx_dense_default_params(C.byref(p))
    return p


def dense_ptrs(ctx: Context, jobs, rows, cols, params=None, images_on_device=True):
    """ssx_stereo_dense on memory the caller holds: jobs = [(left address, left stride in bytes, right address, right stride in bytes,
    disp address, disp stride in int16 elements)]"""
    lib = _fns(ctx.lib)
    n = len(jobs)
    arr = (DenseJob * max(n, 1))()
    for k, (l, ls, r, rs, d, ds) in enumerate(jobs):
        arr[k].left = l; arr[k].left_stride = ls; arr[k].right = r; arr[k].right_stride = rs; arr[k].disp = d; arr[k].disp_stride = ds
    prm = params if params is not None else DenseParams()
    ctx.check(lib.ssx_stereo_dense(ctx.handle, n, arr, rows, cols, C.byref(prm), 1 if images_on_device else 0))


def _host_image(im, shape=None):
    if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 2 or im.strides[1] != 1 or im.strides[0] < im.shape[1] or \
            (shape is not None and im.shape != shape):
        raise ValueError("images: 2-D uint8 arrays of one shape with contiguous rows")
    return im


def dense_disparity_batch(ctx: Context, pairs, params=None, on_device=False, disp_stride=None, post=None, want_maps=True):
    """One ssx_stereo_dense call over pairs = [(left, right)].
    on_device=False: 2-D uint8 numpy arrays of one shape (a row pitch is kept) -> int16 arrays [rows, cols] (with disp_stride, in
    elements: each the [rows, cols] view of a [rows, disp_stride] buffer filled with 0x5a5a).
    on_device=True: 2-D uint8 torch tensors on the context's device (a row pitch is kept) -> int16 torch tensors on that device, read
    and written where they lie.
    post (a DensePost): one ssx_stereo_dense_post call instead -- the maps are filtered; with post.cloud_stride > 0 the result is
    (maps, samples), samples as samples_buffers() / samples_result() make them, and want_maps=False leaves the maps on the device
    (maps is then None)."""
    if not pairs:
        return [] if post is None or post.cloud_stride == 0 else ([], [])
    rows, cols = pairs[0][0].shape
    outs, jobs, keep = [], [], []
    if on_device:
        import torch
        for l, r in pairs:
            for t in (l, r):
                if t.dtype != torch.uint8 or t.dim() != 2 or tuple(t.shape) != (rows, cols) or t.stride(1) != 1 or not t.is_cuda:
                    raise ValueError("images: 2-D uint8 device tensors of one shape with contiguous rows")
            d = torch.full((rows, cols if disp_stride is None else int(disp_stride)), 0x5a5a, dtype=torch.int16, device=l.device)
            outs.append(d)
            jobs.append((l.data_ptr(), l.stride(0), r.data_ptr(), r.stride(0), d.data_ptr(), d.stride(0)))
        torch.cuda.synchronize(pairs[0][0].device)              # the tensors were made on torch's stream, the call runs on the context's
    else:
        for l, r in pairs:
            _host_image(l, (rows, cols)); _host_image(r, (rows, cols))
            d = np.full((rows, cols if disp_stride is None else int(disp_stride)), 0x5a5a, dtype=np.int16)
            outs.append(d)
            jobs.append((l.ctypes.data, l.strides[0], r.ctypes.data, r.strides[0], d.ctypes.data, d.strides[0] // 2))
    if post is None:
        dense_ptrs(ctx, jobs, rows, cols, params, images_on_device=on_device)
        return [d[:, :cols] for d in outs]
    sampling = post.cloud_stride > 0
    if not want_maps:
        if not sampling:
            raise ValueError("want_maps=False asks for samples: post.cloud_stride > 0")
        jobs = [(l, ls, r, rs, None, 0) for l, ls, r, rs, _, _ in jobs]
    bufs = samples_buffers(len(jobs), rows, cols, post, device=pairs[0][0].device if on_device else None) if sampling else None
    counts = dense_post_ptrs(ctx, jobs, [(_address(b), sample_capacity(rows, cols, post)) for b in bufs] if sampling else None, rows, cols, params, post,
                             images_on_device=on_device)
    maps = [d[:, :cols] for d in outs] if want_maps else None
    return (maps, samples_result(bufs, counts)) if sampling else maps


def dense_disparity(ctx: Context, left, right, params=None, post=None):
    """The disparity map of one rectified pair of host images -> int16 [rows, cols] in 1/16 pixel, INVALID (-16) where a check fails.
    post (a DensePost): the filtered map, or (map, samples) when post.cloud_stride > 0"""
    out = dense_disparity_batch(ctx, [(left, right)], params, post=post)
    if post is not None and post.cloud_stride > 0:
        return out[0][0], out[1][0]
    return out[0]


# ---- what follows a map: the speckle filter and the samples (contract: tools/dense_post_model.py) ----
SAMPLE_DTYPE = np.dtype([("u", "<u2"), ("v", "<u2"), ("disp16", "<i2"), ("intensity", "u1"), ("reserved", "u1")])   # ssx_dense_sample


class DensePost(DensePostC):
    """ssx_dense_post with ssx_dense_default_post's values (everything off): speckle_size 0 .. rows * cols (0: no filter), speckle_range
    in 1/16 pixel, cloud_stride 0 (no samples) or 1 .. 4000, cloud_min_disp16 1 .. 32768 (min_disp16())"""

    def __init__(self, speckle_size=0, speckle_range=16, cloud_stride=0, cloud_min_disp16=1):
        super().__init__(int(speckle_size), int(speckle_range), int(cloud_stride), int(cloud_min_disp16))


def default_post() -> DensePost:
    """ssx_dense_default_post.  Needs no device."""
    lib = _fns(load())
    p = DensePost()
    lib.ssx_dense_default_post(C.byref(p))
    return p


def min_disp16(bf, max_depth) -> int:
    """ssx_dense_min_disp16: the depth bar bf * 16 / disp16 <= max_depth as the smallest disp16 that passes.  Needs no device."""
    return int(_fns(load()).ssx_dense_min_disp16(float(bf), float(max_depth)))


def sample_capacity(rows, cols, post) -> int:
    s = post.cloud_stride
    return -(-rows // s) * -(-cols // s) if s > 0 else 0


def samples_buffers(n, rows, cols, post, device=None):
    """n buffers of sample_capacity records: numpy arrays of SAMPLE_DTYPE filled with 0xa5 bytes, or (device given) int16 torch tensors
    [capacity, 4] on it"""
    cap = max(sample_capacity(rows, cols, post), 1)
    if device is None:
        return [np.full(cap * 8, 0xA5, dtype=np.uint8).view(SAMPLE_DTYPE) for _ in range(n)]
    import torch
    return [torch.full((cap, 4), -23131, dtype=torch.int16, device=device) for _ in range(n)]


def samples_result(bufs, counts):
    """the first count records of every buffer, as arrays of SAMPLE_DTYPE (device tensors are copied to the host)"""
    out = []
    for b, c in zip(bufs, counts):
        if not isinstance(b, np.ndarray):
            b = b.cpu().numpy().view(np.uint8).reshape(-1).view(SAMPLE_DTYPE)
        out.append(b[:c])
    return out


def samples_table(s):
    """samples of SAMPLE_DTYPE -> int64 [n, 4] = u, v, disp16, intensity, as tools/dense_post_model.py's samples()"""
    return np.stack([s["u"], s["v"], s["disp16"], s["intensity"]], axis=1).astype(np.int64).reshape(-1, 4)


def _address(b):
    return b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()


def _post_call(ctx, fn_name, jobs, clouds, rows, cols, extra, post, on_device):
    lib = _fns(ctx.lib)
    n = len(jobs)
    arr = (DenseJob * max(n, 1))()
    for k, (l, ls, r, rs, d, ds) in enumerate(jobs):
        arr[k].left = l; arr[k].left_stride = ls; arr[k].right = r; arr[k].right_stride = rs; arr[k].disp = d; arr[k].disp_stride = ds
    cl = None
    if clouds is not None:
        cl = (DenseCloud * max(n, 1))()
        for k, (p, cap) in enumerate(clouds):
            cl[k].samples = p; cl[k].capacity = cap; cl[k].count = -1
    ctx.check(getattr(lib, fn_name)(ctx.handle, n, arr, cl, rows, cols, *extra, C.byref(post), 1 if on_device else 0))
    return [cl[k].count for k in range(n)] if clouds is not None else None


def dense_post_ptrs(ctx: Context, jobs, clouds, rows, cols, params=None, post=None, images_on_device=True):
    """ssx_stereo_dense_post on memory the caller holds: jobs as dense_ptrs takes them (a disp address may be None with clouds), clouds =
    [(samples address, capacity in records)] or None -> the counts, or None"""
    prm = params if params is not None else DenseParams()
    return _post_call(ctx, "ssx_stereo_dense_post", jobs, clouds, rows, cols, (C.byref(prm),), post if post is not None else DensePost(), images_on_device)


def postprocess_ptrs(ctx: Context, jobs, clouds, rows, cols, post, on_device=True):
    """ssx_dense_postprocess on memory the caller holds: jobs = [(left address or None, left stride in bytes, disp address, disp stride in
    int16 elements)], clouds as dense_post_ptrs takes them -> the counts, or None"""
    return _post_call(ctx, "ssx_dense_postprocess", [(l, ls, None, 0, d, ds) for l, ls, d, ds in jobs], clouds, rows, cols, (), post, on_device)


def postprocess(ctx: Context, maps, lefts=None, post=None, on_device=False):
    """One ssx_dense_postprocess call over maps of one shape, which are filtered IN PLACE: 2-D int16 numpy arrays with contiguous rows (a
    row pitch is kept), or with on_device int16 torch tensors on the context's device.  lefts (the left images, uint8, the same kind of
    memory) are needed with post.cloud_stride > 0 -> maps, or (maps, samples) then."""
    post = post if post is not None else DensePost()
    sampling = post.cloud_stride > 0
    if not maps:
        return ([], []) if sampling else []
    rows, cols = maps[0].shape
    if sampling and (lefts is None or len(lefts) != len(maps)):
        raise ValueError("post.cloud_stride > 0 needs the left image of every map")
    jobs = []
    for k, m in enumerate(maps):
        l = lefts[k] if sampling else None
        if on_device:
            import torch
            if m.dtype != torch.int16 or m.dim() != 2 or tuple(m.shape) != (rows, cols) or m.stride(1) != 1 or not m.is_cuda:
                raise ValueError("maps: 2-D int16 device tensors of one shape with contiguous rows")
            if l is not None and (l.dtype != torch.uint8 or tuple(l.shape) != (rows, cols) or l.stride(1) != 1 or not l.is_cuda):
                raise ValueError("lefts: 2-D uint8 device tensors of the maps' shape with contiguous rows")
            jobs.append((l.data_ptr() if l is not None else None, l.stride(0) if l is not None else 0, m.data_ptr(), m.stride(0)))
        else:
            if not isinstance(m, np.ndarray) or m.dtype != np.int16 or m.shape != (rows, cols) or m.strides[1] != 2 or m.strides[0] % 2 or m.strides[0] < 2 * cols:
                raise ValueError("maps: 2-D int16 arrays of one shape with contiguous rows")
            if l is not None:
                _host_image(l, (rows, cols))
            jobs.append((l.ctypes.data if l is not None else None, l.strides[0] if l is not None else 0, m.ctypes.data, m.strides[0] // 2))
    if on_device:
        import torch
        torch.cuda.synchronize(maps[0].device)
    bufs = samples_buffers(len(maps), rows, cols, post, device=maps[0].device if on_device else None) if sampling else None
    counts = postprocess_ptrs(ctx, jobs, [(_address(b), sample_capacity(rows, cols, post)) for b in bufs] if sampling else None, rows, cols, post, on_device)
    return (maps, samples_result(bufs, counts)) if sampling else maps


def components(ctx: Context, disp, speckle_range):
    """ssx_dense_debug_components -> (size, root), int32 [rows, cols], as tools/dense_post_model.py's components()"""
    lib = _fns(ctx.lib)
    if not isinstance(disp, np.ndarray) or disp.dtype != np.int16 or disp.ndim != 2 or disp.strides[1] != 2 or disp.strides[0] % 2:
        raise ValueError("disp: a 2-D int16 array with contiguous rows")
    rows, cols = disp.shape
    size, root = np.zeros((rows, cols), dtype=np.int32), np.zeros((rows, cols), dtype=np.int32)
    ctx.check(lib.ssx_dense_debug_components(ctx.handle, disp.ctypes.data, disp.strides[0] // 2, rows, cols, int(speckle_range), size.ctypes.data, root.ctypes.data))
    return size, root


def last_call(ctx: Context):
    """ssx_dense_debug_last_call -> dict(launches, syncs, bytes_up, bytes_down, groups) of the context's last ssx_stereo_dense"""
    lib = _fns(ctx.lib)
    a, b, c, d, e = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    ctx.check(lib.ssx_dense_debug_last_call(ctx.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
    return dict(launches=a.value, syncs=b.value, bytes_up=c.value, bytes_down=d.value, groups=e.value)


def set_workspace_cap(ctx: Context, nbytes):
    """ssx_dense_debug_set_workspace_cap: the cap, in bytes, that the context's dense calls group their jobs by from now on; 0 = the
    default, SSX_DENSE_WORKSPACE_CAP.  A test that sets one restores 0 in a finally."""
    ctx.check(_fns(ctx.lib).ssx_dense_debug_set_workspace_cap(ctx.handle, int(nbytes)))


def stages(ctx: Context, left, right, params=None, direction=0):
    """ssx_dense_debug_stages -> dict(census_left, census_right, path_volume (of `direction`), sum_volume, right_disparity) as
    tools/dense_model.py names and shapes them"""
    lib = _fns(ctx.lib)
    prm = params if params is not None else DenseParams()
    _host_image(left); _host_image(right, left.shape)
    rows, cols = left.shape
    D = prm.disparities
    cl, cr = np.zeros((rows, cols), dtype=np.uint64), np.zeros((rows, cols), dtype=np.uint64)
    Lv, S, dR = np.zeros((rows, cols, D), dtype=np.uint8), np.zeros((rows, cols, D), dtype=np.uint16), np.zeros((rows, cols), dtype=np.uint8)
    ctx.check(lib.ssx_dense_debug_stages(ctx.handle, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], rows, cols, C.byref(prm),
                                         int(direction), cl.ctypes.data, cr.ctypes.data, Lv.ctypes.data, S.ctypes.data, dR.ctypes.data))
    return dict(census_left=cl, census_right=cr, path_volume=Lv, sum_volume=S, right_disparity=dR)
