"""Dense stereo over ctypes: ssx_stereo_dense / ssx_dense_default_params (include/ssx.h; contract: tools/dense_model.py) -- a disparity
for every pixel of a rectified pair by census + semi-global matching, int16 in 1/16 pixel, -16 where a pixel is invalid."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, DenseJob, DenseParamsC, load

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
        if hasattr(lib, "ssx_dense_debug_last_call"):           # include/ssx_test_hooks.h: absent from a product build
            i32_p, i64_p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
            lib.ssx_dense_debug_last_call.restype = C.c_int
            lib.ssx_dense_debug_last_call.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p, i32_p]
            lib.ssx_dense_debug_stages.restype = C.c_int
            lib.ssx_dense_debug_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DenseParamsC),
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
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


def dense_disparity_batch(ctx: Context, pairs, params=None, on_device=False, disp_stride=None):
    """One ssx_stereo_dense call over pairs = [(left, right)].
    on_device=False: 2-D uint8 numpy arrays of one shape (a row pitch is kept) -> int16 arrays [rows, cols] (with disp_stride, in
    elements: each the [rows, cols] view of a [rows, disp_stride] buffer filled with 0x5a5a).
    on_device=True: 2-D uint8 torch tensors on the context's device (a row pitch is kept) -> int16 torch tensors on that device, read
    and written where they lie."""
    if not pairs:
        return []
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
    dense_ptrs(ctx, jobs, rows, cols, params, images_on_device=on_device)
    return [d[:, :cols] for d in outs]


def dense_disparity(ctx: Context, left, right, params=None):
    """The disparity map of one rectified pair of host images -> int16 [rows, cols] in 1/16 pixel, INVALID (-16) where a check fails"""
    return dense_disparity_batch(ctx, [(left, right)], params)[0]


def last_call(ctx: Context):
    """ssx_dense_debug_last_call -> dict(launches, syncs, bytes_up, bytes_down, groups) of the context's last ssx_stereo_dense"""
    lib = _fns(ctx.lib)
    a, b, c, d, e = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    ctx.check(lib.ssx_dense_debug_last_call(ctx.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
    return dict(launches=a.value, syncs=b.value, bytes_up=c.value, bytes_down=d.value, groups=e.value)


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
