"""Image undistortion over ctypes: ssx_undistort / ssx_undistort_default (include/ssx.h; contract: tools/undistort_model.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, UndistortJob, UndistortParams, load


def _fns(lib):
    if not getattr(lib, "_undistort_ready", False):
        lib.ssx_undistort_default.restype = None
        lib.ssx_undistort_default.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(UndistortParams)]
        lib.ssx_undistort.restype = C.c_int
        lib.ssx_undistort.argtypes = [C.c_void_p, C.c_int32, C.POINTER(UndistortJob), C.c_int32, C.c_int32, C.c_int32]
        if hasattr(lib, "ssx_undistort_debug_last_call"):       # include/ssx_test_hooks.h: absent from a product build
            i32_p, i64_p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
            lib.ssx_undistort_debug_last_call.restype = C.c_int
            lib.ssx_undistort_debug_last_call.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p]
        lib._undistort_ready = True
    return lib


def make_params(K, dist, iR=None) -> UndistortParams:
    """K = (fx, fy, cx, cy); dist = (k1, k2, p1, p2[, k3]); iR = 9 doubles (inverse of newK * R), default: ssx_undistort_default's
    (R = I, newK = K).  Needs no device."""
    lib = _fns(load())
    d = [float(v) for v in dist] + [0.0] * (5 - len(dist))
    if len(K) != 4 or len(d) != 5:
        raise ValueError("K has 4 entries, dist 4 or 5")
    out = UndistortParams()
    lib.ssx_undistort_default((C.c_double * 4)(*[float(v) for v in K]), (C.c_double * 5)(*d), C.byref(out))
    if iR is not None:
        iR = np.asarray(iR, dtype=np.float64).reshape(-1)
        if iR.size != 9:
            raise ValueError("iR has 9 entries")
        out.iR[:] = [float(v) for v in iR]
    return out


def undistort_ptrs(ctx: Context, jobs, rows, cols, images_on_device=True):
    """ssx_undistort on memory the caller holds: jobs = [(src address, src stride, dst address, dst stride, UndistortParams)]"""
    lib = _fns(ctx.lib)
    n = len(jobs)
    arr = (UndistortJob * max(n, 1))()
    for k, (src, ss, dst, ds, prm) in enumerate(jobs):
        arr[k].src = src; arr[k].src_stride = ss; arr[k].dst = dst; arr[k].dst_stride = ds; arr[k].prm = prm
    ctx.check(lib.ssx_undistort(ctx.handle, n, arr, rows, cols, 1 if images_on_device else 0))


def undistort(ctx: Context, images, params, dst_stride=None):
    """One ssx_undistort call over host images.  images: 2-D uint8 arrays of one shape (a row pitch is kept: only the last axis must be
    contiguous); params: one UndistortParams per image.  -> the undistorted images, contiguous unless dst_stride (bytes, >= cols) is
    given: then each is the [rows, cols] view of a [rows, dst_stride] buffer of zeros."""
    if len(images) != len(params):
        raise ValueError("one parameter set per image")
    if not images:
        return []
    rows, cols = images[0].shape
    outs, jobs = [], []
    for im, prm in zip(images, params):
        if im.dtype != np.uint8 or im.ndim != 2 or im.shape != (rows, cols) or im.strides[1] != 1 or im.strides[0] < cols:
            raise ValueError("images: 2-D uint8 arrays of one shape with contiguous rows")
        buf = np.zeros((rows, cols if dst_stride is None else int(dst_stride)), dtype=np.uint8)
        outs.append(buf)
        jobs.append((im.ctypes.data, im.strides[0], buf.ctypes.data, buf.strides[0], prm))
    undistort_ptrs(ctx, jobs, rows, cols, images_on_device=False)
    return [b[:, :cols] for b in outs]


def last_call(ctx: Context):
    """ssx_undistort_debug_last_call -> dict(launches, syncs, bytes_up, bytes_down) of the context's last ssx_undistort"""
    lib = _fns(ctx.lib)
    a, b, c, d = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    ctx.check(lib.ssx_undistort_debug_last_call(ctx.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return dict(launches=a.value, syncs=b.value, bytes_up=c.value, bytes_down=d.value)
