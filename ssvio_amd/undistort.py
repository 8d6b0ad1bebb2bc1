"""Image undistortion over ctypes: ssx_undistort / ssx_undistort_default and the plan of stored maps, ssx_undistort_plan_* (include/ssx.h;
contract: tools/undistort_model.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, UndistortJob, UndistortParams, UndistortPlanJob, load


def _fns(lib):
    if not getattr(lib, "_undistort_ready", False):
        lib.ssx_undistort_default.restype = None
        lib.ssx_undistort_default.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(UndistortParams)]
        lib.ssx_undistort.restype = C.c_int
        lib.ssx_undistort.argtypes = [C.c_void_p, C.c_int32, C.POINTER(UndistortJob), C.c_int32, C.c_int32, C.c_int32]
        i32_p, i64_p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        if hasattr(lib, "ssx_undistort_debug_last_call"):       # include/ssx_test_hooks.h: absent from a product build
            lib.ssx_undistort_debug_last_call.restype = C.c_int
            lib.ssx_undistort_debug_last_call.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p]
        lib.ssx_undistort_plan_create.restype = C.c_int
        lib.ssx_undistort_plan_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.ssx_undistort_plan_add.restype = C.c_int
        lib.ssx_undistort_plan_add.argtypes = [C.c_void_p, C.POINTER(UndistortParams), i32_p]
        lib.ssx_undistort_plan_apply.restype = C.c_int
        lib.ssx_undistort_plan_apply.argtypes = [C.c_void_p, C.c_int32, C.POINTER(UndistortPlanJob), C.c_int32]
        lib.ssx_undistort_plan_size.restype = C.c_int
        lib.ssx_undistort_plan_size.argtypes = [C.c_void_p, i32_p, i32_p, i32_p]
        lib.ssx_undistort_plan_destroy.restype = None
        lib.ssx_undistort_plan_destroy.argtypes = [C.c_void_p]
        if hasattr(lib, "ssx_undistort_plan_debug_last_call"):  # include/ssx_test_hooks.h
            lib.ssx_undistort_plan_debug_last_call.restype = C.c_int
            lib.ssx_undistort_plan_debug_last_call.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p, i32_p, i32_p]
            lib.ssx_undistort_plan_debug_map.restype = C.c_int
            lib.ssx_undistort_plan_debug_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint16)]
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


class UndistortPlan:
    """ssx_undistort_plan: the stored maps of one image size (one per camera shown to `add`), applied to n images in one launch.  The
    result is ssx_undistort's, byte for byte; the stored form is tools/undistort_model.py's pack_map."""

    def __init__(self, ctx: Context, rows, cols):
        self.ctx, self.lib = ctx, _fns(ctx.lib)
        self.rows, self.cols = int(rows), int(cols)
        h = C.c_void_p()
        ctx.check(self.lib.ssx_undistort_plan_create(ctx.handle, self.rows, self.cols, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            self.lib.ssx_undistort_plan_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def add(self, prm: UndistortParams) -> int:
        """-> the index of the parameter set's map; equal bytes return the index they have, a new set launches k_undistort_map once"""
        m = C.c_int32(-1)
        self.ctx.check(self.lib.ssx_undistort_plan_add(self.handle, C.byref(prm), C.byref(m)))
        return m.value

    def size(self):
        """-> (rows, cols, number of maps)"""
        a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.ctx.check(self.lib.ssx_undistort_plan_size(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def apply_ptrs(self, jobs, images_on_device=True):
        """ssx_undistort_plan_apply on memory the caller holds: jobs = [(src address, src stride, dst address, dst stride, map index)]"""
        n = len(jobs)
        arr = (UndistortPlanJob * max(n, 1))()
        for k, (src, ss, dst, ds, m) in enumerate(jobs):
            arr[k].src = src; arr[k].src_stride = ss; arr[k].dst = dst; arr[k].dst_stride = ds; arr[k].map = m
        self.ctx.check(self.lib.ssx_undistort_plan_apply(self.handle, n, arr, 1 if images_on_device else 0))

    def apply(self, images, maps, dst_stride=None):
        """One call over host images (2-D uint8 arrays of the plan's shape, contiguous rows; a row pitch is kept) with one map index each
        -> the undistorted images, as undistort() returns them"""
        if len(images) != len(maps):
            raise ValueError("one map index per image")
        outs, jobs = [], []
        for im, m in zip(images, maps):
            if im.dtype != np.uint8 or im.ndim != 2 or im.shape != (self.rows, self.cols) or im.strides[1] != 1 or im.strides[0] < self.cols:
                raise ValueError("images: 2-D uint8 arrays of the plan's shape with contiguous rows")
            buf = np.zeros((self.rows, self.cols if dst_stride is None else int(dst_stride)), dtype=np.uint8)
            outs.append(buf)
            jobs.append((im.ctypes.data, im.strides[0], buf.ctypes.data, buf.strides[0], int(m)))
        self.apply_ptrs(jobs, images_on_device=False)
        return [b[:, :self.cols] for b in outs]

    def packed_map(self, m):
        """ssx_undistort_plan_debug_map -> (xs, ys, ab), three uint16 [rows, cols]: pack_map's form of map m"""
        out = np.zeros((3, self.rows, self.cols), dtype=np.uint16)
        self.ctx.check(self.lib.ssx_undistort_plan_debug_map(self.handle, int(m), out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out[0], out[1], out[2]

    def last_call(self):
        """ssx_undistort_plan_debug_last_call -> dict(launches, syncs, bytes_up, bytes_down, copies_up, copies_down) of the plan's last
        add or apply"""
        a, b, c, d, e, f = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
        self.ctx.check(self.lib.ssx_undistort_plan_debug_last_call(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), C.byref(f)))
        return dict(launches=a.value, syncs=b.value, bytes_up=c.value, bytes_down=d.value, copies_up=e.value, copies_down=f.value)
