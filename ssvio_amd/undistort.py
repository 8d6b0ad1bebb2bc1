"""Image undistortion over ctypes: ssx_undistort / ssx_undistort_default and the plan of stored maps, ssx_undistort_plan_* (include/ssx.h;
contract: tools/undistort_model.py); and raw stereo rigs: ssx_stereo_rectify, ssx_undistort_lens, ssx_undistort_plan_add_lens with a lens
model (radtan or kb4) per image (contract: tools/rectify_model.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context, LensJob, LensParams, StereoRawRig, StereoRectified, UndistortJob, UndistortParams, UndistortPlanJob, load


ENTRY_UNDISTORT, ENTRY_LENS, ENTRY_PLAN_APPLY = 0, 1, 2      # include/ssx_test_hooks.h: SSX_UD_ENTRY_*
STAGED, IN_PLACE, RANGE, EACH = 0, 1, 2, 3                   # SSX_UD_*: how one side's images reach the device
NEITHER, DEVICE, PINNED = -1, 0, 1                           # a side's facts: kind[k]
WHERE_IT_LIES, BASE, STAGING = -1, 1 << 40, None             # SSX_UD_WHERE_IT_LIES, SSX_UD_BASE; a copy's host_off when it is the staging buffer


class UndistortJobFacts(C.Structure):
    """ssx_undistort_job_facts: offsets from job 0's src; tag = lens model or map index; flags 1 / 2: src / dst is null"""
    _fields_ = [("src_off", C.c_int64), ("dst_off", C.c_int64), ("src_stride", C.c_int32), ("dst_stride", C.c_int32), ("tag", C.c_int32), ("flags", C.c_int32)]


class UndistortSideFacts(C.Structure):
    _fields_ = [("one_allocation", C.c_int32), ("reserved", C.c_int32), ("kind", C.POINTER(C.c_int8))]


class _CallJob(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("src_off", "dst_off", "src_stride", "dst_stride")]     # (offsets read as signed: WHERE_IT_LIES is -1)


class _CallUp(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("off", "host", "bytes", "images")]


class _CallDown(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("host", "host_pitch", "off", "dev_pitch", "width", "height")]


class UndistortCallInfo(C.Structure):
    """ssx_undistort_call_info"""
    _fields_ = [("status", C.c_int32), ("error", C.c_char * 256), ("grid", C.c_int32 * 3), ("block", C.c_int32 * 3), ("src_intake", C.c_int32),
                ("dst_intake", C.c_int32), ("span_off", C.c_uint64 * 3), ("span_bytes", C.c_uint64 * 3), ("up_bytes", C.c_uint64),
                ("arena_bytes", C.c_uint64), ("stage_bytes", C.c_uint64), ("n_jobs", C.c_int32), ("n_up", C.c_int32), ("n_down", C.c_int32),
                ("launches", C.c_int32), ("syncs", C.c_int32), ("copies_up", C.c_int32), ("copies_down", C.c_int32), ("reserved", C.c_int32),
                ("bytes_up", C.c_int64), ("bytes_down", C.c_int64), ("job", _CallJob * 1024), ("up", _CallUp * 1025), ("down", _CallDown * 1024)]


def debug_plan(entry, rows, cols, jobs, images_on_device=False, n_maps=0, src_facts=None, dst_facts=None, n=None, null_table=False):
    """ssx_undistort_debug_plan: the call an entry point (ENTRY_*) would issue, planned without a GPU.
    jobs = [(src_off, src_stride, dst_off, dst_stride, tag)], offsets in bytes from job 0's src, None for a null pointer; n overrides the
    count handed in; *_facts = (one_allocation, [kind per image]) as the runtime would answer.
    -> dict: status, error, and for SSX_OK with n > 0: grid, block, src_intake, dst_intake, spans [(off, bytes)] of table / sources /
    results, up_bytes, arena_bytes, stage_bytes, jobs [dict], up [dict], down [dict], stats (the dict last_call() would return)"""
    lib = _fns(load())
    arr = (UndistortJobFacts * max(len(jobs), 1))()
    for k, (so, ss, do, ds, tag) in enumerate(jobs):
        arr[k] = UndistortJobFacts(so or 0, do or 0, ss, ds, tag, (1 if so is None else 0) | (2 if do is None else 0))
    keep, sides = [], []
    for f in (src_facts, dst_facts):
        if f is None:
            sides.append(None)
            continue
        kinds = (C.c_int8 * max(len(f[1]), 1))(*f[1])
        keep.append(kinds)
        sides.append(C.byref(UndistortSideFacts(1 if f[0] else 0, 0, C.cast(kinds, C.POINTER(C.c_int8)))))
    info = UndistortCallInfo()
    st = lib.ssx_undistort_debug_plan(entry, rows, cols, 1 if images_on_device else 0, len(jobs) if n is None else n, None if null_table else arr, n_maps,
                                      sides[0], sides[1], C.byref(info))
    assert st == info.status
    out = dict(status=info.status, error=info.error.decode())
    if info.status != 0 or info.n_jobs == 0:
        return out
    def rec(s):                                                   # a copy's host address -> host_off: from jobs[0].src's origin, or STAGING
        d = {k: getattr(s, k) for k, _ in s._fields_}
        if "host" in d:
            host = d.pop("host")
            d["host_off"] = host - BASE if host else STAGING
        return d

    out.update(grid=tuple(info.grid), block=tuple(info.block), src_intake=info.src_intake, dst_intake=info.dst_intake,
               spans=[(info.span_off[i], info.span_bytes[i]) for i in range(3)], up_bytes=info.up_bytes, arena_bytes=info.arena_bytes,
               stage_bytes=info.stage_bytes, jobs=[rec(info.job[k]) for k in range(info.n_jobs)], up=[rec(info.up[k]) for k in range(info.n_up)],
               down=[rec(info.down[k]) for k in range(info.n_down)],
               stats=dict(launches=info.launches, syncs=info.syncs, bytes_up=info.bytes_up, bytes_down=info.bytes_down, copies_up=info.copies_up,
                          copies_down=info.copies_down))
    return out


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
        if hasattr(lib, "ssx_undistort_lens"):                  # (an older build named by SSX_LIB lacks them: the A/B runs of tools/; using one then raises)
            lib.ssx_undistort_lens.restype = C.c_int
            lib.ssx_undistort_lens.argtypes = [C.c_void_p, C.c_int32, C.POINTER(LensJob), C.c_int32, C.c_int32, C.c_int32]
            lib.ssx_undistort_plan_add_lens.restype = C.c_int
            lib.ssx_undistort_plan_add_lens.argtypes = [C.c_void_p, C.POINTER(LensParams), i32_p]
            lib.ssx_stereo_rectify.restype = C.c_int
            lib.ssx_stereo_rectify.argtypes = [C.POINTER(StereoRawRig), C.POINTER(StereoRectified), C.c_char_p, C.c_int32]
        if hasattr(lib, "ssx_undistort_debug_plan"):            # include/ssx_test_hooks.h
            lib.ssx_undistort_debug_plan.restype = C.c_int
            lib.ssx_undistort_debug_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(UndistortJobFacts), C.c_int32,
                                                     C.POINTER(UndistortSideFacts), C.POINTER(UndistortSideFacts), C.POINTER(UndistortCallInfo)]
        if hasattr(lib, "ssx_lens_debug_atan"):                 # include/ssx_test_hooks.h
            lib.ssx_lens_debug_atan.restype = C.c_int
            lib.ssx_lens_debug_atan.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
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


def make_lens_params(model, K, coeffs, iR=None) -> LensParams:
    """model = SSX_LENS_RADTAN (coeffs = k1 k2 p1 p2[ k3]) or SSX_LENS_KB4 (coeffs = k1 k2 k3 k4); K = (fx, fy, cx, cy); iR = 9 doubles
    (inverse of newK * R), default: ssx_undistort_default's (R = I, newK = K).  Needs no device."""
    co = [float(v) for v in coeffs] + [0.0] * (5 - len(coeffs))
    if len(co) != 5:
        raise ValueError("coeffs has at most 5 entries")
    base = make_params(K, co, iR)
    out = LensParams()
    out.model = int(model)
    out.K[:] = base.K[:]
    out.coeffs[:] = base.dist[:]
    out.iR[:] = base.iR[:]
    return out


def stereo_rectify(cams, R, t, f=None, cx=None, cy=None) -> StereoRectified:
    """ssx_stereo_rectify (host arithmetic, no device; contract: tools/rectify_model.py's rectify).  cams = the left and the right
    LensParams (iR ignored), X_right = R X_left + t; f, cx, cy: the common camera's, None or 0 for the default.  -> StereoRectified,
    whose cam[0], cam[1] are ready for undistort_lens / UndistortPlan.add_lens.  A refused rig raises ValueError with the reason."""
    lib = _fns(load())
    rig = StereoRawRig()
    rig.cam[0], rig.cam[1] = cams
    rig.R[:] = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)]
    rig.t[:] = [float(v) for v in np.asarray(t, dtype=np.float64).reshape(3)]
    rig.f, rig.cx, rig.cy = (0.0 if v is None else float(v) for v in (f, cx, cy))
    out = StereoRectified()
    why = C.create_string_buffer(160)
    if lib.ssx_stereo_rectify(C.byref(rig), C.byref(out), why, len(why)) != 0:
        raise ValueError(why.value.decode())
    return out


def undistort_ptrs(ctx: Context, jobs, rows, cols, images_on_device=True):
    """ssx_undistort, or ssx_undistort_lens when the first job's parameters are LensParams, on memory the caller holds:
    jobs = [(src address, src stride, dst address, dst stride, UndistortParams or LensParams)]"""
    lib = _fns(ctx.lib)
    n = len(jobs)
    lens = n > 0 and isinstance(jobs[0][4], LensParams)
    arr = ((LensJob if lens else UndistortJob) * max(n, 1))()
    for k, (src, ss, dst, ds, prm) in enumerate(jobs):
        arr[k].src = src; arr[k].src_stride = ss; arr[k].dst = dst; arr[k].dst_stride = ds; arr[k].prm = prm
    ctx.check((lib.ssx_undistort_lens if lens else lib.ssx_undistort)(ctx.handle, n, arr, rows, cols, 1 if images_on_device else 0))


def undistort_lens(ctx: Context, images, params, dst_stride=None):
    """undistort() through ssx_undistort_lens: params is one LensParams per image, of either model"""
    if not all(isinstance(p, LensParams) for p in params):
        raise ValueError("one LensParams per image")
    return undistort(ctx, images, params, dst_stride=dst_stride)


def lens_atan(ctx: Context, r):
    """ssx_lens_debug_atan -> (atan_c(r), sqrt(r)) as the device computes them, float64 arrays of r's shape"""
    lib = _fns(ctx.lib)
    r = np.ascontiguousarray(r, dtype=np.float64)
    a, s = np.empty_like(r), np.empty_like(r)
    dp = C.POINTER(C.c_double)
    ctx.check(lib.ssx_lens_debug_atan(ctx.handle, r.size, r.ctypes.data_as(dp), a.ctypes.data_as(dp), s.ctypes.data_as(dp)))
    return a, s


def undistort(ctx: Context, images, params, dst_stride=None):
    """One ssx_undistort call over host images.  images: 2-D uint8 arrays of one shape (a row pitch is kept: only the last axis must be
    contiguous); params: one UndistortParams per image (or one LensParams per image: ssx_undistort_lens).  -> the undistorted images,
    contiguous unless dst_stride (bytes, >= cols) is given: then each is the [rows, cols] view of a [rows, dst_stride] buffer of zeros."""
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

    def add_lens(self, prm: LensParams) -> int:
        """add() for a lens of either model (ssx_undistort_plan_add_lens); a RADTAN lens and its UndistortParams form are one map"""
        m = C.c_int32(-1)
        self.ctx.check(self.lib.ssx_undistort_plan_add_lens(self.handle, C.byref(prm), C.byref(m)))
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
