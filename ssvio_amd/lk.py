"""Pyramidal Lucas-Kanade tracking: the host-side mirror of the two
cv::calcOpticalFlowPyrLK calls of the reference front-end (frontend.cpp:156-166 and :374-384)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import Context


class LkParams(C.Structure):
    _fields_ = [("win", C.c_int32), ("max_level", C.c_int32), ("max_iters", C.c_int32), ("eps", C.c_double),
                ("min_eig_threshold", C.c_float), ("use_initial_flow", C.c_int32)]


u8_p = C.POINTER(C.c_ubyte)
f32_p = C.POINTER(C.c_float)


def _img(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.ndim == 2
    return a


def calcOpticalFlowPyrLK(ctx: Context, prev, nxt, prev_pts, next_pts=None, winSize=11, maxLevel=3, maxCount=30,
                         epsilon=0.01, minEigThreshold=1e-4):
    """cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(win, win), maxLevel,
    TermCriteria(COUNT+EPS, maxCount, epsilon), next_pts is None ? 0 : OPTFLOW_USE_INITIAL_FLOW, minEigThreshold).
    Returns (next_pts [n,2] f32, status [n] u8, err [n] f32, top_level).
    prev=None chains frames (ssx_lk_track_next): the previous image is the `nxt` image of the last call on ctx,
    whose pyramid is still on the device."""
    nxt = _img(nxt)
    chain = prev is None
    if not chain:
        prev = _img(prev)
        if prev.shape != nxt.shape:
            raise ValueError("calcOpticalFlowPyrLK: the two images must have the same size")
    pp = np.ascontiguousarray(prev_pts, dtype=np.float32).reshape(-1, 2)
    use_init = next_pts is not None
    npts = np.ascontiguousarray(next_pts, dtype=np.float32).reshape(-1, 2).copy() if use_init else pp.copy()
    if len(npts) != len(pp):
        raise ValueError("calcOpticalFlowPyrLK: prev_pts and next_pts differ in length")
    n = len(pp)
    status = np.zeros(n, np.uint8); err = np.zeros(n, np.float32)
    prm = LkParams(int(winSize), int(maxLevel), int(maxCount), float(epsilon), float(minEigThreshold), int(use_init))
    top = C.c_int32(0)
    lib = ctx.lib
    lib.ssx_lk_track.restype = C.c_int
    lib.ssx_lk_track_next.restype = C.c_int
    if chain:
        ctx.check(lib.ssx_lk_track_next(ctx.handle, nxt.ctypes.data_as(u8_p), nxt.strides[0], nxt.shape[0], nxt.shape[1], n,
                                        pp.ctypes.data_as(f32_p), npts.ctypes.data_as(f32_p), status.ctypes.data_as(u8_p),
                                        err.ctypes.data_as(f32_p), C.byref(prm), C.byref(top)))
        return npts, status, err, top.value
    ctx.check(lib.ssx_lk_track(ctx.handle, prev.ctypes.data_as(u8_p), prev.strides[0], nxt.ctypes.data_as(u8_p), nxt.strides[0],
                               prev.shape[0], prev.shape[1], n, pp.ctypes.data_as(f32_p), npts.ctypes.data_as(f32_p),
                               status.ctypes.data_as(u8_p), err.ctypes.data_as(f32_p), C.byref(prm), C.byref(top)))
    return npts, status, err, top.value


class LkJob(C.Structure):
    _fields_ = [("slot", C.c_int32), ("prev", u8_p), ("prev_stride", C.c_int32), ("next", u8_p), ("next_stride", C.c_int32), ("n", C.c_int32),
                ("prev_pts", f32_p), ("next_pts", f32_p), ("status", u8_p), ("err", f32_p)]


def _batch_fn(lib):
    """ssx_lk_track_batch with its C signature, declared in one place"""
    fn = lib.ssx_lk_track_batch
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(LkJob), C.c_int32, C.c_int32, C.POINTER(LkParams), C.c_int32]
    return fn


def _fill_job(a, j, next_ptr, next_stride, prev_ptr=None, prev_stride=0):
    """one ssx_lk_job from a job dict (slot, prev_pts, next_pts or None) and its image pointers -> (prev_pts, guess, outputs): the
    arrays the struct points into"""
    pp = np.ascontiguousarray(j["prev_pts"], dtype=np.float32).reshape(-1, 2)
    guess = np.ascontiguousarray(j["next_pts"], dtype=np.float32).reshape(-1, 2).copy() if j.get("next_pts") is not None else pp.copy()
    npts = guess.copy(); st = np.zeros(len(pp), np.uint8); er = np.zeros(len(pp), np.float32)
    a.slot = int(j["slot"])
    a.prev = prev_ptr; a.prev_stride = prev_stride
    a.next = next_ptr; a.next_stride = next_stride
    a.n = len(pp); a.prev_pts = pp.ctypes.data_as(f32_p); a.next_pts = npts.ctypes.data_as(f32_p)
    a.status = st.ctypes.data_as(u8_p); a.err = er.ctypes.data_as(f32_p)
    return pp, guess, (npts, st, er)


class PreparedTrackBatch:
    """ssx_lk_track_batch with everything a C caller holds between frames prepared once: the job structs, the points, and the images in
    PINNED memory handed over with images_on_device = 1 -- ONE arena (ssx_host_alloc) with a slice per job, as
    ssvio_amd/host/stream_batcher.cpp keeps its streams' images, so that they cross in one copy (a pinned allocation per image is never
    one copy, however the allocator places them: include/ssx.h).  run() is the library call alone; outputs in .outs
    [(next_pts, status, err)] (the guesses are restored before every run)."""

    def __init__(self, ctx: Context, jobs, winSize=11, maxLevel=3, maxCount=30, epsilon=0.01, minEigThreshold=1e-4):
        self.ctx = ctx
        lib = ctx.lib
        lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
        lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
        n = len(jobs)
        self.arr = (LkJob * n)()
        self.keep, self.outs, self.guess, self.pins = [], [], [], []
        use_init = any(j.get("next_pts") is not None for j in jobs)
        imgs = [_img(j["next"]) for j in jobs]
        self.rows, self.cols = imgs[0].shape
        slice_bytes = (imgs[0].size + 255) & ~255
        arena = lib.ssx_host_alloc(n * slice_bytes)
        if not arena:
            raise MemoryError("ssx_host_alloc")
        self.pins.append(arena)
        for i, (j, nxt) in enumerate(zip(jobs, imgs)):
            if nxt.shape != imgs[0].shape:
                raise ValueError("PreparedTrackBatch: the jobs of a call share the image size")
            pin = arena + i * slice_bytes
            C.memmove(pin, nxt.ctypes.data, nxt.size)
            pp, g, out = _fill_job(self.arr[i], j, C.cast(pin, u8_p), self.cols)
            self.keep.append(pp); self.outs.append(out); self.guess.append(g)
        self.n = n
        self.prm = LkParams(int(winSize), int(maxLevel), int(maxCount), float(epsilon), float(minEigThreshold), int(use_init))
        self.fn = _batch_fn(lib)

    def run(self):
        for (npts, _, _), g in zip(self.outs, self.guess):
            npts[:] = g
        self.ctx.check(self.fn(self.ctx.handle, self.n, self.arr, self.rows, self.cols, C.byref(self.prm), 1))
        return self.outs

    def close(self):
        for p_ in self.pins:
            self.ctx.lib.ssx_host_free(p_)
        self.pins = []


def track_batch(ctx: Context, jobs, winSize=11, maxLevel=3, maxCount=30, epsilon=0.01, minEigThreshold=1e-4, images_on_device=False):
    """ssx_lk_track_batch: jobs = [dict(slot, prev (image or None = chained to the slot's last job), next, prev_pts, next_pts or None)];
    every job with the same image size.  -> [(next_pts, status, err)] per job.  images_on_device: the arrays' memory is readable by
    the GPU (pinned)."""
    n = len(jobs)
    arr = (LkJob * n)()
    keep, outs = [], []
    use_init = any(j.get("next_pts") is not None for j in jobs)
    rows = cols = None
    for i, j in enumerate(jobs):
        nxt = _img(j["next"]); prev = None if j.get("prev") is None else _img(j["prev"])
        rows, cols = nxt.shape
        pp, _, out = _fill_job(arr[i], j, nxt.ctypes.data_as(u8_p), nxt.strides[0], None if prev is None else prev.ctypes.data_as(u8_p),
                               0 if prev is None else prev.strides[0])
        keep.append((nxt, prev, pp)); outs.append(out)
    prm = LkParams(int(winSize), int(maxLevel), int(maxCount), float(epsilon), float(minEigThreshold), int(use_init))
    ctx.check(_batch_fn(ctx.lib)(ctx.handle, n, arr, rows, cols, C.byref(prm), 1 if images_on_device else 0))
    return outs


def track_batch_ptrs(ctx: Context, jobs, rows, cols, winSize=11, maxLevel=3, maxCount=30, epsilon=0.01, minEigThreshold=1e-4):
    """ssx_lk_track_batch with images_on_device = 1 on images the caller holds in memory the GPU can read: jobs = [dict(slot, prev
    (address or None), next (address), stride, prev_pts, next_pts or None)].  -> [(next_pts, status, err)] per job."""
    arr = (LkJob * len(jobs))()
    use_init = any(j.get("next_pts") is not None for j in jobs)
    filled = [_fill_job(arr[i], j, C.cast(j["next"], u8_p), j["stride"], None if j.get("prev") is None else C.cast(j["prev"], u8_p),
                        0 if j.get("prev") is None else j["stride"]) for i, j in enumerate(jobs)]
    prm = LkParams(int(winSize), int(maxLevel), int(maxCount), float(epsilon), float(minEigThreshold), int(use_init))
    ctx.check(_batch_fn(ctx.lib)(ctx.handle, len(jobs), arr, rows, cols, C.byref(prm), 1))
    return [f[2] for f in filled]


# ---- the plan of a call (include/ssx_test_hooks.h: ssx_lk_debug_plan needs no GPU, ssx_lk_debug_last_call reports the last call) ----
STAGED, ARENA, EACH, IN_PLACE = range(4)
FACT_NEXT0_IS_HOST, FACT_SEVERAL_ALLOCATIONS = 1, 2
KERNELS = ("k_lk_pyramid", "k_lk_pad_level0", "k_lk_pyr_down", "k_lk_scharr", "k_lk_track")
SPANS = ("tab", "images", "prev_pts", "next_pts", "status", "err", "dev_images")


class LkLaunch(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("grid", C.c_int32 * 3), ("which", C.c_int32), ("level", C.c_int32)]


class LkCallInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("error", C.c_char * 256), ("levels", C.c_int32), ("win", C.c_int32), ("pad", C.c_int32),
                ("rows", C.c_int32 * 8), ("cols", C.c_int32 * 8), ("pitch", C.c_int32 * 8), ("off", C.c_uint64 * 8), ("doff", C.c_uint64 * 8),
                ("pyr_bytes", C.c_uint64), ("deriv_words", C.c_uint64), ("fused_ok", C.c_int32), ("use_fused", C.c_int32),
                ("scharr_now", C.c_int32), ("intake", C.c_int32), ("span_off", C.c_uint64 * 7), ("span_bytes", C.c_uint64 * 7),
                ("in_bytes", C.c_uint64), ("host_end", C.c_uint64), ("io_bytes", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("n_launches", C.c_int32), ("n_jobs", C.c_int32), ("launch", LkLaunch * 32), ("slot_flags", C.c_uint8 * 256),
                ("job_roles", C.c_uint8 * 256)]


class LkJobFacts(C.Structure):
    _fields_ = [("slot", C.c_int32), ("fresh", C.c_int32), ("n", C.c_int32), ("prev_stride", C.c_int32), ("next_stride", C.c_int32),
                ("reserved", C.c_int32), ("next_off", C.c_int64)]


def debug_plan(lib, rows, cols, jobs, slot_flags=None, win=11, max_level=3, planned_key=None, images_on_device=0, next0_is_host=0, one_allocation=1):
    """ssx_lk_debug_plan: jobs = [dict(slot, fresh, n, prev_stride, next_stride, next_off)] (strides default to cols, next_off to
    job index x rows x cols); slot_flags per job (default: 3 for a chained job, 0 for a fresh one); next0_is_host, one_allocation:
    what the runtime would answer about the image pointers -> LkCallInfo"""
    n = len(jobs)
    arr = (LkJobFacts * n)()
    for i, j in enumerate(jobs):
        arr[i] = LkJobFacts(j["slot"], int(j["fresh"]), j.get("n", 0), j.get("prev_stride", cols if j["fresh"] else 0),
                            j.get("next_stride", cols), 0, j.get("next_off", i * rows * cols))
    if slot_flags is None:
        slot_flags = [0 if j["fresh"] else 3 for j in jobs]
    out = LkCallInfo()
    key = None if planned_key is None else (C.c_int32 * 4)(*planned_key)
    lib.ssx_lk_debug_plan.restype = C.c_int
    lib.ssx_lk_debug_plan.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_int32), C.c_int32, C.POINTER(LkJobFacts), C.POINTER(C.c_uint8), C.c_int32,
                                                        C.c_int32, C.POINTER(LkCallInfo)]
    call_facts = (FACT_NEXT0_IS_HOST if next0_is_host else 0) | (0 if one_allocation else FACT_SEVERAL_ALLOCATIONS)
    st = lib.ssx_lk_debug_plan(rows, cols, win, max_level, key, n, arr, (C.c_uint8 * n)(*slot_flags), int(images_on_device), call_facts, C.byref(out))
    assert st == out.status
    return out


def debug_intake(ctx: Context, nexts, rows, cols, stride=None, winSize=11, maxLevel=3):
    """ssx_lk_debug_intake: which intake ssx_lk_track_batch (images_on_device = 1) would take for jobs whose `next` images are at the
    addresses `nexts` -> (intake, the pointers pass the arena's arithmetic).  Asks the runtime about the pointers, runs nothing."""
    arr = (LkJob * len(nexts))()
    for i, a in enumerate(nexts):
        arr[i].slot = i; arr[i].next = C.cast(a, u8_p); arr[i].next_stride = cols if stride is None else stride
    prm = LkParams(int(winSize), int(maxLevel), 30, 0.01, 1e-4, 1)
    intake, arithmetic = C.c_int32(-1), C.c_int32(-1)
    fn = ctx.lib.ssx_lk_debug_intake
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(LkJob), C.c_int32, C.c_int32, C.POINTER(LkParams), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    ctx.check(fn(ctx.handle, len(nexts), arr, rows, cols, C.byref(prm), 1, C.byref(intake), C.byref(arithmetic)))
    return intake.value, bool(arithmetic.value)


def last_call(ctx: Context):
    """ssx_lk_debug_last_call -> LkCallInfo of the last successful LK call of ctx"""
    out = LkCallInfo()
    ctx.lib.ssx_lk_debug_last_call.restype = C.c_int
    ctx.lib.ssx_lk_debug_last_call.argtypes = [C.c_void_p, C.POINTER(LkCallInfo)]
    ctx.check(ctx.lib.ssx_lk_debug_last_call(ctx.handle, C.byref(out)))
    return out


def stage_level(ctx: Context, which, level):
    r = C.c_int32(0); c = C.c_int32(0)
    ctx.check(ctx.lib.ssx_lk_stage_level(ctx.handle, which, level, None, 0, C.byref(r), C.byref(c)))
    out = np.zeros((r.value, c.value), np.uint8)
    ctx.check(ctx.lib.ssx_lk_stage_level(ctx.handle, which, level, out.ctypes.data_as(u8_p), out.size, C.byref(r), C.byref(c)))
    return out


def stage_deriv(ctx: Context, level):
    r = C.c_int32(0); c = C.c_int32(0)
    ctx.check(ctx.lib.ssx_lk_stage_deriv(ctx.handle, level, None, 0, C.byref(r), C.byref(c)))
    out = np.zeros((r.value, c.value, 2), np.int16)
    ctx.check(ctx.lib.ssx_lk_stage_deriv(ctx.handle, level, out.ctypes.data_as(C.c_void_p), out.size, C.byref(r), C.byref(c)))
    return out
