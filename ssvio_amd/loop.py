"""The keyframe database of LoopClosing, resident on the device -- ssx_kfdb_* of include/ssx.h: AddToKeyframeDatabase, DetectLoop
and MatchFeatures (reference: src/ssvio/loopclosing.cpp:646-649, :72-103, :105-145)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SSX_ERR_CAPACITY, Context, dbl_p, i32_p, u8_p

i64_p = C.POINTER(C.c_int64)


def _bind(lib):
    if getattr(lib, "_kfdb_bound", False):
        return
    lib.ssx_kfdb_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.ssx_kfdb_destroy.argtypes = [C.c_void_p]
    lib.ssx_kfdb_destroy.restype = None
    lib.ssx_kfdb_size.argtypes = [C.c_void_p, i32_p, i64_p, i64_p]
    lib.ssx_kfdb_add.argtypes = [C.c_void_p, C.c_int64, C.c_int32, i32_p, dbl_p, C.c_int32, u8_p, i32_p]
    lib.ssx_kfdb_detect_loop.argtypes = [C.c_void_p, C.c_int64, C.c_int32, i32_p, dbl_p, C.c_int32, C.c_float, i32_p, i64_p,
                                         C.POINTER(C.c_float), C.c_int32, dbl_p, i32_p]
    lib.ssx_kfdb_match_features.argtypes = [C.c_void_p, C.c_int64, C.c_int32, u8_p, i32_p, C.c_int32, i32_p, i32_p, i32_p]
    lib._kfdb_bound = True


def _bow(bow):
    return np.ascontiguousarray(bow[0], dtype=np.int32), np.ascontiguousarray(bow[1], dtype=np.float64)


class KeyframeDatabase:
    def __init__(self, ctx: Context, keyframes_hint: int = 256):
        _bind(ctx.lib)
        self.ctx, self.handle = ctx, C.c_void_p()
        ctx.check(ctx.lib.ssx_kfdb_create(ctx.handle, int(keyframes_hint), C.byref(self.handle)))

    def close(self):
        if self.handle:
            self.ctx.lib.ssx_kfdb_destroy(self.handle)
            self.handle = None

    def size(self):
        """-> (keyframes, BowVector entries, descriptors) stored"""
        n, nb, nd = C.c_int32(), C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.ssx_kfdb_size(self.handle, C.byref(n), C.byref(nb), C.byref(nd)))
        return n.value, nb.value, nd.value

    def __len__(self):
        return self.size()[0]

    def add(self, kf_id, bow, desc=None, class_id=None):
        """bow = (ids ascending, values); desc [n, 32] uint8 with class_id [n] (the feature index of each pyramid keypoint), or
        neither: the keyframe then takes part in detect_loop only.  kf_id must exceed every id stored."""
        ids, vals = _bow(bow)
        if desc is None:
            nd, pd, pc = 0, None, None
        else:
            desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
            class_id = np.ascontiguousarray(class_id, dtype=np.int32)
            if len(class_id) != len(desc):
                raise ValueError("one class_id per descriptor")
            nd = len(desc)
            # (an empty set of descriptors is still "with descriptors": a non-null pointer)
            pd = desc.ctypes.data_as(u8_p) if nd else C.cast(C.create_string_buffer(32), u8_p)
            pc = class_id.ctypes.data_as(i32_p) if nd else C.cast(C.create_string_buffer(4), i32_p)
        self.ctx.check(self.ctx.lib.ssx_kfdb_add(self.handle, int(kf_id), len(ids), ids.ctypes.data_as(i32_p), vals.ctypes.data_as(dbl_p), nd, pd, pc))

    def detect_loop(self, kf_id, bow, threshold, min_id_gap=20, with_scores=False):
        """-> (found, best_kf_id, best_score, n_scored[, scores]): DetectLoop for the current keyframe (kf_id, bow).  best_* are None
        when nothing was found; scores are the doubles of Vocabulary.score(bow, stored) for the n_scored eligible keyframes."""
        ids, vals = _bow(bow)
        found, best, score, n = C.c_int32(), C.c_int64(), C.c_float(), C.c_int32()
        cap = len(self) if with_scores else 0
        scores = np.zeros(max(cap, 1), np.float64)
        self.ctx.check(self.ctx.lib.ssx_kfdb_detect_loop(self.handle, int(kf_id), len(ids), ids.ctypes.data_as(i32_p), vals.ctypes.data_as(dbl_p),
                                                         int(min_id_gap), float(threshold), C.byref(found), C.byref(best), C.byref(score), cap,
                                                         scores.ctypes.data_as(dbl_p) if with_scores else None, C.byref(n)))
        out = (bool(found.value), best.value if found.value else None, np.float32(score.value) if found.value else None, n.value)
        return out + (scores[:n.value].copy(),) if with_scores else out

    def match_features(self, loop_kf_id, cur_desc, cur_class_id, cap=None):
        """-> (pairs [m, 2] int32 of (current class_id, loop class_id), unique and ascending; min_distance): MatchFeatures of the
        current keyframe against the stored loop_kf_id.  cap limits the pairs accepted (SsxError with status SSX_ERR_CAPACITY and
        .n_pairs when there are more)."""
        cur_desc = np.ascontiguousarray(cur_desc, dtype=np.uint8).reshape(-1, 32)
        cur_class_id = np.ascontiguousarray(cur_class_id, dtype=np.int32)
        if len(cur_class_id) != len(cur_desc):
            raise ValueError("one class_id per descriptor")
        if cap is None:
            cap = self.size()[2]                              # no more pairs than the loop keyframe has descriptors
        pairs = np.zeros((max(cap, 1), 2), np.int32)
        n, md = C.c_int32(), C.c_int32()
        st = self.ctx.lib.ssx_kfdb_match_features(self.handle, int(loop_kf_id), len(cur_desc), cur_desc.ctypes.data_as(u8_p),
                                                  cur_class_id.ctypes.data_as(i32_p), int(cap), pairs.ctypes.data_as(i32_p), C.byref(n), C.byref(md))
        try:
            self.ctx.check(st)
        except Exception as e:
            if st == SSX_ERR_CAPACITY:
                e.n_pairs = n.value
            raise
        return pairs[:n.value].copy(), md.value
