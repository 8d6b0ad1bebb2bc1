"""Loop closing on the device -- include/ssx.h.

KeyframeDatabase       ssx_kfdb_*: AddToKeyframeDatabase, DetectLoop and MatchFeatures (reference: src/ssvio/loopclosing.cpp:646-649,
                       :72-103, :105-145), and the per-keyframe step of LoopClosingThread as one call (process_keyframe / add_pending /
                       pending: ProcessNewKeyframe :596-634 + DetectLoop + MatchFeatures, the keyframe left on the device)
                       and relocalisation: relocalize_query (the candidates of a lost frame and its matches against each) and, behind
                       an accepted candidate, guided_search / project_match (map points projected with the pose just found and matched
                       in a window; the rule: tools/guided_model.py)
process_keyframe_batch ssx_kfdb_process_keyframe_batch: that step for one keyframe of each of several databases, one launch chain
pnp_ransac             ssx_pnp_ransac: the cv::solvePnPRansac call of ComputeCorrectPose (:205-206) under the contract of
                       tools/pnp_model.py
loop_pose_opt          ssx_loop_pose_opt: OptimizeCurrentPose (:245-351)
compute_correct_pose   ssx_loop_compute_pose: ComputeCorrectPose (:147-243) as a whole
loop_correct           ssx_loop_correct: the geometry of LoopCorrect (:353-594) -- the active window moved with the corrected current
                       keyframe, the pose-graph optimisation, every map point re-anchored -- under the contract of
                       tools/loop_correct_model.py"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import KP_DTYPE, SSX_ERR_CAPACITY, Context, OrbParams, dbl_p, i32_p, ptr, u8_p
from .ba import PoseGraphResult

i64_p = C.POINTER(C.c_int64)


class StepResult(C.Structure):
    """ssx_kfdb_step_result"""
    _fields_ = [("n_pyramid", C.c_int32), ("n_bow", C.c_int32), ("detect_ran", C.c_int32), ("n_scored", C.c_int32), ("found", C.c_int32),
                ("score", C.c_float), ("loop_kf_id", C.c_int64), ("n_pairs", C.c_int32), ("min_distance", C.c_int32)]


class StepJob(C.Structure):
    """ssx_kfdb_step_job"""
    _fields_ = [("db", C.c_void_p), ("kf_id", C.c_int64), ("img", C.c_void_p), ("stride", C.c_int32), ("n_features", C.c_int32),
                ("features", C.c_void_p), ("commit_pending", C.c_int32), ("pairs_cap", C.c_int32), ("pairs_out", i32_p),
                ("res", C.POINTER(StepResult)), ("status_out", i32_p)]


RELOC_MAX_CANDIDATES = 8                                       # SSX_RELOC_MAX_CANDIDATES


class RelocCandidate(C.Structure):
    """ssx_reloc_candidate"""
    _fields_ = [("kf_id", C.c_int64), ("score", C.c_float), ("row", C.c_int32), ("no_descriptors", C.c_int32), ("n_pairs", C.c_int32),
                ("min_distance", C.c_int32)]


class RelocQueryResult(C.Structure):
    """ssx_reloc_query_result"""
    _fields_ = [("n_pyramid", C.c_int32), ("n_bow", C.c_int32), ("n_scored", C.c_int32), ("n_candidates", C.c_int32),
                ("cand", RelocCandidate * RELOC_MAX_CANDIDATES)]


class RelocQueryJob(C.Structure):
    """ssx_reloc_query_job"""
    _fields_ = [("db", C.c_void_p), ("img", C.c_void_p), ("stride", C.c_int32), ("n_features", C.c_int32), ("features", C.c_void_p),
                ("commit_pending", C.c_int32), ("pairs_cap", C.c_int32), ("pairs_out", i32_p), ("res", C.POINTER(RelocQueryResult)),
                ("status_out", i32_p)]


def _bind(lib):
    if getattr(lib, "_kfdb_bound", False):
        return
    lib.ssx_kfdb_relocalize_query_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RelocQueryJob), C.c_int32, C.c_int32, C.POINTER(OrbParams), C.c_int32,
                                                    C.c_int32, C.c_float, C.c_float, C.c_int32]
    lib.ssx_kfdb_relocalize_query.argtypes = [C.c_void_p, C.c_void_p, u8_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(OrbParams), C.c_int32, C.c_void_p,
                                              C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, i32_p, C.POINTER(RelocQueryResult)]
    lib.ssx_kfdb_process_keyframe_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(StepJob), C.c_int32, C.c_int32, C.POINTER(OrbParams), C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_float, C.c_int32]
    if hasattr(lib, "ssx_kfdb_debug_last_batch"):
        lib.ssx_kfdb_debug_last_batch.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p]
    lib.ssx_kfdb_process_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, u8_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(OrbParams), C.c_int32,
                                              C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, i32_p, C.POINTER(StepResult)]
    lib.ssx_kfdb_add_pending.argtypes = [C.c_void_p]
    lib.ssx_kfdb_pending.argtypes = [C.c_void_p, i64_p, C.c_int32, C.c_void_p, u8_p, i32_p, i32_p, C.c_int32, i32_p, dbl_p, i32_p]
    if hasattr(lib, "ssx_kfdb_debug_last_step"):              # include/ssx_test_hooks.h: absent from a product build
        lib.ssx_kfdb_debug_last_step.argtypes = [C.c_void_p, i32_p, i32_p, i64_p, i64_p]
        lib.ssx_kfdb_debug_bow.argtypes = [C.c_void_p, u8_p, C.c_int32, C.c_int32, i32_p, dbl_p, i32_p]
    lib.ssx_kfdb_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    lib.ssx_kfdb_destroy.argtypes = [C.c_void_p]
    lib.ssx_kfdb_destroy.restype = None
    lib.ssx_kfdb_size.argtypes = [C.c_void_p, i32_p, i64_p, i64_p]
    lib.ssx_kfdb_add.argtypes = [C.c_void_p, C.c_int64, C.c_int32, i32_p, dbl_p, C.c_int32, u8_p, i32_p]
    lib.ssx_kfdb_detect_loop.argtypes = [C.c_void_p, C.c_int64, C.c_int32, i32_p, dbl_p, C.c_int32, C.c_float, i32_p, i64_p,
                                         C.POINTER(C.c_float), C.c_int32, dbl_p, i32_p]
    lib.ssx_kfdb_match_features.argtypes = [C.c_void_p, C.c_int64, C.c_int32, u8_p, i32_p, C.c_int32, i32_p, i32_p, i32_p]
    guided_tail = [C.c_int32, i64_p, i32_p, dbl_p, C.c_double, C.c_int32, C.c_int32, i32_p, i32_p, i32_p, i32_p, dbl_p, i32_p]
    lib.ssx_kfdb_project_match.argtypes = [C.c_void_p, dbl_p, dbl_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), u8_p, C.c_int32, u8_p, i32_p] + guided_tail
    lib.ssx_kfdb_guided_search.argtypes = [C.c_void_p, u8_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(OrbParams), C.c_int32, C.c_void_p, C.c_int32, u8_p,
                                           dbl_p, dbl_p] + guided_tail
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


    def process_keyframe(self, voc, kf_id, image, features, prm, threshold, pyramid_levels=8, min_db_size=0, min_id_gap=20, pairs_cap=None):
        """The per-keyframe step in one call: ProcessNewKeyframe (features [n] KP_DTYPE = the left features' kp_position_, replicated over
        pyramid_levels), DetectLoop when more than min_db_size keyframes are stored, MatchFeatures against the winner.  -> dict of
        ssx_kfdb_step_result's fields (loop_kf_id / score None when nothing was found) and pairs [n_pairs, 2].  The keyframe stays on the
        device as the pending one: add_pending() stores it, pending() downloads it.  SsxError with status SSX_ERR_CAPACITY carries .result
        (the first pairs_cap pairs in it) when pairs_cap is too small; the keyframe is pending all the same."""
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != np.uint8 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, dtype=np.uint8)
        features = np.ascontiguousarray(features, dtype=KP_DTYPE)
        if pairs_cap is None:
            pairs_cap = len(features) * int(pyramid_levels)       # a std::set of (current class_id, loop class_id): bounded by the stored
            pairs_cap = max(pairs_cap, self.size()[2])            # keyframe's descriptors
        pairs = np.zeros((max(pairs_cap, 1), 2), np.int32)
        r = StepResult()
        st = self.ctx.lib.ssx_kfdb_process_keyframe(self.handle, voc.handle, int(kf_id), ptr(image, u8_p), image.strides[0], image.shape[0], image.shape[1],
                                                    C.byref(prm), len(features), features.ctypes.data_as(C.c_void_p), int(pyramid_levels),
                                                    int(min_db_size), int(min_id_gap), float(threshold), int(pairs_cap), ptr(pairs, i32_p), C.byref(r))
        out = _step_dict(r, pairs, pairs_cap)
        try:
            self.ctx.check(st)
        except Exception as e:
            if st == SSX_ERR_CAPACITY:
                e.result = out
            raise
        return out

    def relocalize_query(self, voc, image, features, prm, max_candidates=4, threshold=0.0, ratio=0.75, pyramid_levels=8, pairs_cap=None):
        """The candidate query of relocalisation (ssx_kfdb_relocalize_query): the stored keyframes a frame that lost tracking resembles,
        best first, and its feature matches against each, in one call.  -> dict(n_pyramid, n_bow, n_scored, candidates = list of
        dict(kf_id, score float32, row, no_descriptors, n_pairs, min_distance, pairs [n_pairs, 2] as match_features)).  The database and
        its pending keyframe are not touched.  SsxError with status SSX_ERR_CAPACITY carries .result (the first pairs_cap pairs of each
        candidate in it) when pairs_cap is too small."""
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != np.uint8 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, dtype=np.uint8)
        features = np.ascontiguousarray(features, dtype=KP_DTYPE)
        if pairs_cap is None:                                     # a std::set of (current class_id, stored class_id): bounded by the stored
            pairs_cap = max(self.size()[2], 1)                    # keyframe's descriptors
        K = int(max_candidates)
        pairs = np.zeros((max(K, 1), max(pairs_cap, 1), 2), np.int32)
        r = RelocQueryResult()
        st = self.ctx.lib.ssx_kfdb_relocalize_query(self.handle, voc.handle, ptr(image, u8_p), image.strides[0], image.shape[0], image.shape[1], C.byref(prm),
                                                    len(features), features.ctypes.data_as(C.c_void_p), int(pyramid_levels), K, float(threshold), float(ratio),
                                                    int(pairs_cap), ptr(pairs, i32_p), C.byref(r))
        cands = [dict(kf_id=q.kf_id, score=np.float32(q.score), row=q.row, no_descriptors=bool(q.no_descriptors), n_pairs=q.n_pairs,
                      min_distance=q.min_distance, pairs=pairs[c, :min(q.n_pairs, pairs_cap)].copy())
                 for c, q in enumerate(r.cand[:max(0, min(r.n_candidates, RELOC_MAX_CANDIDATES))])]
        out = dict(n_pyramid=r.n_pyramid, n_bow=r.n_bow, n_scored=r.n_scored, candidates=cands)
        try:
            self.ctx.check(st)
        except Exception as e:
            if st == SSX_ERR_CAPACITY:
                e.result = out
            raise
        return out

    def project_match(self, K4, T_cw, rows, cols, feat_xy, cur_desc, cur_class_id, point_kf, point_cls, xyz, taken=None, radius=10.0, max_distance=50,
                      ratio_pct=90):
        """The guided search of relocalisation on a caller's arrays (ssx_kfdb_project_match; the rule: tools/guided_model.py): the points
        xyz [P, 3], each with the stored keyframe point_kf [P] and the class id point_cls [P] that hold its descriptors, projected with
        K4 = (fx, fy, cx, cy) and T_cw = 12 doubles [R|t] and matched in a window of `radius` pixels against the frame's features
        feat_xy [F, 2] (taken [F]: non-zero = no candidate) with descriptors cur_desc [n, 32] of features cur_class_id [n].
        -> dict(feat, d1, d2, status int32 [P], uv f64 [P, 2], n_matched)"""
        feat_xy = np.ascontiguousarray(feat_xy, dtype=np.float32).reshape(-1, 2)
        cur_desc = np.ascontiguousarray(cur_desc, dtype=np.uint8).reshape(-1, 32)
        cur_class_id = np.ascontiguousarray(cur_class_id, dtype=np.int32).reshape(-1)
        if len(cur_class_id) != len(cur_desc):
            raise ValueError("one class_id per descriptor")
        g = _GuidedCall(K4, T_cw, point_kf, point_cls, xyz, taken, len(feat_xy))
        nz = lambda arr, t: ptr(arr, t) if arr.size else None   # an empty array has no address worth passing
        self.ctx.check(self.ctx.lib.ssx_kfdb_project_match(self.handle, ptr(g.K4, dbl_p), ptr(g.T, dbl_p), int(rows), int(cols), len(feat_xy),
                                                           nz(feat_xy, C.POINTER(C.c_float)), g.taken_p, len(cur_desc), nz(cur_desc, u8_p), nz(cur_class_id, i32_p),
                                                           *g.tail(radius, max_distance, ratio_pct)))
        return g.result()

    def guided_search(self, image, features, prm, K4, T_cw, point_kf, point_cls, xyz, taken=None, radius=10.0, max_distance=50, ratio_pct=90,
                      pyramid_levels=8):
        """The guided search as the system runs it (ssx_kfdb_guided_search): the frame is described as relocalize_query describes it and
        the search reads its descriptors on the device.  features [n] KP_DTYPE, taken [n]; the rest and the result as project_match."""
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != np.uint8 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, dtype=np.uint8)
        features = np.ascontiguousarray(features, dtype=KP_DTYPE)
        g = _GuidedCall(K4, T_cw, point_kf, point_cls, xyz, taken, len(features))
        self.ctx.check(self.ctx.lib.ssx_kfdb_guided_search(self.handle, ptr(image, u8_p), image.strides[0], image.shape[0], image.shape[1], C.byref(prm),
                                                           len(features), features.ctypes.data_as(C.c_void_p), int(pyramid_levels), g.taken_p,
                                                           ptr(g.K4, dbl_p), ptr(g.T, dbl_p), *g.tail(radius, max_distance, ratio_pct)))
        return g.result()

    def add_pending(self):
        """AddToKeyframeDatabase for the keyframe of the last process_keyframe, device to device"""
        self.ctx.check(self.ctx.lib.ssx_kfdb_add_pending(self.handle))

    def pending(self):
        """-> dict(kf_id, keypoints [n] KP_DTYPE, desc [n, 32], class_id [n], bow = (ids, values)): the pending keyframe, downloaded"""
        lib = self.ctx.lib
        kf, n, nb = C.c_int64(), C.c_int32(), C.c_int32()
        self.ctx.check(lib.ssx_kfdb_pending(self.handle, C.byref(kf), 0, None, None, None, C.byref(n), 0, None, None, C.byref(nb)))
        kps = np.zeros(max(n.value, 1), KP_DTYPE); desc = np.zeros((max(n.value, 1), 32), np.uint8); cls = np.zeros(max(n.value, 1), np.int32)
        ids = np.zeros(max(nb.value, 1), np.int32); vals = np.zeros(max(nb.value, 1), np.float64)
        self.ctx.check(lib.ssx_kfdb_pending(self.handle, None, n.value, kps.ctypes.data_as(C.c_void_p), ptr(desc, u8_p), ptr(cls, i32_p), None,
                                            nb.value, ptr(ids, i32_p), ptr(vals, dbl_p), None))
        return dict(kf_id=kf.value, keypoints=kps[:n.value], desc=desc[:n.value], class_id=cls[:n.value], bow=(ids[:nb.value], vals[:nb.value]))

    def debug_last_step(self):
        """tests / tools hook -> dict(launches, syncs, bytes_up, bytes_down) of the last process_keyframe, relocalize_query or guided_search"""
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self.ctx.check(self.ctx.lib.ssx_kfdb_debug_last_step(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(launches=a.value, syncs=b.value, bytes_up=c.value, bytes_down=d.value)


class _GuidedCall:
    """the arguments project_match and guided_search share, as contiguous arrays, and their output arrays"""

    def __init__(self, K4, T_cw, point_kf, point_cls, xyz, taken, F):
        self.K4 = np.ascontiguousarray(K4, dtype=np.float64).reshape(-1)
        self.T = np.ascontiguousarray(T_cw, dtype=np.float64).reshape(-1)
        self.kf = np.ascontiguousarray(point_kf, dtype=np.int64).reshape(-1)
        self.cls = np.ascontiguousarray(point_cls, dtype=np.int32).reshape(-1)
        self.xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self.P = P = len(self.xyz)
        if self.K4.size != 4 or self.T.size != 12 or len(self.kf) != P or len(self.cls) != P:
            raise ValueError("K4 = (fx, fy, cx, cy), T_cw = 12 doubles [R|t], one keyframe and one class id per point")
        self.taken = None if taken is None else np.ascontiguousarray(taken, dtype=np.uint8).reshape(-1)
        if self.taken is not None and len(self.taken) != F:
            raise ValueError("one taken flag per feature")
        # (a non-null pointer for `taken set` even when there is no feature)
        self.taken_p = None if self.taken is None else (ptr(self.taken, u8_p) if F else C.cast(C.create_string_buffer(1), u8_p))
        self.feat, self.d1, self.d2, self.status = (np.zeros(max(P, 1), np.int32) for _ in range(4))
        self.uv = np.zeros((max(P, 1), 2), np.float64)
        self.n = C.c_int32()

    def tail(self, radius, max_distance, ratio_pct):
        return (self.P, ptr(self.kf, i64_p), ptr(self.cls, i32_p), ptr(self.xyz, dbl_p), float(radius), int(max_distance), int(ratio_pct),
                ptr(self.feat, i32_p), ptr(self.d1, i32_p), ptr(self.d2, i32_p), ptr(self.status, i32_p), ptr(self.uv, dbl_p), C.byref(self.n))

    def result(self):
        P = self.P
        return dict(feat=self.feat[:P], d1=self.d1[:P], d2=self.d2[:P], status=self.status[:P], uv=self.uv[:P], n_matched=self.n.value)


def _step_dict(r, pairs, pairs_cap):
    return dict(n_pyramid=r.n_pyramid, n_bow=r.n_bow, detect_ran=bool(r.detect_ran), n_scored=r.n_scored, found=bool(r.found),
                score=np.float32(r.score) if r.found else None, loop_kf_id=r.loop_kf_id if r.found else None, n_pairs=r.n_pairs,
                min_distance=r.min_distance, pairs=pairs[:min(r.n_pairs, pairs_cap)].copy())


def step_job_table(jobs):
    """the ssx_kfdb_step_job table of process_keyframe_batch's jobs -> (table, results, statuses, per job (image, features, pairs, pairs_cap),
    image shape); the arrays the table points into live as long as the returned objects"""
    n = len(jobs)
    table = (StepJob * max(n, 1))()
    res, status, keep = (StepResult * max(n, 1))(), (C.c_int32 * max(n, 1))(), []
    shape = None
    for j, q in enumerate(jobs):
        image = np.asarray(q["image"])
        if image.ndim != 2 or image.dtype != np.uint8 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, dtype=np.uint8)
        if shape is None:
            shape = image.shape
        elif image.shape != shape:
            raise ValueError("the images of a call share one shape")
        features = np.ascontiguousarray(q["features"], dtype=KP_DTYPE)
        cap = q.get("pairs_cap")
        if cap is None:                                           # a std::set of (current class_id, loop class_id): bounded by the winner's
            cap = 65535                                           # descriptors, and a keyframe has no more than 65535
        pairs = np.zeros((max(cap, 1), 2), np.int32)
        keep.append((image, features, pairs, int(cap)))
        table[j] = StepJob(q["db"].handle, int(q["kf_id"]), image.ctypes.data, image.strides[0], len(features), features.ctypes.data,
                           1 if q.get("commit_pending") else 0, int(cap), ptr(pairs, i32_p), C.pointer(res[j]), C.cast(C.byref(status, 4 * j), i32_p))
    return table, res, status, keep, shape if shape is not None else (0, 0)


def process_keyframe_batch(voc, jobs, prm, threshold, pyramid_levels=8, min_db_size=0, min_id_gap=20, images_on_device=False):
    """The per-keyframe step of several databases of voc's context in ONE call (ssx_kfdb_process_keyframe_batch).  jobs = dicts of
    db (KeyframeDatabase), kf_id, image, features and optionally commit_pending (add_pending() first, inside the call) and pairs_cap;
    the images share one shape and row stride.  -> one dict per job in process_keyframe's form plus status, the job's ssx_status.
    SsxError carries .results (that list) when the call reports a job's status; a call that was rejected has touched nothing.
    images_on_device: the image buffers are pinned or device memory and are read where they lie."""
    ctx = voc.ctx
    _bind(ctx.lib)
    n = len(jobs)
    table, res, status, keep, (rows, cols) = step_job_table(jobs)
    st = ctx.lib.ssx_kfdb_process_keyframe_batch(voc.handle, n, table, rows, cols, C.byref(prm), int(pyramid_levels), int(min_db_size), int(min_id_gap),
                                                 float(threshold), 1 if images_on_device else 0)
    out = [dict(_step_dict(res[j], keep[j][2], keep[j][3]), status=status[j]) for j in range(n)]
    try:
        ctx.check(st)
    except Exception as e:
        e.results = out
        raise
    return out


def _reloc_dict(r, pairs, pairs_cap):
    cands = [dict(kf_id=q.kf_id, score=np.float32(q.score), row=q.row, no_descriptors=bool(q.no_descriptors), n_pairs=q.n_pairs,
                  min_distance=q.min_distance, pairs=pairs[c, :min(q.n_pairs, pairs_cap)].copy())
             for c, q in enumerate(r.cand[:max(0, min(r.n_candidates, RELOC_MAX_CANDIDATES))])]
    return dict(n_pyramid=r.n_pyramid, n_bow=r.n_bow, n_scored=r.n_scored, candidates=cands)


def relocalize_query_batch(voc, jobs, prm, max_candidates=4, threshold=0.0, ratio=0.75, pyramid_levels=8, images_on_device=False):
    """The candidate query of several databases of voc's context in ONE call (ssx_kfdb_relocalize_query_batch).  jobs = dicts of
    db (KeyframeDatabase), image, features and optionally commit_pending (add_pending() first, inside the call) and pairs_cap; the
    images share one shape and row stride.  -> one dict per job in relocalize_query's form plus status, the job's ssx_status.
    SsxError carries .results (that list) when the call reports a job's status; a call that was rejected has touched nothing."""
    ctx = voc.ctx
    _bind(ctx.lib)
    n, K = len(jobs), int(max_candidates)
    table = (RelocQueryJob * max(n, 1))()
    res, status, keep = (RelocQueryResult * max(n, 1))(), (C.c_int32 * max(n, 1))(), []
    shape = None
    for j, q in enumerate(jobs):
        image = np.asarray(q["image"])
        if image.ndim != 2 or image.dtype != np.uint8 or image.strides[1] != 1:
            image = np.ascontiguousarray(image, dtype=np.uint8)
        if shape is None:
            shape = image.shape
        elif image.shape != shape:
            raise ValueError("the images of a call share one shape")
        features = np.ascontiguousarray(q["features"], dtype=KP_DTYPE)
        cap = q.get("pairs_cap")
        if cap is None:                                           # bounded by the stored keyframes' descriptors and by those of the
            cap = q["db"].size()[2]                               # keyframe the job commits (no more than its pyramid keypoints)
            if q.get("commit_pending"):
                cap += 65535
        cap = max(int(cap), 0)
        pairs = np.zeros((max(K, 1), max(cap, 1), 2), np.int32)
        keep.append((image, features, pairs, cap))
        table[j] = RelocQueryJob(q["db"].handle, image.ctypes.data, image.strides[0], len(features), features.ctypes.data,
                                 1 if q.get("commit_pending") else 0, cap, ptr(pairs, i32_p), C.pointer(res[j]), C.cast(C.byref(status, 4 * j), i32_p))
    rows, cols = shape if shape is not None else (0, 0)
    st = ctx.lib.ssx_kfdb_relocalize_query_batch(voc.handle, n, table, rows, cols, C.byref(prm), int(pyramid_levels), K, float(threshold), float(ratio),
                                                 1 if images_on_device else 0)
    out = [dict(_reloc_dict(res[j], keep[j][2], keep[j][3]), status=status[j]) for j in range(n)]
    try:
        ctx.check(st)
    except Exception as e:
        e.results = out
        raise
    return out


def debug_last_batch(ctx):
    """tests / tools hook -> dict(launches, syncs, bytes_up, bytes_down) of the context's last process_keyframe_batch or relocalize_query_batch"""
    _bind(ctx.lib)
    a, b, c, d = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
    ctx.check(ctx.lib.ssx_kfdb_debug_last_batch(ctx.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return dict(launches=a.value, syncs=b.value, bytes_up=c.value, bytes_down=d.value)


def debug_bow(voc, desc):
    """tests hook -> (ids, values): the BowVector of desc [n, 32] as the step's device kernels assemble it"""
    _bind(voc.ctx.lib)
    desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
    n = len(desc)
    ids = np.zeros(max(n, 1), np.int32); vals = np.zeros(max(n, 1), np.float64); m = C.c_int32()
    voc.ctx.check(voc.ctx.lib.ssx_kfdb_debug_bow(voc.handle, ptr(desc, u8_p), n, max(n, 1), ptr(ids, i32_p), ptr(vals, dbl_p), C.byref(m)))
    return ids[:m.value].copy(), vals[:m.value].copy()


# ---- the pose correction: ComputeCorrectPose / OptimizeCurrentPose ---------------------------------------------------------------
LOOP_OK, LOOP_FEW_MAP_POINTS, LOOP_NO_POSE, LOOP_FEW_INLIERS = 0, 1, 2, 3      # ssx_loop_verdict
PNP_MAX_ITERS = 4096                                                           # SSX_PNP_MAX_ITERS


class LoopPoseResult(C.Structure):
    """ssx_loop_pose_result"""
    _fields_ = [("verdict", C.c_int32), ("n_with_point", C.c_int32), ("n_ransac_inliers", C.c_int32), ("best_hypothesis", C.c_int32),
                ("n_inliers", C.c_int32), ("need_correct", C.c_int32), ("error", C.c_double), ("corrected_pose", C.c_double * 7),
                ("relative_to_loop", C.c_double * 7)]


def _bind_pose(lib):
    if getattr(lib, "_loop_pose_bound", False):
        return
    lib.ssx_pnp_ransac.argtypes = [C.c_void_p, dbl_p, C.c_int32, dbl_p, dbl_p, C.c_int32, C.c_double, C.c_uint32, dbl_p, u8_p, i32_p, i32_p, i32_p]
    lib.ssx_loop_pose_opt.argtypes = [C.c_void_p, dbl_p, dbl_p, C.c_int32, dbl_p, dbl_p, C.c_double, C.c_double, u8_p, i32_p]
    lib.ssx_loop_compute_pose.argtypes = [C.c_void_p, C.c_int32, dbl_p, u8_p, dbl_p, dbl_p, dbl_p, dbl_p, C.c_int32, C.c_uint32, u8_p,
                                          C.POINTER(LoopPoseResult)]
    lib.ssx_pnp_pose_batch.argtypes = [C.c_void_p, dbl_p, C.c_int32, C.POINTER(PnpPoseJob), C.c_int32, C.c_double, C.c_double, C.c_double]
    lib._loop_pose_bound = True


def _f64(a, cols):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, cols)


def pnp_ransac(ctx: Context, K, xyz, uv, max_iters=100, reproj_px=5.991, seed=0):
    """-> dict(found, pose (qx qy qz qw tx ty tz), inliers uint8 [M], n_inliers, best = 4 h + s of the winner or -1).  All
    max_iters hypotheses are scored; the same arguments give the same bytes."""
    _bind_pose(ctx.lib)
    K = np.ascontiguousarray(K, dtype=np.float64)
    xyz, uv = _f64(xyz, 3), _f64(uv, 2)
    if len(xyz) != len(uv) or K.size != 4:
        raise ValueError("one pixel per point, K = (fx, fy, cx, cy)")
    M = len(xyz)
    pose, inl = np.zeros(7), np.zeros(max(M, 1), np.uint8)
    n, best, found = C.c_int32(), C.c_int32(), C.c_int32()
    ctx.check(ctx.lib.ssx_pnp_ransac(ctx.handle, ptr(K, dbl_p), M, ptr(xyz, dbl_p), ptr(uv, dbl_p), int(max_iters), float(reproj_px),
                                     int(seed) & 0xFFFFFFFF, ptr(pose, dbl_p), ptr(inl, u8_p), C.byref(n), C.byref(best), C.byref(found)))
    return dict(found=bool(found.value), pose=pose, inliers=inl[:M], n_inliers=n.value, best=best.value)


def loop_pose_opt(ctx: Context, pose, K, xyz, uv, chi2_th=5.991, huber_delta=1.0):
    """OptimizeCurrentPose from `pose` over all pairs -> dict(pose, inliers uint8 [M], n_inliers)"""
    _bind_pose(ctx.lib)
    pose = np.ascontiguousarray(pose, dtype=np.float64).copy()
    K = np.ascontiguousarray(K, dtype=np.float64)
    xyz, uv = _f64(xyz, 3), _f64(uv, 2)
    if len(xyz) != len(uv) or K.size != 4 or pose.size != 7:
        raise ValueError("one pixel per point, K = (fx, fy, cx, cy), pose = 7 doubles")
    M = len(xyz)
    inl = np.zeros(max(M, 1), np.uint8)
    n = C.c_int32()
    ctx.check(ctx.lib.ssx_loop_pose_opt(ctx.handle, ptr(pose, dbl_p), ptr(K, dbl_p), M, ptr(xyz, dbl_p), ptr(uv, dbl_p), float(chi2_th),
                                        float(huber_delta), ptr(inl, u8_p), C.byref(n)))
    return dict(pose=pose, inliers=inl[:M], n_inliers=n.value)


PNP_BATCH_MAX = 64                                                             # SSX_PNP_BATCH_MAX


class PnpPoseJob(C.Structure):
    """ssx_pnp_pose_job"""
    _fields_ = [("M", C.c_int32), ("xyz", dbl_p), ("uv", dbl_p), ("seed", C.c_uint32), ("pose_out", C.c_double * 7), ("inlier_out", u8_p),
                ("found", C.c_int32), ("n_ransac_inliers", C.c_int32), ("best_hypothesis", C.c_int32), ("n_inliers", C.c_int32)]


def pnp_pose_batch(ctx: Context, K, jobs, max_iters=100, reproj_px=5.991, chi2_th=5.991, huber_delta=1.0):
    """ssx_pnp_pose_batch: per job = dict(xyz [M, 3], uv [M, 2], seed) the bits of pnp_ransac and, where it found a pose, loop_pose_opt from
    it, all jobs in one call.  -> one dict(found, pose, inliers uint8 [M], n_inliers, n_ransac_inliers, best) per job; pose, inliers and
    n_inliers are the refinement's (the identity, zeros and 0 where nothing was found)."""
    _bind_pose(ctx.lib)
    K = np.ascontiguousarray(K, dtype=np.float64)
    if K.size != 4:
        raise ValueError("K = (fx, fy, cx, cy)")
    n = len(jobs)
    table = (PnpPoseJob * max(n, 1))()
    keep = []
    for j, q in enumerate(jobs):
        xyz, uv = _f64(q["xyz"], 3), _f64(q["uv"], 2)
        if len(xyz) != len(uv):
            raise ValueError("one pixel per point")
        inl = np.zeros(max(len(xyz), 1), np.uint8)
        keep.append((xyz, uv, inl))
        table[j].M, table[j].xyz, table[j].uv, table[j].seed = len(xyz), ptr(xyz, dbl_p), ptr(uv, dbl_p), int(q.get("seed", 0)) & 0xFFFFFFFF
        table[j].inlier_out = ptr(inl, u8_p)
    ctx.check(ctx.lib.ssx_pnp_pose_batch(ctx.handle, ptr(K, dbl_p), n, table, int(max_iters), float(reproj_px), float(chi2_th), float(huber_delta)))
    return [dict(found=bool(table[j].found), pose=np.array(table[j].pose_out), inliers=keep[j][2][:len(keep[j][0])], n_inliers=table[j].n_inliers,
                 n_ransac_inliers=table[j].n_ransac_inliers, best=table[j].best_hypothesis) for j in range(n)]


def compute_correct_pose(ctx: Context, loop_xyz, has_point, cur_uv, T_cur, T_loop, K, max_iters=100, seed=0):
    """ComputeCorrectPose for the pairs of KeyframeDatabase.match_features: loop_xyz [n, 3] the loop keyframe's map point of each pair
    (any value where has_point [n] is 0), cur_uv [n, 2] the current keyframe's pixel.  -> dict(verdict (LOOP_*), ok, kept uint8 [n],
    corrected_pose, error, need_correct, relative_to_loop, n_with_point, n_ransac_inliers, n_inliers, best)"""
    _bind_pose(ctx.lib)
    K = np.ascontiguousarray(K, dtype=np.float64)
    xyz, uv = _f64(loop_xyz, 3), _f64(cur_uv, 2)
    has = np.ascontiguousarray(has_point, dtype=np.uint8).reshape(-1)
    T_cur, T_loop = np.ascontiguousarray(T_cur, dtype=np.float64), np.ascontiguousarray(T_loop, dtype=np.float64)
    if not (len(xyz) == len(uv) == len(has)) or K.size != 4 or T_cur.size != 7 or T_loop.size != 7:
        raise ValueError("one map point, flag and pixel per pair; K = (fx, fy, cx, cy); poses = 7 doubles")
    n = len(has)
    kept = np.zeros(max(n, 1), np.uint8)
    r = LoopPoseResult()
    ctx.check(ctx.lib.ssx_loop_compute_pose(ctx.handle, n, ptr(xyz, dbl_p), ptr(has, u8_p), ptr(uv, dbl_p), ptr(T_cur, dbl_p), ptr(T_loop, dbl_p),
                                            ptr(K, dbl_p), int(max_iters), int(seed) & 0xFFFFFFFF, ptr(kept, u8_p), C.byref(r)))
    return dict(verdict=r.verdict, ok=r.verdict == LOOP_OK, kept=kept[:n], corrected_pose=np.array(r.corrected_pose), error=r.error,
                need_correct=bool(r.need_correct), relative_to_loop=np.array(r.relative_to_loop), n_with_point=r.n_with_point,
                n_ransac_inliers=r.n_ransac_inliers, n_inliers=r.n_inliers, best=r.best_hypothesis)


class LoopCorrectProblem(C.Structure):
    """ssx_loop_correct_problem"""
    _fields_ = [("n_keyframes", C.c_int32), ("n_edges", C.c_int32), ("n_points", C.c_int32), ("cur_kf", C.c_int32), ("loop_kf", C.c_int32),
                ("initial_kf", C.c_int32), ("keep_kf", C.c_int32), ("poses", dbl_p), ("kf_active", u8_p), ("corrected_pose", dbl_p),
                ("edge_i", i32_p), ("edge_j", i32_p), ("edge_meas", dbl_p), ("points", dbl_p), ("point_anchor", i32_p), ("point_active", u8_p),
                ("stage1_poses_out", dbl_p), ("edge_err_out", dbl_p), ("stats_cap", C.c_int32), ("stats_chi2", dbl_p), ("stats_lambda", dbl_p),
                ("stats_trials", i32_p)]


class LoopCorrectResult(C.Structure):
    """ssx_loop_correct_result"""
    _fields_ = [("pg", PoseGraphResult), ("n_active_kf", C.c_int32), ("n_active_points_moved", C.c_int32), ("n_other_points_moved", C.c_int32),
                ("n_points_skipped", C.c_int32)]


def loop_correct_struct(pr, iters=20):
    """the ctypes problem for pr (see loop_correct) -> (struct, arrays): arrays holds every buffer the struct points into, the in/out ones
    under "poses" and "points", the outputs under "stage1_poses", "edge_err", "chi2", "lambdas", "trials" """
    a = dict(poses=np.ascontiguousarray(pr["poses"], dtype=np.float64).reshape(-1, 7).copy(),
             kf_active=np.ascontiguousarray(pr["kf_active"], dtype=np.uint8).reshape(-1),
             corrected=np.ascontiguousarray(pr["corrected_pose"], dtype=np.float64).reshape(-1),
             ei=np.ascontiguousarray(pr["ei"], dtype=np.int32).reshape(-1), ej=np.ascontiguousarray(pr["ej"], dtype=np.int32).reshape(-1),
             meas=np.ascontiguousarray(pr["meas"], dtype=np.float64).reshape(-1, 7),
             points=np.ascontiguousarray(pr["points"], dtype=np.float64).reshape(-1, 3).copy(),
             point_anchor=np.ascontiguousarray(pr["point_anchor"], dtype=np.int32).reshape(-1),
             point_active=np.ascontiguousarray(pr["point_active"], dtype=np.uint8).reshape(-1))
    P, E, N = len(a["poses"]), len(a["ei"]), len(a["points"])
    if not (len(a["kf_active"]) == P and a["corrected"].size == 7 and len(a["ej"]) == E and len(a["meas"]) == E and
            len(a["point_anchor"]) == N and len(a["point_active"]) == N):
        raise ValueError("one flag per keyframe, 7 doubles of corrected pose, one (i, j, measurement) per edge, one anchor and flag per point")
    cap = max(int(iters), 0) + 2
    a.update(stage1_poses=np.zeros((P, 7)), edge_err=np.zeros((max(E, 1), 6)), chi2=np.zeros(cap), lambdas=np.zeros(cap), trials=np.zeros(cap, np.int32))
    nz = lambda arr, t: ptr(arr, t) if arr.size else None       # an empty array has no address worth passing
    prob = LoopCorrectProblem(P, E, N, int(pr["cur_kf"]), int(pr["loop_kf"]), int(pr.get("initial_kf", -1)), int(pr.get("keep_kf", -1)),
                              ptr(a["poses"], dbl_p), ptr(a["kf_active"], u8_p), ptr(a["corrected"], dbl_p), nz(a["ei"], i32_p), nz(a["ej"], i32_p),
                              nz(a["meas"], dbl_p), nz(a["points"], dbl_p), nz(a["point_anchor"], i32_p), nz(a["point_active"], u8_p),
                              ptr(a["stage1_poses"], dbl_p), ptr(a["edge_err"], dbl_p), cap, ptr(a["chi2"], dbl_p), ptr(a["lambdas"], dbl_p),
                              ptr(a["trials"], i32_p))
    return prob, a


def loop_correct(ctx: Context, pr, iters=20):
    """The geometry of LoopClosing::LoopCorrect (:353-594) on a flat problem:
    pr = dict(poses [P, 7] T_cw, kf_active [P], cur_kf, loop_kf, initial_kf (-1: none), keep_kf (-1: none), corrected_pose [7],
              ei [E], ej [E], meas [E, 7], points [N, 3], point_anchor [N] (-1: leave alone), point_active [N]).
    -> dict(poses, points, stage1_poses, edge_err, n_iters, chi2, lambdas, trials, chi2_initial, chi2_final, n_active_kf,
            n_active_points_moved, n_other_points_moved, n_points_skipped); the inputs are not modified."""
    prob, a = loop_correct_struct(pr, iters)
    res = LoopCorrectResult()
    ctx.lib.ssx_loop_correct.restype = C.c_int
    ctx.lib.ssx_loop_correct.argtypes = [C.c_void_p, C.POINTER(LoopCorrectProblem), C.c_int32, C.POINTER(LoopCorrectResult)]
    ctx.check(ctx.lib.ssx_loop_correct(ctx.handle, C.byref(prob), int(iters), C.byref(res)))
    k, E = res.pg.stats_n, len(a["ei"])
    return dict(poses=a["poses"], points=a["points"], stage1_poses=a["stage1_poses"], edge_err=a["edge_err"][:E], n_iters=res.pg.n_iters,
                chi2=a["chi2"][:k].copy(), lambdas=a["lambdas"][:k].copy(), trials=a["trials"][:k].copy(), chi2_initial=res.pg.chi2_initial,
                chi2_final=res.pg.chi2_final, n_active_kf=res.n_active_kf, n_active_points_moved=res.n_active_points_moved,
                n_other_points_moved=res.n_other_points_moved, n_points_skipped=res.n_points_skipped)
