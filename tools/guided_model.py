"""The contract of the guided search of relocalisation, in plain numpy (the style of tools/reloc_model.py and tools/pnp_model.py): the
second step behind an accepted candidate -- its local map projected into the frame with the pose just found, descriptors matched in a
small window round each projection (ssx_kfdb_project_match / ssx_kfdb_guided_search, csrc/loop_guided.inc: k_kfdb_project,
k_kfdb_claim), and the host's rules round it (LoopClosing::Relocalize).

search_by_projection  The rule the kernels follow operation by operation.  Per point, all in f64, every operation rounded on its own,
                      left to right as written:
                        xc = ((R00 X + R01 Y) + R02 Z) + t0, likewise yc, zc          non-finite or zc <= 0: BEHIND
                        u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy                 not 0 <= u < cols and 0 <= v < rows: OUTSIDE
                      The point's descriptors are ALL stored descriptors of keyframe point_kf whose class id is point_cls; an unknown
                      keyframe, one stored without descriptors or none of that class: NO_DESCRIPTOR (no error: the keyframe may not
                      have reached the database yet).  Feature i is a candidate iff it is not taken, |double(x_i) - u| <= radius and
                      |double(y_i) - v| <= radius (a square, edges inclusive) and it has a frame descriptor; none: NO_FEATURE.
                      d(p, i) = the least popcount(a xor b) over the point's descriptors a and feature i's descriptors b.  The best
                      feature has the lowest d, then the lowest index; the second is the lowest d over all OTHER candidates.  Accepted
                      iff d1 <= max_distance (else DISTANCE) and there is no second or 100 d1 < ratio_pct d2 in integers (else RATIO).
                      A feature goes to one point: of the accepted points that claim it the lowest d1 wins, then the lowest point
                      index; the losers are CLAIMED and do not fall back to their second.
refine_accept         The guided result replaces the first one iff the second refinement found a pose and kept at least as many
                      inliers as the first had.
gather_points         The host's gather: the accepted keyframe, then its neighbours in the map's id order by increasing distance, the
                      lower id first; of each, in feature order, every feature whose map point is alive, no outlier, not matched by the
                      first pass and not gathered yet."""
import numpy as np

MATCHED, BEHIND, OUTSIDE, NO_DESCRIPTOR, NO_FEATURE, DISTANCE, RATIO, CLAIMED = range(8)      # ssx_guided_status
STATUS_NAMES = ("MATCHED", "BEHIND", "OUTSIDE", "NO_DESCRIPTOR", "NO_FEATURE", "DISTANCE", "RATIO", "CLAIMED")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """[na, 32] x [nb, 32] uint8 -> [na, nb] int32"""
    return _POP[a[:, None, :] ^ b[None, :, :]].sum(axis=2, dtype=np.int32)


def project(K4, T_cw12, xyz):
    """-> (behind bool [P], uv f64 [P, 2]): uv is zero where behind"""
    K4 = np.ascontiguousarray(K4, dtype=np.float64).reshape(4)
    T = np.ascontiguousarray(T_cw12, dtype=np.float64).reshape(3, 4)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    X, Y, Z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        c = [((T[r, 0] * X + T[r, 1] * Y) + T[r, 2] * Z) + T[r, 3] for r in range(3)]
        behind = ~(np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])) | ~(c[2] > 0)
        zc = np.where(behind, 1.0, c[2])
        u = K4[0] * (c[0] / zc) + K4[2]
        v = K4[1] * (c[1] / zc) + K4[3]
    uv = np.stack([np.where(behind, 0.0, u), np.where(behind, 0.0, v)], axis=1)
    return behind, uv


def search_by_projection(db, K4, T_cw12, rows, cols, feat_xy, taken, cur_desc, cur_cls, point_kf, point_cls, xyz, radius, max_distance,
                         ratio_pct):
    """db: {kf_id: (desc uint8 [n, 32], class_id int32 [n])}, or None for a keyframe stored without descriptors.
    -> dict(feat, d1, d2, status int32 [P], uv f64 [P, 2], n_matched)"""
    feat_xy = np.ascontiguousarray(feat_xy, dtype=np.float32).reshape(-1, 2)
    F = len(feat_xy)
    taken = np.zeros(F, np.uint8) if taken is None else np.ascontiguousarray(taken, dtype=np.uint8).reshape(-1)
    cur_desc = np.ascontiguousarray(cur_desc, dtype=np.uint8).reshape(-1, 32)
    cur_cls = np.ascontiguousarray(cur_cls, dtype=np.int32).reshape(-1)
    point_kf = np.ascontiguousarray(point_kf, dtype=np.int64).reshape(-1)
    point_cls = np.ascontiguousarray(point_cls, dtype=np.int32).reshape(-1)
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    P = len(xyz)
    radius, max_distance, ratio_pct = float(radius), int(max_distance), int(ratio_pct)
    if len(taken) != F or len(cur_cls) != len(cur_desc) or len(point_kf) != P or len(point_cls) != P:
        raise ValueError("one flag per feature, one class id per descriptor, one keyframe and class per point")
    if len(cur_cls) and (cur_cls.min() < 0 or cur_cls.max() >= F):
        raise ValueError("a class id outside [0, F)")
    if not (np.isfinite(radius) and radius >= 0) or not 0 <= max_distance <= 256 or not 0 <= ratio_pct <= 100:
        raise ValueError("radius negative or not finite, max_distance outside [0, 256] or ratio_pct outside [0, 100]")
    behind, uv = project(K4, T_cw12, xyz)
    feat = np.full(P, -1, np.int32); d1 = np.full(P, -1, np.int32); d2 = np.full(P, -1, np.int32)
    status = np.zeros(P, np.int32)
    fx, fy = feat_xy[:, 0].astype(np.float64), feat_xy[:, 1].astype(np.float64)
    described = np.zeros(F, bool)
    described[cur_cls] = True
    best = np.full(P, -1, np.int64)
    for p in range(P):
        if behind[p]:
            status[p] = BEHIND
            continue
        u, v = uv[p]
        if not (0 <= u < cols and 0 <= v < rows):
            status[p] = OUTSIDE
            continue
        kf = db.get(int(point_kf[p]))
        mine = None if kf is None else np.ascontiguousarray(kf[0], dtype=np.uint8).reshape(-1, 32)[np.asarray(kf[1]).reshape(-1) == point_cls[p]]
        if mine is None or len(mine) == 0:
            status[p] = NO_DESCRIPTOR
            continue
        cand = (taken == 0) & (np.abs(fx - u) <= radius) & (np.abs(fy - v) <= radius) & described
        if not cand.any():
            status[p] = NO_FEATURE
            continue
        use = cand[cur_cls]
        dist = hamming(mine, cur_desc[use]).min(axis=0)         # per kept frame descriptor: the nearest of the point's
        d = np.full(F, 1 << 30, np.int64)
        np.minimum.at(d, cur_cls[use], dist)
        order = np.lexsort((np.arange(F), d))                   # d ascending, then the feature index
        b = int(order[0])
        d1[p] = d[b]
        if cand.sum() > 1:
            d2[p] = d[order[1]]
        if d1[p] > max_distance:
            status[p] = DISTANCE
        elif d2[p] >= 0 and not 100 * int(d1[p]) < ratio_pct * int(d2[p]):
            status[p] = RATIO
        else:
            best[p] = b                                         # accepted: it claims its feature
    for f in np.unique(best[best >= 0]):
        claim = np.nonzero(best == f)[0]
        win = claim[np.lexsort((claim, d1[claim]))[0]]          # the lowest d1, then the lowest point
        status[claim] = CLAIMED
        status[win] = MATCHED
        feat[win] = f
    return dict(feat=feat, d1=d1, d2=d2, status=status, uv=uv, n_matched=int((status == MATCHED).sum() if P else 0))


def refine_accept(n_before, n_after, found=True):
    """does the second refinement's result (found: it has a pose; n_after inliers) replace the first pass's (n_before inliers)?"""
    return bool(found) and int(n_after) >= int(n_before)


def gather_points(kf_ids, accepted, neighbours, features, first_points):
    """kf_ids: the map's keyframe ids in its order (ascending); accepted: the accepted candidate's id; features[kf_id]: per feature of
    that keyframe, in feature order, (point id, alive, outlier) or None where the feature has no map point; first_points: the ids of the
    map points the first pass matched.  -> [(point id, keyframe id, feature index)] in the order the host gathers them"""
    kf_ids = [int(k) for k in kf_ids]
    at = kf_ids.index(int(accepted))
    order = [at]
    for step in range(1, int(neighbours) + 1):                  # by increasing distance in the id order, the lower id first
        for i in (at - step, at + step):
            if 0 <= i < len(kf_ids):
                order.append(i)
    seen, out = set(int(p) for p in first_points), []
    for i in order:
        for f, entry in enumerate(features[kf_ids[i]]):
            if entry is None:
                continue
            pid, alive, outlier = entry
            if not alive or outlier or int(pid) in seen:
                continue
            seen.add(int(pid))
            out.append((int(pid), kf_ids[i], f))
    return out
