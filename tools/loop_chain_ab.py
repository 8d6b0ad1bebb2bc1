"""Keyframe database A/B: two builds of the library must return the same bytes and issue the same launches, synchronisations and bytes.

    SSX_LIB=<library> python tools/loop_chain_ab.py out.json     digests and counts of one library (GPU; a fresh process per library)
    python tools/loop_chain_ab.py --compare a.json b.json        exit 1 unless every digest and every count is equal
    python tools/loop_chain_ab.py --times LABEL=FILE ...         (no GPU) the medians of tools/loop_db_time.py, tools/loop_batch_time.py and
        tools/reloc_time.py outputs, FILEs of the same label being runs of one library: min / median / max per figure, and where the
        second label's median lies in the first's min-max (exit 1 if above it)

Digested (sha256 of the bytes of every output), on the drive and scenes of tests/test_loop_keyframe_gpu.py and the twins of
tests/test_reloc_query_gpu.py:
  drive/<i>/...   database A by ssx_kfdb_add, ssx_kfdb_detect_loop with scores and ssx_kfdb_match_features, database B by
                  ssx_kfdb_process_keyframe + ssx_kfdb_pending + ssx_kfdb_add_pending; at the end every stored keyframe of both matched
                  against the last one and scored against one query
  batch<S>/...    ssx_kfdb_process_keyframe_batch with S = 1 and 5 streams over the drive's places (stream s starts s places later), each
                  job committing its previous pending keyframe inside the call unless a loop was confirmed; every job's pending keyframe
  reloc/...       ssx_kfdb_relocalize_query on every twin with K = 1, 4, 8
  bow/...         ssx_kfdb_debug_bow at BOW_SIZES, random and tiled descriptors
Recorded as they are: (launches, syncs, bytes_up, bytes_down) of every step, batch and query (ssx_kfdb_debug_last_step / _last_batch).
ssx_kfdb_detect_loop, ssx_kfdb_match_features and ssx_kfdb_debug_bow report none."""
import hashlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(r):
    """sha256 over a dict / tuple / list / array / scalar / None, keys in order"""
    import numpy as np
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, dict):
            for k in sorted(v):
                h.update(str(k).encode()); feed(v[k])
        elif isinstance(v, (tuple, list)):
            h.update(b"[%d]" % len(v))
            for x in v:
                feed(x)
        elif isinstance(v, (np.ndarray, np.generic)):
            a = np.ascontiguousarray(v)
            h.update(str((a.dtype.str, a.shape)).encode()); h.update(a.tobytes())
        else:
            h.update(repr(v).encode())
    feed(r)
    return h.hexdigest()


def outputs():
    import numpy as np
    import ssvio_amd
    import test_loop_keyframe_gpu as kf
    import test_reloc_query_gpu as rq
    from oracle import pyoracle as po
    from ssvio_amd import loop as sloop
    from ssvio_amd import orb as sorb
    from ssvio_amd import voc as svoc
    from tools.synth import make_stereo_pair, make_vocabulary
    po.build()
    dig, counts = {}, {}
    places = list(range(6)) + [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11, 0, 12, 6, 13, 7, 1, 14, 8, 9, 15, 2, 10]      # the drive of test_loop_keyframe_gpu.py
    with ssvio_amd.Context(0) as ctx:
        voc = make_vocabulary(k=10, L=3)
        V = svoc.Vocabulary.from_arrays(ctx, 10, 3, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
        ex = sorb.ORBextractor(ctx, nfeatures=2000)
        scenes = {s: kf.small_scene(po, s) for s in sorted(set(places))}
        step = dict(pyramid_levels=kf.LEVELS, min_db_size=2, min_id_gap=3)

        # ---- the drive: five calls against the step ----
        A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=4), sloop.KeyframeDatabase(ctx, keyframes_hint=4)
        frames = []
        for i, place in enumerate(places):
            img, feats = scenes[place]
            kf_id = 2 * i + 1
            ra, frame = kf.five_calls(A, V, ex, kf_id, img, feats, min_db_size=2, min_id_gap=3)
            dig[f"drive/{i:02d}/five_calls"] = digest(ra)
            dig[f"drive/{i:02d}/detect_loop_scores"] = digest(A.detect_loop(kf_id, frame["bow"], kf.THRESHOLD, min_id_gap=3, with_scores=True))
            rb = B.process_keyframe(V, kf_id, img, feats, ex.prm, kf.THRESHOLD, **step)
            counts[f"drive/{i:02d}/step"] = B.debug_last_step()
            dig[f"drive/{i:02d}/process_keyframe"] = digest(rb)
            dig[f"drive/{i:02d}/pending"] = digest(B.pending())
            if ra["n_pairs"] < 10:
                A.add(kf_id, frame["bow"], frame["desc"], frame["class_id"])
                frames.append(frame)
            if rb["n_pairs"] < 10:
                B.add_pending()
            dig[f"drive/{i:02d}/sizes"] = digest((A.size(), B.size()))
        cur = frame
        for name, db in (("A", A), ("B", B)):
            dig[f"drive/end/{name}/scores"] = digest(db.detect_loop(1000, frames[3]["bow"], 0.0, min_id_gap=0, with_scores=True))
            for f in frames:
                dig[f"drive/end/{name}/match/{f['kf_id']:02d}"] = digest(db.match_features(f["kf_id"], cur["desc"], cur["class_id"]))
        A.close(); B.close()

        # ---- the batched step, with commits ----
        for S in (1, 5):
            dbs = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(S)]
            commit = [False] * S
            for i in range(len(places)):
                jobs = []
                for s, db in enumerate(dbs):
                    img, feats = scenes[places[(i + s) % len(places)]]
                    jobs.append(dict(db=db, kf_id=2 * i + 1, image=img, features=feats, commit_pending=commit[s]))
                got = sloop.process_keyframe_batch(V, jobs, ex.prm, kf.THRESHOLD, **step)
                counts[f"batch{S}/{i:02d}"] = sloop.debug_last_batch(ctx)
                for s, r in enumerate(got):
                    dig[f"batch{S}/{i:02d}/{s}/result"] = digest(r)
                    dig[f"batch{S}/{i:02d}/{s}/pending"] = digest(dbs[s].pending())
                    commit[s] = r["n_pairs"] < 10
            for s, db in enumerate(dbs):
                dig[f"batch{S}/end/{s}"] = digest((db.size(), db.detect_loop(1000, frames[3]["bow"], 0.0, min_id_gap=0, with_scores=True)))
                db.close()

        # ---- the relocalisation query on the twins ----
        img = make_stereo_pair(seed=140, h=200, w=320, n_blobs=400)[0]
        feats = po.orb_detect(img, prm=po.orb_params(nfeatures=60))
        kps, desc = ex.ScreenAndComputeKPsParams_CalcDescriptors(img, rq.expand(feats))
        frame = dict(img=img, feats=feats, desc=desc, cls=np.ascontiguousarray(kps["class_id"]), bow=V.transform(desc))
        rng = np.random.default_rng(77)
        kfs = [rq.synthetic_keyframe(rng, frame) for _ in range(max(rq.SIZES))]
        for n in rq.SIZES:
            db = sloop.KeyframeDatabase(ctx, keyframes_hint=4)
            for i in range(n):
                db.add(3 * i + 3, *kfs[i])
            for K in (1, 4, 8):
                for thr, ratio in ((0.0, 0.75), (0.02, 0.5)):
                    key = f"reloc/{n:04d}/K{K}/{thr}-{ratio}"
                    dig[key] = digest(db.relocalize_query(V, img, feats, ex.prm, max_candidates=K, threshold=thr, ratio=ratio, pyramid_levels=rq.LEVELS))
                    counts[key] = db.debug_last_step()
            db.close()
        V.close()

        # ---- the BowVector alone ----
        sizes = kf.BOW_SIZES
        rng = np.random.default_rng(1003)
        random = rng.integers(0, 256, (sizes[-1], 32), dtype=np.uint8)
        tiled = np.tile(rng.integers(0, 256, (40, 32), dtype=np.uint8), (sizes[-1] // 40, 1))
        for k, L, weighting in ((10, 3, 0), (2, 8, 1), (20, 2, 3)):
            voc = make_vocabulary(k=k, L=L, seed=k + L, stop_fraction=0.0)
            W = svoc.Vocabulary.from_arrays(ctx, k, L, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], weighting=weighting)
            for name, src in (("random", random), ("tiled", tiled)):
                for n in sizes:
                    dig[f"bow/{k}-{L}-{weighting}/{name}/{n:04d}"] = digest(sloop.debug_bow(W, src[:n]))
            W.close()
    return dict(digests=dig, counts=counts)


def compare(a, b):
    bad = 0
    da, db = a["digests"], b["digests"]
    diff = [k for k in sorted(set(da) | set(db)) if da.get(k) != db.get(k)]
    for g in sorted({k.split("/")[0] for k in da}):
        print(f"{g:10s} {sum(k.startswith(g + '/') for k in da):5d} digests, different: {[k for k in diff if k.startswith(g + '/')]}")
    print("digests", len(da), "|", len(db), "different", len(diff))
    bad += len(diff) + (not da)
    ca, cb = a["counts"], b["counts"]
    for k in sorted(set(ca) | set(cb)):
        if ca.get(k) != cb.get(k):
            print(f"counts {k}: {ca.get(k)} | {cb.get(k)}")
            bad += 1
    tot = lambda c, f: sum(v[f] for v in c.values())      # noqa: E731
    for f in ("launches", "syncs", "bytes_up", "bytes_down"):
        print(f"{f:10s} over {len(ca)} | {len(cb)} calls: {tot(ca, f)} | {tot(cb, f)}")
    return bad


def time_figures(path):
    """{label: microseconds}: the medians a tools/loop_db_time.py, tools/loop_batch_time.py or tools/reloc_time.py output states"""
    num = r"\s+([\d.]+)"
    out = {}
    for line in open(path):
        m = re.match(r"\s*(\d+)" + (num + r" \(\s*[\d.]+\)") * 3 + num + r"\s+[\d.]+x", line)
        if m:
            out[f"detect_loop {int(m.group(1)):5d} keyframes, end to end"] = float(m.group(4))
            out[f"detect_loop {int(m.group(1)):5d} keyframes, k_kfdb_score"] = float(m.group(5))
        m = re.match(r"\s*(\d+)" + (num + r" \(\s*[\d.]+\)") * 2 + num * 2 + r"\s*$", line)
        if m:
            out[f"match_features {int(m.group(1))} x {int(m.group(1))}, end to end"] = float(m.group(3))
            out[f"match_features {int(m.group(1))} x {int(m.group(1))}, k_kfdb_pairs"] = float(m.group(5))
        m = re.match(r"\s*(\d+)\s+(no loop|loop)" + (num + r" \[[^\]]*\] \([^)]*\)") * 2, line)
        if m:
            out[f"step  S {int(m.group(1)):2d} {m.group(2):7s} single calls"] = float(m.group(3))
            out[f"step  S {int(m.group(1)):2d} {m.group(2):7s} batch call"] = float(m.group(4))
        m = re.match(r"query  database\s+(\d+)  K (\d):  one call ([\d.]+) ms", line)
        if m:
            out[f"relocalize_query database {int(m.group(1)):4d} K {m.group(2)}"] = 1e3 * float(m.group(3))
    return out


def times(args):
    """LABEL=FILE ...: FILEs of the same label are runs of one library.  Per figure min / median / max of each label, and where the second
    label's median lies in the first's min-max (the rule of tools/po_host_ab.py --times); -> the figures above it"""
    runs = {}
    for a in args:
        label, path = a.split("=", 1)
        for k, v in time_figures(path).items():
            runs.setdefault(k, {}).setdefault(label, []).append(v)
    bad = 0
    for k, by in runs.items():
        (la, va), (lb, vb) = list(by.items())[:2]
        med = statistics.median(vb)
        where = "ABOVE" if med > max(va) else "below (faster than)" if med < min(va) else "inside"
        bad += med > max(va)
        f = lambda l, v: f"{l} min {min(v):9.1f} median {statistics.median(v):9.1f} max {max(v):9.1f} ({len(v)} runs: {' '.join('%.1f' % x for x in v)})"      # noqa: E731
        print(f"{k:46s} us  {f(la, va)} | {f(lb, vb)} | {lb} median {where} {la}'s min-max")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(1 if compare(json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))) else 0)
    if sys.argv[1] == "--times":
        sys.exit(1 if times(sys.argv[2:]) else 0)
    res = outputs()
    json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
    print("digests", len(res["digests"]), "counts", len(res["counts"]), "library", os.environ.get("SSX_LIB") or "ssvio_amd/libssx.so")
