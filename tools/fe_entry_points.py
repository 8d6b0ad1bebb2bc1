"""Every ORB / stereo entry point once, on fixed inputs: the run to put under `rocprofv3 --kernel-trace --stats` (kernels and their
call counts) or under a runtime trace (copies, synchronisations) when the host side changes and the device side must not, and, with
an output directory, every result as .npy for a byte-for-byte comparison between two builds (SSX_LIB=<the other libssx.so>).
    python tools/fe_entry_points.py [out_dir]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import ssvio_amd
from ssvio_amd import orb
from tools.synth import make_stereo_pair

out_dir = sys.argv[1] if len(sys.argv) > 1 else None
res = {}
ctx = ssvio_amd.Context(0)
L, R = make_stereo_pair(seed=0)[:2]
S = make_stereo_pair(seed=7, h=160, w=260, n_blobs=260)[0]
mask = np.full(L.shape, 255, np.uint8); mask[100:200, 300:700] = 0
boxes = np.array([[300, 100, 699, 199], [10, 10, 60, 60]], np.int32)
ex = orb.ORBextractor(ctx, nfeatures=300)
res["detect"] = ex.Detect(L)
res["detect_mask"] = ex.Detect(L, mask)
res["detect_boxes"] = ex.DetectBoxes(L, boxes)
for j, k in enumerate(ex.DetectBoxesBatch([L, R, L], [boxes, boxes[:1], boxes[:0]])):      # plans I = 4
    res["detect_batch_%d" % j] = k
for j, k in enumerate(ex.DetectBoxesBatch([R], [boxes])):                                  # runs on the larger plan
    res["detect_batch_small_%d" % j] = k
ex2 = orb.ORBextractor(ctx)
kL, dL = ex2.DetectAndCompute(L); kR, dR = ex2.DetectAndCompute(R)
res.update(extract_k=kL, extract_d=dL)
k3, d3 = orb.ORBextractor(ctx, nfeatures=300, nlevels=4).DetectAndCompute(S, np.where(np.arange(S.shape[1])[None, :] < 130, 255, 0).astype(np.uint8).repeat(S.shape[0], 0))
res.update(extract_mask_k=k3, extract_mask_d=d3)
kk, dd = ex2.ScreenAndComputeKPsParams_CalcDescriptors(L, kL[:500])
res.update(describe_k=kk, describe_d=dd)
mi, md = orb.stereo_match(ctx, kL, dL, kR, dR)
res.update(match_idx=mi, match_dist=md)
bi, bd = orb.bf_match(ctx, dL, dR)
res.update(bf_idx=bi, bf_dist=bd)
uvL = np.array([[kL["x"][i], kL["y"][i]] for i in range(len(kL)) if mi[i] >= 0], np.float64)
uvR = np.array([[kR["x"][mi[i]], kR["y"][mi[i]]] for i in range(len(kL)) if mi[i] >= 0], np.float64)
xyz, ok = orb.triangulate(ctx, uvL, uvR)
res.update(tri_xyz=xyz, tri_ok=ok)
for j, (x, o) in enumerate(orb.triangulate_batch(ctx, [dict(uvL=uvL, uvR=uvR), dict(uvL=uvL[:7], uvR=uvR[:7])])):
    res["tri_batch_xyz_%d" % j] = x; res["tri_batch_ok_%d" % j] = o
fr = orb.stereo_frame(ctx, L, R)
for k, v in fr.items():
    res["frame_" + k] = np.asarray(v)
B, H, W = 4, 200, 320
prm = orb.OrbParams(300, 1.2, 4, 20, 7)
batches = [np.stack([np.stack(make_stereo_pair(seed=50 + 10 * b + i, h=H, w=W, n_blobs=400)[:2]) for i in range(B)]) for b in range(3)]
dev = torch.from_numpy(batches[0]).cuda()
res["batch_dev_counts"] = orb.stereo_batch_dev(ctx, dev.data_ptr(), B, W, H, W, orb=prm).copy()
for p in range(B):
    for k, v in orb.stereo_batch_fetch(ctx, p, 2048).items():
        res["batch_dev_%d_%s" % (p, k)] = np.asarray(v)
pinned = [torch.from_numpy(hb).pin_memory() for hb in batches]
st = orb.StereoStream(ctx, B, H, W, orb=prm)
st.upload(pinned[0].data_ptr())
for b in range(3):
    if b + 1 < 3:
        st.upload(pinned[b + 1].data_ptr())                          # one ahead
    st.run()
    res["stream_counts_%d" % b] = np.asarray(st.wait_counts()).copy()
for k, v in orb.stereo_batch_fetch(ctx, B - 1, 2048).items():
    res["stream_last_%s" % k] = np.asarray(v)
ctx.close()
import hashlib
h = hashlib.sha256()
for k in sorted(res):
    a = np.ascontiguousarray(res[k]); h.update(k.encode()); h.update(a.tobytes())
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, k + ".npy"), a)
print("entry points run:", len(res), "arrays, sha256", h.hexdigest())
