"""A lateral drive with an interruption, for the relocalisation tests and profiles.

The rig of tools.synth.make_lateral_sequence moves sideways by `step` baselines per frame (the camera and settings of
tools.loop_drive: 320 x 200, fx = 450, a keyframe on every frame).  Frames b .. b + n_blank - 1 are replaced in BOTH images -- by
constant grey, or by noise textures that have nothing to do with the scene or with each other -- so that the tracker loses every
feature at frame b.  Without relocalisation the run is over there; with it, frame b + n_blank has to find itself in the keyframe
database.

What frame b + n_blank still shares with the last keyframe before the gap (frame b - 1): the rig has moved (n_blank + 1) * step
baselines, a point at the scene's median depth has moved that many median disparities across the image.  The drive's "overlap" is the
share of the image width that remains; the tests require at least half."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                        # (run as a script: python tools/reloc_drive.py)
    sys.path.insert(0, ROOT)

from tools import synth  # noqa: E402


# the drive of tests/test_reloc_host.py, tests/test_reloc_system_gpu.py and profiles/reloc/drive.txt: 4 steps of a quarter baseline between the
# last keyframe before the gap and the first frame after it
TEST_DRIVE = dict(n_frames=16, step=0.25, b=8, n_blank=3)
# loop closing as tests/test_loop_system_gpu.py sets it, with a keyframe gap no pair of this short drive reaches: no loop is looked for,
# every keyframe enters the database
LOOP_SETTINGS = {"Loop.Closing.Open": 1, "Loop.Show.Closing.Result": 0, "Loop.Threshold.Heigher": 0.5, "Loop.Threshold.Lower": 0.02, "Pyramid.Level": 4,
                 "Loop.Closig.Keyframe.Database.Min.Size": 3, "Loop.Min.Keyframe.Gap": 100}


def make_reloc_drive(root, n_frames=16, step=0.25, b=8, n_blank=3, blank="grey", seed=0, h=200, w=320, n_blobs=1500, dt=0.1, fx=450.0, tag="seq"):
    """Writes <root>/<tag> in KITTI layout.  blank: "grey", "noise" or None (the same drive uninterrupted).  -> dict(dir, dt, centres
    [n, 3] ground truth, n_frames, b, n_blank, K, bf, step, disp_med (pixels per baseline at the median depth), z_med, overlap)."""
    from PIL import Image
    K = (float(fx), float(fx), w / 2.0, h / 2.0)
    baseline = synth.KITTI_BF / float(fx)
    frames, gt, disp = synth.make_lateral_sequence(n_frames=n_frames, step=step, seed=seed, h=h, w=w, n_blobs=n_blobs)
    frames = [list(f) for f in frames]
    rng = np.random.default_rng(900 + seed)
    for i in range(b, b + n_blank if blank else b):
        for cam in (0, 1):
            if blank == "grey":
                frames[i][cam] = np.full((h, w), 128, np.uint8)
            elif blank == "noise":                                  # smooth noise with corners of its own: trackable, but not this scene
                coarse = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1)).astype(np.float32)
                img = np.kron(coarse, np.ones((8, 8), np.float32))[:h, :w] * 0.7 + rng.integers(0, 77, (h, w))
                frames[i][cam] = np.clip(img, 0, 255).astype(np.uint8)
            else:
                raise ValueError("blank: grey, noise or None")
    alphas = step * np.arange(n_frames)
    centres = np.stack([alphas * baseline, np.zeros(n_frames), np.zeros(n_frames)], 1)
    d = os.path.join(root, tag)
    for sub in ("image_0", "image_1"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    with open(os.path.join(d, "times.txt"), "w") as f:
        for i, (L, R) in enumerate(frames):
            f.write(f"{i * dt:e}\n")
            Image.fromarray(L).save(os.path.join(d, "image_0", f"{i:06d}.png"))
            Image.fromarray(R).save(os.path.join(d, "image_1", f"{i:06d}.png"))
    disp_med = float(np.median(disp))
    return dict(dir=d, dt=dt, centres=centres, n_frames=n_frames, b=b, n_blank=n_blank, K=K, bf=synth.KITTI_BF, step=step, disp_med=disp_med,
                z_med=synth.KITTI_BF / disp_med, overlap=1.0 - (n_blank + 1) * step * disp_med / w)


def centre_errors(traj_path, drive):
    """-> (frames, |estimated centre - ground truth| per keyframe of a TUM trajectory, both relative to the first keyframe)"""
    tum = np.loadtxt(traj_path, ndmin=2)
    frame = np.rint(tum[:, 0] / drive["dt"]).astype(int)
    est = tum[:, 1:4] - tum[0, 1:4]
    gt = drive["centres"][frame] - drive["centres"][frame[0]]
    return frame, np.linalg.norm(est - gt, axis=1)


def run_drive(run_kitti, root, drive, voc, tag, overrides=None, extra=(), timeout=120):
    """ssx_run_kitti on the drive with LOOP_SETTINGS + overrides -> dict(r = the finished process, traj, log, cfg)"""
    import subprocess

    from tools import loop_drive
    over = dict(LOOP_SETTINGS, **{"DBOW2.VOC.Path": '"%s"' % voc})
    over.update(overrides or {})
    cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), loop_drive.drive_settings(drive, over))
    traj, log = os.path.join(root, tag + ".traj"), os.path.join(root, tag + ".looplog")
    r = subprocess.run([run_kitti, "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + drive["dir"], "--trajectory=" + traj, "--loop_log=" + log, *extra],
                       capture_output=True, text=True, timeout=timeout)
    return dict(r=r, traj=traj, log=log, cfg=cfg)


def accuracy(traj_reloc, traj_clean, drive, first):
    """the accuracy bar over the keyframes of frames >= first: -> (largest centre error of the relocalised run, of the uninterrupted run on those
    frames, the margin 2 px of reprojection error mean at the scene's median depth = 2 * z_med / fx)"""
    fr, er = centre_errors(traj_reloc, drive)
    fc, ec = centre_errors(traj_clean, drive)
    frames = [f for f in fr if f >= first]
    e_reloc = max(float(er[list(fr).index(f)]) for f in frames)
    e_clean = max(float(ec[list(fc).index(f)]) for f in frames)
    return e_reloc, e_clean, 2.0 * drive["z_med"] / drive["K"][0]


def main():
    """profiles/reloc/drive.txt: the test drive interrupted with relocalisation on, and uninterrupted with the key absent"""
    import argparse
    import tempfile
    root_dir = ROOT
    sys.path.insert(0, os.path.join(root_dir, "tests"))
    import host_util
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root_dir, "profiles", "reloc", "drive.txt"))
    args = ap.parse_args()
    built = host_util.build_test_binaries()
    root = tempfile.mkdtemp()
    drive = make_reloc_drive(root, **TEST_DRIVE)
    clean = make_reloc_drive(root, blank=None, tag="clean", **TEST_DRIVE)
    voc = os.path.join(root, "voc.txt")
    synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
    on = run_drive(built["run_kitti"], root, drive, voc, "on", {"Relocalization.Open": 1})
    base = run_drive(built["run_kitti"], root, clean, voc, "clean", {})
    if on["r"].returncode != 0 or base["r"].returncode != 0:
        raise SystemExit(on["r"].stderr[-2000:] + base["r"].stderr[-2000:])
    attempts = [l.strip() for l in open(on["log"]) if l.startswith("reloc_frame")]
    first = [int(l.split()[1]) for l in attempts if int(l.split()[-1]) >= 0][0]
    e_reloc, e_clean, margin = accuracy(on["traj"], base["traj"], drive, first)
    fr, er = centre_errors(on["traj"], drive)
    fc, ec = centre_errors(base["traj"], drive)
    lines = ["relocalisation drive: %(n_frames)d frames, step %(step)g baselines, frames %(b)d .. " % drive + "%d constant grey; 320 x 200, fx 450" % (drive["b"] + drive["n_blank"] - 1),
             "median disparity %.3f px per baseline, median depth %.3f m, shared view of frame %d and frame %d: %.1f %%" %
             (drive["disp_med"], drive["z_med"], drive["b"] + drive["n_blank"], drive["b"] - 1, 100 * drive["overlap"])]
    lines += [l for l in on["r"].stderr.splitlines() if "tracking lost" in l or "relocalisation" in l] + attempts
    lines += ["keyframe centre error against ground truth, relocalised run:   " + " ".join("%d:%.4f" % (f, e) for f, e in zip(fr, er)),
              "keyframe centre error against ground truth, uninterrupted run: " + " ".join("%d:%.4f" % (f, e) for f, e in zip(fc, ec)),
              "largest error over the keyframes from frame %d on: relocalised %.4f m, uninterrupted %.4f m; margin 2 * z_med / fx = %.4f m; bar %.4f m: %s" %
              (first, e_reloc, e_clean, margin, e_clean + margin, "met" if e_reloc <= e_clean + margin else "MISSED")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
