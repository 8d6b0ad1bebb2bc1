"""A lateral drive seen through distorting lenses, for the system tests and profiles of Camera.NeedUndistortion.

The rectified drive is tests/host_util.write_sequence at 320 x 200 (tools.synth.make_lateral_sequence) with the camera of
tools.loop_drive (fx = 450, principal point at the image centre, a keyframe on every frame).  Every image is then warped by
tools.undistort_model.distort_image with barrel coefficients -- barrel, because the undistorted image then samples only valid source
pixels; with pincushion it would carry black corners and FAST would track their edges -- left and right with different ones.  Three
sequences come out: `rect` (as rendered), `dist` (what the distorting cameras see) and `model` (tools.undistort_model.undistort of
`dist`: what ssx_undistort must make of it, byte for byte).

The accuracy bar of the distorted drive: the rectified drive's own largest keyframe-centre error plus the translation 2 px of
reprojection error mean at the scene's median depth, 2 * z_med / fx (the allowance of tools/reloc_drive.py): the images were resampled
twice, bilinearly, on the way."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                        # (run as a script: python tools/undistort_drive.py)
    sys.path.insert(0, ROOT)

from tools import loop_drive, synth  # noqa: E402
from tools import undistort_model as um  # noqa: E402

H, W, FX = 200, 320, 450.0
K = (FX, FX, W / 2.0, H / 2.0)
# k1 k2 p1 p2 per camera, as the settings file states them; System reads them as float and widens them
COEFFS = {"Camera1": (-0.20, 0.03, 0.0008, -0.0005), "Camera2": (-0.18, 0.02, -0.0006, 0.0004)}
TEST_DRIVE = dict(n_frames=12, step=0.25, seed=0)


def as_read(coeffs):
    """(k1, k2, p1, p2) of the settings file -> dist (k1, k2, p1, p2, k3 = 0) as System hands it on: float, widened"""
    return tuple(float(np.float32(v)) for v in coeffs) + (0.0,)


def coefficient_settings(coeffs=COEFFS):
    return {f"{cam}.{name}": v for cam, c in coeffs.items() for name, v in zip(("k1", "k2", "p1", "p2"), c)}


def _write(d, frames, dt):
    from PIL import Image
    for sub in ("image_0", "image_1"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    with open(os.path.join(d, "times.txt"), "w") as f:
        for i, (L, R) in enumerate(frames):
            f.write(f"{i * dt:e}\n")
            Image.fromarray(L).save(os.path.join(d, "image_0", f"{i:06d}.png"))
            Image.fromarray(R).save(os.path.join(d, "image_1", f"{i:06d}.png"))
    return d


def make_drives(root, write_sequence, n_frames=12, step=0.25, seed=0):
    """write_sequence: tests/host_util.write_sequence.  -> dict(rect, dist, model: sequence directories; dt, centres [n, 3] ground truth,
    K, bf, z_med, margin = 2 * z_med / fx, all_taps_inside: no undistorted pixel reads the border)"""
    seq = write_sequence(os.path.join(root, "rect"), n_frames=n_frames, step=step, seed=seed, h=H, w=W)
    dl, dr = as_read(COEFFS["Camera1"]), as_read(COEFFS["Camera2"])
    dist = [(um.distort_image(L, K, dl), um.distort_image(R, K, dr)) for L, R in seq["frames"]]
    model = [(um.undistort(L, K, dl), um.undistort(R, K, dr)) for L, R in dist]
    baseline = synth.KITTI_BF / FX
    centres = np.stack([step * np.arange(n_frames) * baseline, np.zeros(n_frames), np.zeros(n_frames)], 1)
    disp = synth.make_stereo_pair(seed=seed, h=H, w=W, n_blobs=4000, bf=synth.KITTI_BF)[2]      # the scene write_sequence rendered
    z_med = synth.KITTI_BF / float(np.median(disp))
    return dict(rect=seq["dir"], dist=_write(os.path.join(root, "dist", "seq"), dist, seq["dt"]), model=_write(os.path.join(root, "model", "seq"), model, seq["dt"]),
                dt=seq["dt"], centres=centres, K=K, bf=synth.KITTI_BF, z_med=z_med, margin=2.0 * z_med / FX, n_frames=n_frames,
                all_taps_inside=all(bool(um.all_taps_inside(H, W, *um.undistort_map(H, W, K, d)).all()) for d in (dl, dr)))


def run(run_kitti, root, drives, which, tag, overrides=None, extra=(), timeout=120):
    """ssx_run_kitti on one of the drive's sequences -> dict(r = the finished process, traj, cfg)"""
    cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), loop_drive.drive_settings(drives, overrides))
    traj = os.path.join(root, tag + ".traj")
    r = subprocess.run([run_kitti, "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + drives[which], "--trajectory=" + traj, *extra],
                       capture_output=True, text=True, timeout=timeout)
    return dict(r=r, traj=traj, cfg=cfg)


def centre_errors(traj_path, drives):
    """-> (frames, |estimated centre - ground truth| per keyframe of a TUM trajectory, both relative to the first keyframe)"""
    tum = np.loadtxt(traj_path, ndmin=2)
    frame = np.rint(tum[:, 0] / drives["dt"]).astype(int)
    est = tum[:, 1:4] - tum[0, 1:4]
    gt = drives["centres"][frame] - drives["centres"][frame[0]]
    return frame, np.linalg.norm(est - gt, axis=1)


def main():
    """profiles/undistort/drive.txt: the distorted drive with the key set against the rectified drive, and the runner's frames/s on one
    full-size drive with the key 0 and with the key 1 at zero coefficients"""
    import argparse
    import re
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import host_util
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort", "drive.txt"))
    args = ap.parse_args()
    built = host_util.build_test_binaries()
    root = tempfile.mkdtemp()
    drives = make_drives(root, host_util.write_sequence, **TEST_DRIVE)
    on = dict({"Camera.NeedUndistortion": 1}, **coefficient_settings())
    a = run(built["run_kitti"], root, drives, "dist", "a", on)
    b = run(built["run_kitti"], root, drives, "model", "b", {})
    rect = run(built["run_kitti"], root, drives, "rect", "rect", {})
    for r in (a, b, rect):
        if r["r"].returncode != 0:
            raise SystemExit(r["r"].stderr[-2000:])
    fa, ea = centre_errors(a["traj"], drives)
    fr, er = centre_errors(rect["traj"], drives)
    same = open(a["traj"], "rb").read() == open(b["traj"], "rb").read()
    bar = float(er.max()) + drives["margin"]
    lines = ["undistortion drive: %d frames a quarter baseline apart, 320 x 200, fx 450; barrel, k1 k2 p1 p2 left %s right %s" % (drives["n_frames"], COEFFS["Camera1"], COEFFS["Camera2"]),
             "median depth %.3f m; margin 2 * z_med / fx = %.4f m" % (drives["z_med"], drives["margin"]),
             "run A (distorted images, Camera.NeedUndistortion: 1) and run B (the model's undistorted images, key 0) write %s trajectory bytes" % ("THE SAME" if same else "DIFFERENT"),
             "keyframe centre error against ground truth, run A:           " + " ".join("%d:%.4f" % (f, e) for f, e in zip(fa, ea)),
             "keyframe centre error against ground truth, rectified drive: " + " ".join("%d:%.4f" % (f, e) for f, e in zip(fr, er)),
             "largest error: run A %.4f m, rectified drive %.4f m; bar %.4f m: %s" % (ea.max(), er.max(), bar, "met" if ea.max() <= bar else "MISSED")]
    # the runner's rate on one full-size drive (KITTI 00's camera and size), key 0 against key 1 with zero coefficients, alternating
    big = host_util.write_sequence(os.path.join(root, "big"), n_frames=40, step=0.6)
    rates = {0: [], 1: []}
    for rep in range(3):
        for key in (0, 1):
            cfg = synth.write_settings(os.path.join(root, "big%d.yaml" % key), {"Camera.NeedUndistortion": key})
            r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + big["dir"], "--trajectory=" + os.path.join(root, "big%d.traj" % key)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-2000:])
            rates[key].append(float(re.search(r"RunStep [0-9.]+ ms/frame \(([0-9.]+) frames/s\)", r.stdout).group(1)))
            if key == 1 and rep == 2:
                lines += [l for l in r.stdout.splitlines() if "undistort (pair)" in l]
    lines.append("ssx_run_kitti, 40 frames of 1241 x 376, RunStep frames/s (three runs each, alternating): key 0 %s; key 1 with zero coefficients %s" %
                 (" ".join("%.1f" % v for v in rates[0]), " ".join("%.1f" % v for v in rates[1])))
    lines.append("the two trajectories are %s" % ("byte-identical" if open(os.path.join(root, "big0.traj"), "rb").read() == open(os.path.join(root, "big1.traj"), "rb").read() else "DIFFERENT"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
