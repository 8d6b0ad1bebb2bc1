"""A lateral drive seen by a RAW stereo rig -- a fisheye (kb4) left camera, a radtan right camera, a rotation between them -- for the
system tests and profiles of Camera.Rectify (modelled on tools/undistort_drive.py).

1. The raw rig is chosen: lenses, R21 = rot(1.5, -2, 1 degrees), a baseline of the length tests/host_util.write_sequence renders with,
   Camera.Rectified.f / cx / cy = the rendering camera (fx = 450, the principal point at the centre of 320 x 200).
2. The rectified rig follows from it by the contract (tools.rectify_model.rectify).
3. `rect` is rendered in that rig (write_sequence: tools.synth.make_lateral_sequence, a keyframe on every frame).
4. Every image is warped out by tools.rectify_model.unrectify_image: `raw`, what the raw cameras see.
5. `model` is the contract's rectification of `raw`: what ssx_undistort_lens must make of it, byte for byte.

The raw cameras see wider than the rectified one (f = 360 against 450) and their lenses are mild, so that no rectified pixel reads
the border of a raw image (all_taps_inside): black corners would give FAST edges to track.

A run on `model` with the key off reads its intrinsics and Camera.Base.Line as float (the reference's way); a run on `raw` with the key
set gets doubles from ssx_stereo_rectify.  f, cx, cy are floats as they stand; the baseline is made one: t21 is moved along the baseline by
a few units in its last place until the contract's b is exactly the float quotient the other run computes (baseline_as_read).

The accuracy bar of the raw drive: the rectified drive's own largest keyframe-centre error plus 2 * z_med / f (two pixels at the median
scene depth, the allowance of tools/undistort_drive.py): the images were resampled twice, bilinearly, on the way."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                        # (run as a script: python tools/rectify_drive.py)
    sys.path.insert(0, ROOT)

from tools import rectify_model as rm  # noqa: E402
from tools import synth  # noqa: E402
from tools import undistort_drive as ud_drive  # noqa: E402
from tools import undistort_model as um  # noqa: E402

H, W, FX = ud_drive.H, ud_drive.W, ud_drive.FX
K_RECT = (FX, FX, W / 2.0, H / 2.0)
CAMS = [dict(name="kb4", model=rm.KB4, K=(360.0, 362.0, 157.0, 102.0), coeffs=(-0.02, 0.005, -0.001, 0.0002)),
        dict(name="radtan", model=rm.RADTAN, K=(365.0, 361.0, 163.0, 98.5), coeffs=(-0.05, 0.01, 0.0008, -0.0005, 0.0))]
ANGLES_DEG = (1.5, -2.0, 1.0)
BASELINE_DIRECTION = (1.0, -0.03, 0.02)                         # of the right camera's centre, in the left camera's frame
TEST_DRIVE = ud_drive.TEST_DRIVE


def baseline_as_read():
    """the baseline a run with the key off computes: Camera.Base.Line / fx in float arithmetic, widened"""
    return float(np.float32(synth.KITTI_BF) / np.float32(FX))


def raw_rig():
    """-> (the rig as tools.rectify_model.rectify takes it, its rectification) with b == baseline_as_read() exactly"""
    R = rm.rot(*np.deg2rad(ANGLES_DEG))
    want = baseline_as_read()
    e = np.array(BASELINE_DIRECTION) / np.linalg.norm(BASELINE_DIRECTION)
    best = None
    for step in sorted(range(-64, 65), key=abs):                 # b moves by about one unit in its last place per step
        c = want + step * float(np.spacing(want))
        t = -(R @ (c * e))
        rig = dict(cam=[dict(model=cam["model"], K=cam["K"], coeffs=cam["coeffs"]) for cam in CAMS], R=R, t=tuple(float(v) for v in t),
                   f=K_RECT[0], cx=K_RECT[2], cy=K_RECT[3])
        out = rm.rectify(rig)
        if best is None or abs(out["b"] - want) < abs(best[1]["b"] - want):
            best = (rig, out)
        if out["b"] == want:
            break
    return best


def rig_settings(rig):
    """the settings keys of the raw rig (tests add Camera.Rectify: 1)"""
    cfg = {"Camera.Rectified.f": rig["f"], "Camera.Rectified.cx": rig["cx"], "Camera.Rectified.cy": rig["cy"]}
    for key, cam in (("Camera1", CAMS[0]), ("Camera2", CAMS[1])):
        cfg[key + ".Model"] = cam["name"]
        cfg.update({f"{key}.{n}": float(v) for n, v in zip(("fx", "fy", "cx", "cy"), cam["K"])})
        names = ("k1", "k2", "k3", "k4") if cam["model"] == rm.KB4 else ("k1", "k2", "p1", "p2", "k3")
        cfg.update({f"{key}.{n}": float(v) for n, v in zip(names, cam["coeffs"])})
    cfg.update({f"Stereo.R21.{i}": float(v) for i, v in enumerate(np.asarray(rig["R"]).reshape(9))})
    cfg.update({f"Stereo.t21.{i}": float(v) for i, v in enumerate(rig["t"])})
    return cfg


def make_drives(root, write_sequence, n_frames=12, step=0.25, seed=0):
    """write_sequence: tests/host_util.write_sequence.  -> dict(rect, raw, model: sequence directories; settings = the raw rig's keys; dt,
    centres [n, 3] ground truth in the rectified left frame, K, bf, z_med, margin = 2 * z_med / f, all_taps_inside: no rectified pixel
    reads the border of a raw image; exact_baseline: the contract's b is the float the key-off run computes)"""
    rig, out = raw_rig()
    assert tuple(out["newK"]) == K_RECT
    sides = [(out["R_l"], out["iR_l"]), (out["R_r"], out["iR_r"])]
    seq = write_sequence(os.path.join(root, "rect"), n_frames=n_frames, step=step, seed=seed, h=H, w=W)
    raw = [tuple(rm.unrectify_image(im, out["newK"], sides[s][0], CAMS[s]["model"], CAMS[s]["K"], CAMS[s]["coeffs"]) for s, im in enumerate(pair)) for pair in seq["frames"]]
    maps = [rm.lens_map(H, W, CAMS[s]["model"], CAMS[s]["K"], CAMS[s]["coeffs"], sides[s][1]) for s in range(2)]
    model = [tuple(um.remap(im, *maps[s]) for s, im in enumerate(pair)) for pair in raw]
    baseline = synth.KITTI_BF / FX
    centres = np.stack([step * np.arange(n_frames) * baseline, np.zeros(n_frames), np.zeros(n_frames)], 1)
    disp = synth.make_stereo_pair(seed=seed, h=H, w=W, n_blobs=4000, bf=synth.KITTI_BF)[2]      # the scene write_sequence rendered
    z_med = synth.KITTI_BF / float(np.median(disp))
    return dict(rect=seq["dir"], raw=ud_drive._write(os.path.join(root, "raw", "seq"), raw, seq["dt"]), model=ud_drive._write(os.path.join(root, "model", "seq"), model, seq["dt"]),
                settings=rig_settings(rig), rig=rig, rectified=out, dt=seq["dt"], centres=centres, K=K_RECT, bf=synth.KITTI_BF, z_med=z_med, margin=2.0 * z_med / FX,
                n_frames=n_frames, all_taps_inside=all(bool(um.all_taps_inside(H, W, *m).all()) for m in maps), exact_baseline=bool(out["b"] == baseline_as_read()))


run = ud_drive.run
centre_errors = ud_drive.centre_errors


def main():
    """profiles/rectify/drive.txt: the raw drive with Camera.Rectify: 1 against the model's images with the key off and against the rectified drive"""
    import argparse
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import host_util
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify", "drive.txt"))
    args = ap.parse_args()
    built = host_util.build_test_binaries()
    root = tempfile.mkdtemp()
    drives = make_drives(root, host_util.write_sequence, **TEST_DRIVE)
    a = run(built["run_kitti"], root, drives, "raw", "a", dict({"Camera.Rectify": 1}, **drives["settings"]))
    b = run(built["run_kitti"], root, drives, "model", "b", {})
    rect = run(built["run_kitti"], root, drives, "rect", "rect", {})
    for r in (a, b, rect):
        if r["r"].returncode != 0:
            raise SystemExit((r["r"].stdout + r["r"].stderr)[-2000:])
    fa, ea = centre_errors(a["traj"], drives)
    fr, er = centre_errors(rect["traj"], drives)
    same = open(a["traj"], "rb").read() == open(b["traj"], "rb").read()
    bar = float(er.max()) + drives["margin"]
    lines = ["rectification drive: %d frames a quarter baseline apart, 320 x 200, rectified f 450; left %s %s, right %s %s, R21 = rot%s degrees" %
             (drives["n_frames"], CAMS[0]["name"], CAMS[0]["coeffs"], CAMS[1]["name"], CAMS[1]["coeffs"], ANGLES_DEG),
             "no rectified pixel reads a raw image's border: %s; the contract's baseline is the key-off run's float: %s" % (drives["all_taps_inside"], drives["exact_baseline"]),
             "median depth %.3f m; margin 2 * z_med / f = %.4f m" % (drives["z_med"], drives["margin"]),
             "run A (raw images, Camera.Rectify: 1) and run B (the model's rectified images, key off) write %s trajectory bytes" % ("THE SAME" if same else "DIFFERENT"),
             "keyframe centre error against ground truth, run A:           " + " ".join("%d:%.4f" % (f, e) for f, e in zip(fa, ea)),
             "keyframe centre error against ground truth, rectified drive: " + " ".join("%d:%.4f" % (f, e) for f, e in zip(fr, er)),
             "largest error: run A %.4f m, rectified drive %.4f m, margin %.4f m; bar %.4f m: %s" % (ea.max(), er.max(), drives["margin"], bar, "met" if ea.max() <= bar else "MISSED")]
    lines += [l for l in a["r"].stdout.splitlines() if l.startswith("Camera.Rectify:") or "undistort (pair)" in l]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
