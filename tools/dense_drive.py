"""Frames per second of ssx_run_kitti with and without Dense.Open: 1, against another build's runner -> profiles/dense/drive.txt.

    python tools/dense_drive.py [--parent=<ssx_run_kitti of the parent commit>] [--out profiles/dense/drive.txt] [--repeats 3]

The drives: the one tests/test_dense_system_gpu.py renders (host_util.write_sequence, 320 x 200, 8 frames a quarter baseline apart, a
keyframe on every frame) and the same scene at KITTI size (376 x 1241, 12 frames).  The runs alternate in one job -- parent, new without
the key, new with the key -- each repeated; the figure is RunStep's frames per second as the runner prints it (decoding excluded,
warm-up outside the loop), given as median [min - max]."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def arg(name, default=None):
    for a in sys.argv[1:]:
        if a.startswith("--" + name + "="):
            return a.split("=", 1)[1]
    return default


def fps(exe, cfg, seq, extra=()):
    r = subprocess.run([exe, "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + seq, "--trajectory=" + cfg + ".traj", *extra], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit((r.stdout + r.stderr)[-2000:])
    m = re.search(r"RunStep ([\d.]+) ms/frame", r.stdout)
    d = re.search(r"dense \(keyframe pair\)\s+(\d+) calls\s+([\d.]+) ms/call", r.stdout)
    kf = re.search(r"keyframes (\d+)", r.stdout)
    return 1e3 / float(m.group(1)), (float(d.group(2)) if d else None), int(kf.group(1)), open(cfg + ".traj", "rb").read()


def main():
    import host_util as hu
    from ssvio_amd import build as b
    from tools import loop_drive, synth
    _, new = b.build_host()
    parent = arg("parent")
    out = arg("out", os.path.join(ROOT, "profiles", "dense", "drive.txt"))
    repeats = int(arg("repeats", "3"))
    lines = ["ssx_run_kitti with and without Dense.Open: 1 (tools/dense_drive.py): RunStep frames per second, median [min - max] of %d alternating runs" % repeats]
    with tempfile.TemporaryDirectory() as root:
        for name, h, w, fx, n in (("the system test's drive, 320 x 200, 8 frames", 200, 320, 450.0, 8), ("the same scene at 376 x 1241, 12 frames", 376, 1241, 718.856, 12)):
            seq = hu.write_sequence(os.path.join(root, "%dx%d" % (w, h)), n_frames=n, step=0.25, seed=0, h=h, w=w)
            drive = dict(K=(fx, fx, w / 2.0, h / 2.0), bf=synth.KITTI_BF)
            over = {"Camera.width": w, "Camera.height": h}
            off = synth.write_settings(os.path.join(root, "off%d.yaml" % w), loop_drive.drive_settings(drive, over))
            on = {D: synth.write_settings(os.path.join(root, "on%d_%d.yaml" % (w, D)), loop_drive.drive_settings(drive, dict(over, **{"Dense.Open": 1, "Dense.Disparities": D})))
                  for D in (64, 128)}
            runs = {"parent": [], "new, key absent": [], "new, Dense.Open: 1, 64 disparities": [], "new, Dense.Open: 1, 128 disparities": []}
            per_call = {64: [], 128: []}
            trajs = set()
            kfs = 0
            for _ in range(repeats):
                if parent:
                    f, _, kfs, t = fps(parent, off, seq["dir"]); runs["parent"].append(f); trajs.add(t)
                f, _, kfs, t = fps(new, off, seq["dir"]); runs["new, key absent"].append(f); trajs.add(t)
                for D in (64, 128):
                    f, d, kfs, t = fps(new, on[D], seq["dir"]); runs["new, Dense.Open: 1, %d disparities" % D].append(f); per_call[D].append(d); trajs.add(t)
            lines.append("%s, %d keyframes; every run wrote the same trajectory bytes: %s" % (name, kfs, len(trajs) == 1))
            for k, v in runs.items():
                if v:
                    lines.append("  %-38s %8.1f frames/s [%8.1f - %8.1f]" % (k, np.median(v), min(v), max(v)))
                else:
                    lines.append("  %-38s not measured (no --parent given)" % k)
            for D in (64, 128):
                lines.append("  the phase `dense` at %3d disparities: %.3f ms per keyframe [%.3f - %.3f] (host images: staged up and down, one synchronisation)"
                             % (D, np.median(per_call[D]), min(per_call[D]), max(per_call[D])))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def post():
    """--post: the runner's phase `dense` (host images) with the samples made on the host or on the device, with and without the speckle
    filter -> profiles/dense_post/drive.txt.  The same scene at KITTI size; the runs alternate, each repeated."""
    import host_util as hu
    from ssvio_amd import build as b
    from tools import loop_drive, synth
    _, new = b.build_host()
    out = arg("out", os.path.join(ROOT, "profiles", "dense_post", "drive.txt"))
    repeats = int(arg("repeats", "3"))
    h, w, fx, n = 376, 1241, 718.856, 12
    variants = {"Dense.Open: 1 (the map down, SampleDense on the host)": {},
                "+ Dense.Cloud.OnDevice: 1 (samples down, no map)": {"Dense.Cloud.OnDevice": 1},
                "+ Dense.Speckle.Size: 100 (filtered map down, host samples)": {"Dense.Speckle.Size": 100},
                "+ both (samples of the filtered map down, no map)": {"Dense.Speckle.Size": 100, "Dense.Cloud.OnDevice": 1}}
    lines = ["ssx_run_kitti's phase `dense` at %d x %d, %d frames, a keyframe on every frame, host images (tools/dense_drive.py --post):" % (h, w, n),
             "ms per keyframe as the runner prints it, and RunStep frames per second; median [min - max] of %d alternating runs" % repeats]
    with tempfile.TemporaryDirectory() as root:
        seq = hu.write_sequence(os.path.join(root, "seq"), n_frames=n, step=0.25, seed=0, h=h, w=w)
        drive = dict(K=(fx, fx, w / 2.0, h / 2.0), bf=synth.KITTI_BF)
        for D in (64, 128):
            base = {"Camera.width": w, "Camera.height": h, "Dense.Open": 1, "Dense.Disparities": D}
            cfgs = {k: synth.write_settings(os.path.join(root, "v%d_%d.yaml" % (i, D)), loop_drive.drive_settings(drive, dict(base, **v))) for i, (k, v) in enumerate(variants.items())}
            ms, fr, trajs = {k: [] for k in variants}, {k: [] for k in variants}, set()
            for _ in range(repeats):
                for k in variants:
                    f, d, _, t = fps(new, cfgs[k], seq["dir"])
                    ms[k].append(d); fr[k].append(f); trajs.add(t)
            lines.append("  %d disparities; every run wrote the same trajectory bytes: %s" % (D, len(trajs) == 1))
            for k in variants:
                lines.append("    %-62s %7.3f ms [%.3f - %.3f]   %7.1f frames/s [%.1f - %.1f]" % (k, np.median(ms[k]), min(ms[k]), max(ms[k]), np.median(fr[k]), min(fr[k]), max(fr[k])))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    post() if "--post" in sys.argv[1:] else main()
