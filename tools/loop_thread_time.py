"""What loop closing costs in the headless runner: the there-and-back test drive (tools/loop_drive.py, the parameters of
tests/test_loop_system_gpu.py) and the 200-pair corridor drive (BASELINE configs[0] shape), each with loop closing off, inline in the
backend, and on its own thread -- milliseconds per loop step, milliseconds of a correction, frames per second.

    python -m tools.loop_thread_time [corridor frames = 200]        (needs the GPU; prints the table profiles/loop_thread/time.txt holds)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tools import loop_drive, synth  # noqa: E402


def run(exe, cfg, seq, tag):
    r = subprocess.run([exe, "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + seq, "--trajectory=" + cfg + ".traj", "--loop_log=" + cfg + ".looplog"],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(tag + ": " + (r.stdout + r.stderr)[-600:])
    fps = re.search(r"RunStep [\d.]+ ms/frame \(([\d.]+) frames/s\).*whole loop ([\d.]+) frames/s", r.stdout)
    loop = re.search(r"loop closing.*", r.stdout)
    print(f"{tag:42s} RunStep {fps.group(1):>8s} frames/s   whole loop {fps.group(2):>8s} frames/s")
    if loop:
        print(" " * 42 + " " + loop.group(0).strip())


def main():
    import host_util
    from ssvio_amd import build as b
    _, exe = b.build_host()
    n_corridor = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    with tempfile.TemporaryDirectory() as d:
        voc = os.path.join(d, "voc.txt")
        synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
        drive = loop_drive.make_loop_drive(os.path.join(d, "drive"), n_leg=24, reach=7.0, right_factor=2.2, fx=450.0)
        loop = {"Loop.Closing.Open": 1, "DBOW2.VOC.Path": '"%s"' % voc, "Loop.Threshold.Heigher": 0.5, "Pyramid.Level": 4, "Loop.Closig.Keyframe.Database.Min.Size": 3,
                "Loop.Min.Keyframe.Gap": 8}
        print(f"--- the test drive: {drive['n_frames']} pairs of 320 x 200, a keyframe on every frame, window of 5")
        for tag, over in (("loop closing off", {}), ("loop closing inline", loop), ("loop closing on its own thread", dict(loop, **{"Loop.Closing.Async": 1, "Backend.Async": 1})),
                          ("off, Backend.Async: 1", {"Backend.Async": 1})):
            cfg = synth.write_settings(os.path.join(d, "t_" + tag.replace(" ", "_").replace(",", "").replace(":", "") + ".yaml"), loop_drive.drive_settings(drive, over))
            run(exe, cfg, drive["dir"], tag)
        os.makedirs(os.path.join(d, "corridor"))
        seq = host_util.write_corridor_sequence(os.path.join(d, "corridor"), n_frames=n_corridor)
        # the reference's own keys (kitti_00.yaml): 50 keyframes before the first look, candidates 20 ids back, 8 pyramid levels; the threshold of the test drive
        ref = {"Loop.Closing.Open": 1, "DBOW2.VOC.Path": '"%s"' % voc, "Loop.Threshold.Heigher": 0.5, "Pyramid.Level": 8, "Loop.Closig.Keyframe.Database.Min.Size": 50}
        low = dict(ref, **{"Loop.Closig.Keyframe.Database.Min.Size": 3, "Loop.Threshold.Heigher": 0.3})
        print(f"--- the corridor drive: {n_corridor} pairs of 1241 x 376, kitti_00.yaml settings (a keyframe when <= 50 inliers remain), window of 12")
        for tag, over in (("loop closing off", {}), ("loop closing inline", ref), ("inline, database from 3, threshold 0.3", low),
                          ("loop closing on its own thread", dict(ref, **{"Loop.Closing.Async": 1, "Backend.Async": 1}))):
            cfg = synth.write_settings(os.path.join(d, "c_" + tag.replace(" ", "_").replace(",", "").replace(":", "") + ".yaml"), over)
            run(exe, cfg, seq["dir"], tag)


if __name__ == "__main__":
    main()
