"""The relocalisation drive of tools/reloc_drive.py with the guided search (Relocalization.Guided.Open: 1) against the same
drive with the key off: what the second step gathers, matches and keeps, and what it does to the recovered pose.

    python tools/reloc_guided_drive.py [--out profiles/reloc_guided/drive.txt]      (needs the MI355X)"""
from __future__ import annotations

import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import reloc_drive, synth  # noqa: E402

GUIDED_LINE = re.compile(r"frame (\d+): guided search (accepted|refused): (\d+) points, (\d+) matched, inliers (\d+) -> (-?\d+), matches (\d+) -> (\d+)")


def parse_guided(stderr):
    """the front-end's lines about the guided search -> [dict(frame, accepted, points, matched, inliers_before, inliers_after, matches_before, matches_after)]"""
    keys = ("frame", "accepted", "points", "matched", "inliers_before", "inliers_after", "matches_before", "matches_after")
    out = []
    for m in GUIDED_LINE.finditer(stderr):
        g = list(m.groups())
        g[1] = g[1] == "accepted"
        out.append({k: (v if k == "accepted" else int(v)) for k, v in zip(keys, g)})
    return out


def reloc_lines(path):
    """the reloc_frame lines of a loop log as dicts of ints"""
    out = []
    for line in open(path):
        w = line.split()
        if w and w[0] == "reloc_frame":
            out.append({k: int(v) for k, v in zip(w[0::2], w[1::2])})
    return out


def main():
    import argparse
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import host_util
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_guided", "drive.txt"))
    args = ap.parse_args()
    built = host_util.build_test_binaries()
    root = tempfile.mkdtemp()
    drive = reloc_drive.make_reloc_drive(root, **reloc_drive.TEST_DRIVE)
    clean = reloc_drive.make_reloc_drive(root, blank=None, tag="clean", **reloc_drive.TEST_DRIVE)
    voc = os.path.join(root, "voc.txt")
    synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
    off = reloc_drive.run_drive(built["run_kitti"], root, drive, voc, "off", {"Relocalization.Open": 1})
    on = reloc_drive.run_drive(built["run_kitti"], root, drive, voc, "on", {"Relocalization.Open": 1, "Relocalization.Guided.Open": 1})
    base = reloc_drive.run_drive(built["run_kitti"], root, clean, voc, "clean", {})
    for r in (off, on, base):
        if r["r"].returncode != 0:
            raise SystemExit(r["r"].stderr[-2000:])
    lines = ["relocalisation drive of tools/reloc_drive.py (%(n_frames)d frames, step %(step)g baselines, 320 x 200, fx 450), " % drive +
             "Relocalization.Guided.Open: 1 against the key off; defaults: 2 neighbours, radius 10 px, distance 50, ratio 90"]
    lines += [l for l in on["r"].stderr.splitlines() if "relocalisation succeeded" in l or "guided search" in l]
    lines += ["key on:  " + l.strip() for l in open(on["log"]) if l.startswith("reloc_frame")]
    lines += ["key off: " + l.strip() for l in open(off["log"]) if l.startswith("reloc_frame")]
    for tag, run in (("key on", on), ("key off", off)):
        first = [l["reloc_frame"] for l in reloc_lines(run["log"]) if l["accepted"] >= 0][0]
        e_reloc, e_clean, margin = reloc_drive.accuracy(run["traj"], base["traj"], drive, first)
        fr, er = reloc_drive.centre_errors(run["traj"], drive)
        lines += ["%s: keyframe centre error against ground truth: " % tag + " ".join("%d:%.4f" % (f, e) for f, e in zip(fr, er)),
                  "%s: largest error over the keyframes from frame %d on: relocalised %.4f m, uninterrupted %.4f m; margin 2 * z_med / fx = %.4f m; bar %.4f m: %s" %
                  (tag, first, e_reloc, e_clean, margin, e_clean + margin, "met" if e_reloc <= e_clean + margin else "MISSED")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
