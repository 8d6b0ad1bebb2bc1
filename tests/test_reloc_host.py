"""CPU: relocalisation in the host layer, as far as it needs no device.

1. The premise of tests/test_reloc_system_gpu.py, on the CPU-oracle runner: the drive of tools/reloc_drive.py with frames b .. b + 2 replaced
   by constant grey loses tracking at frame b and, without relocalisation (the oracle's Compute has no loop closing), stays LOST to the end:
   no keyframe is written after b.  The step is short enough for frame b + 3 to share most of its view with the last keyframe.
2. LoopClosing::Relocalize against a scripted LoopCompute (tests/host/test_reloc_units.cpp): the settings defaults, what is gathered and
   asked for, and the acceptance rule against tools/reloc_model.accept.
3. The combinations that are refused or ignored."""
import os
import subprocess

import pytest

import host_util
from tools import loop_drive, reloc_drive, synth
from tools.reloc_model import accept

DRIVE = reloc_drive.TEST_DRIVE
BASE = {"ORBextractor.nNewFeatures": 100, "ORBextractor.scaleFactor": 1.2, "ORBextractor.nLevels": 8, "ORBextractor.iniThFAST": 20, "ORBextractor.minThFAST": 7,
        "Loop.Threshold.Heigher": 0.5, "Pyramid.Level": 4, "Loop.Closig.Keyframe.Database.Min.Size": 3, "numFeatures.trackingBad": 20, "Relocalization.Open": 1}


@pytest.fixture(scope="module")
def built():
    return host_util.build_test_binaries()


@pytest.fixture(scope="module")
def units(built):
    """tests/host/build/test_reloc_units, linked like the other unit binary"""
    from ssvio_amd import build as b
    src = os.path.join(host_util.ROOT, "tests", "host", "test_reloc_units.cpp")
    exe = os.path.join(host_util.OUT, "test_reloc_units")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(src), os.path.getmtime(built["host_lib"]))):
        rpath = ["-Wl,-rpath," + os.path.dirname(built["host_lib"]), "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib"]
        subprocess.check_call(["g++", *b.HOST_FLAGS, "-I", host_util.ROOT, src, built["host_lib"], b.LIB, "-lpthread", *rpath, "-o", exe])
    return exe


def run_cases(units, tmp_path, settings, cases, name="scenario.txt"):
    """cases = lists of (live, condemned, none, found, n_inliers) -> per case the dict of its printed lines"""
    lines = ["reset"] + ["setting %s %s" % kv for kv in settings.items()]
    for cands in cases:
        lines.append("case %d" % len(cands))
        lines += ["%d %d %d %d %d" % c for c in cands]
    path = os.path.join(str(tmp_path), name)
    open(path, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([units, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "case":
            out.append({})
        elif w[0] in ("query", "result", "record"):
            out[-1][w[0]] = dict(zip(w[1::2], w[2::2]))
        elif w[0] == "poses":
            out[-1]["poses"] = dict(jobs=int(w[4]), ranks=[int(x) for x in line.replace("[", " ").replace("]", " ").split()[5:][1::10]], line=line)
        elif w[0] == "error":
            out[-1]["error"] = line
    return out


# ---- 1. the premise ----------------------------------------------------------------------------------------------------------------
def test_the_interruption_ends_the_run_without_relocalisation(built, tmp_path):
    root = str(tmp_path)
    drive = reloc_drive.make_reloc_drive(root, **DRIVE)
    b, n = drive["b"], drive["n_frames"]
    # frame b + 3 against the last keyframe before the gap (frame b - 1): 4 steps of 0.25 baselines move a point at the median depth by
    # one median disparity (about 13 of 320 pixels): more than half the width is shared
    assert drive["overlap"] == pytest.approx(1.0 - 4 * DRIVE["step"] * drive["disp_med"] / 320) and drive["overlap"] >= 0.5, drive["overlap"]
    cfg = synth.write_settings(os.path.join(root, "cfg.yaml"), loop_drive.drive_settings(drive))
    r = subprocess.run([built["oracle_runner"], cfg, drive["dir"], os.path.join(root, "traj.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    log = host_util.parse_runner_log(r.stdout)
    status = [l["status"] for l in log]
    LOST = 3
    assert len(log) == n and LOST not in status[:b] and status[b:] == [LOST] * (n - b), status
    assert [l["keyframes"] for l in log[b:]] == [log[b - 1]["keyframes"]] * (n - b) and log[b - 1]["keyframes"] == b   # a keyframe per frame, none after b
    # Relocalization.Open: 1 on a Compute without loop closing: one warning, and the run is the same
    cfg2 = synth.write_settings(os.path.join(root, "cfg2.yaml"), loop_drive.drive_settings(drive, {"Relocalization.Open": 1}))
    r2 = subprocess.run([built["oracle_runner"], cfg2, drive["dir"], os.path.join(root, "traj2.txt")], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stderr.count("Relocalization.Open is set") == 1 and "Relocalization.Open is set" not in r.stderr
    strip = lambda text: [l for l in text.splitlines() if l.startswith("frame ")]
    assert strip(r2.stdout) == strip(r.stdout)
    assert open(os.path.join(root, "traj2.txt"), "rb").read() == open(os.path.join(root, "traj.txt"), "rb").read()


# ---- 2. LoopClosing::Relocalize ------------------------------------------------------------------------------------------------------
def test_settings_defaults_and_overrides(units, tmp_path):
    cand = [(30, 0, 0, 1, 25)]
    d = run_cases(units, tmp_path, BASE, [cand])[0]
    q = d["query"]
    # absent keys: 4 candidates, Loop.Threshold.Heigher, 0.75; the extractor and the levels of the loop step; class_id = feature index
    assert (int(q["K"]), float(q["threshold"]), float(q["ratio"]), int(q["levels"]), int(q["nfeatures"])) == (4, 0.5, 0.75, 4, 100)
    assert int(q["features"]) == 30 and int(q["class_last"]) == 29 and d["result"]["open"] == "1"
    over = dict(BASE, **{"Relocalization.Candidates": 8, "Relocalization.Threshold": 0.125, "Relocalization.Score.Ratio": 0.5})
    q = run_cases(units, tmp_path, over, [cand])[0]["query"]
    assert (int(q["K"]), float(q["threshold"]), float(q["ratio"])) == (8, 0.125, 0.5)
    # the bar: numFeatures.trackingBad when Relocalization.Min.Inliers is absent -- MORE than it
    for bad, n_in, ok in ((24, 25, "1"), (25, 25, "0")):
        assert run_cases(units, tmp_path, dict(BASE, **{"numFeatures.trackingBad": bad}), [[(30, 0, 0, 1, n_in)]])[0]["result"]["ok"] == ok
    for bar, n_in, ok in ((11, 12, "1"), (12, 12, "0")):
        d = run_cases(units, tmp_path, dict(BASE, **{"Relocalization.Min.Inliers": bar, "numFeatures.trackingBad": 0}), [[(30, 0, 0, 1, n_in)]])[0]
        assert d["result"]["ok"] == ok
    assert run_cases(units, tmp_path, dict(BASE, **{"Relocalization.Open": 0}), [cand])[0]["result"]["open"] == "0"
    del_open = {k: v for k, v in BASE.items() if k != "Relocalization.Open"}
    assert run_cases(units, tmp_path, del_open, [cand])[0]["result"]["open"] == "0"            # absent = off
    # settings outside the library's ranges are refused when relocalisation is on
    for kv in ({"Relocalization.Candidates": 0}, {"Relocalization.Candidates": 9}, {"Relocalization.Score.Ratio": 1.5}, {"Relocalization.Threshold": -0.1}):
        assert "Relocalization.Candidates must lie in [1, 8]" in run_cases(units, tmp_path, dict(BASE, **kv), [cand])[0]["error"], kv


CASES = [
    [(30, 0, 0, 1, 25), (40, 0, 0, 1, 35), (50, 0, 0, 1, 22)],          # the most refined inliers wins, whatever its rank
    [(30, 0, 0, 1, 25), (40, 0, 0, 1, 25)],                             # a tie: the lower rank
    [(9, 20, 5, 1, 9), (40, 0, 0, 1, 30)],                              # fewer than 10 pairs with a live, not condemned point: not asked
    [(10, 0, 30, 1, 10), (12, 0, 0, 0, 12)],                            # exactly 10 is asked; a job without a pose never wins
    [(30, 0, 0, 1, 20), (30, 0, 0, 1, 19)],                             # nobody above the bar of 20
    [(30, 0, 0, 1, 21), (5, 0, 0, 1, 5), (30, 0, 0, 1, 21), (30, 0, 0, 1, 22)],
    [(3, 0, 0, 1, 3)],                                                  # nothing to ask: no pose batch at all
    [],                                                                 # no candidate
    [(30, 0, 0, 1, 30)] * 6,                                            # more candidates than Relocalization.Candidates (4) admits
]


def test_acceptance_follows_the_model(units, tmp_path):
    out = run_cases(units, tmp_path, BASE, CASES)
    assert len(out) == len(CASES)
    for cands, d in zip(CASES, out):
        named = cands[:4]
        asked = [k for k, c in enumerate(named) if c[0] >= 10]
        results = [(c[4] if c[3] else None) if c[0] >= 10 else None for c in named]
        want = accept(results, BASE["numFeatures.trackingBad"])
        res, rec = d["result"], d["record"]
        assert int(res["candidates"]) == len(named) and int(res["pairs"]) == sum(c[0] + c[1] + c[2] for c in named)
        if asked:
            assert d["poses"]["jobs"] == len(asked) and d["poses"]["ranks"] == asked, (d["poses"], asked)
            # the seed is the loop step's (0) plus the rank; M counts the live, not condemned points; the frame's pixel, the keyframe's point
            for k in asked:
                assert "[rank %d M %d seed %d xyz0 0.0 uv0 0.5]" % (k, named[k][0], k) in d["poses"]["line"]
        else:
            assert "poses" not in d
        assert int(rec["poses"]) == len(asked) and int(rec["frame"]) == 42
        if want < 0:
            assert res["ok"] == "0" and res["kf"] == "-1" and rec["accepted"] == "-1" and int(res["matches"]) == 0
        else:
            # keyframe ids are the ranks here; the pose is the accepted job's (the script puts rank + 1 into tx)
            assert res["ok"] == "1" and int(res["kf"]) == want and float(res["tx"]) == want + 1.0 and int(rec["accepted"]) == want
            assert int(res["inliers"]) == named[want][4] == int(res["matches"])                    # the surviving pairs, each once
            first_point = sum(c[0] + c[1] for c in named[:want])
            assert res["first_match"] == "0:%d" % first_point                                      # the accepted keyframe's own map points
    assert [int(d["result"]["kf"]) for d in out] == [1, 0, 1, -1, -1, 3, -1, -1, 0]                # by hand, as a check on the check


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_batched_streams_with_relocalisation_are_refused(built, tmp_path):
    """before anything touches a device: the runner reads the settings and says why"""
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "seq", "image_0")); os.makedirs(os.path.join(root, "seq", "image_1"))
    open(os.path.join(root, "seq", "times.txt"), "w").write("")
    for over, flags, word in (({"Relocalization.Open": 1}, ("--streams=2", "--batched=1"), "Relocalization.Open"),
                              ({"Relocalization.Open": 1, "Loop.Closing.Open": 1}, ("--streams=2", "--batched=1", "--loop_batched=1"), "Relocalization.Open")):
        cfg = synth.write_settings(os.path.join(root, "cfg.yaml"), over)
        r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + os.path.join(root, "seq"), *flags], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and "--batched" in r.stderr and word in r.stderr and "not supported" in r.stderr, (r.returncode, r.stderr)
