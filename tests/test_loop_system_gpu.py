"""Loop closing in the headless system, end to end on the GPU, through ssx_run_kitti (ssvio_amd/host/loopclosing.cpp).

The drive (tools/loop_drive.py): tools.synth.make_lateral_sequence at 320 x 200 with a camera of fx = 450 (Camera.Base.Line / fx = 0.858 m),
a keyframe on every frame (numFeatures.trackingGood above any count), Map.ActiveMap.Size 5.  24 frames out to 7 baselines (6.0 m) on half a
cosine, then the outbound LEFT images in reverse (47 frames), the return leg's RIGHT images rendered 2.2 baselines beside the left camera
while the settings keep stating one: every map point of the return leg is 2.2 times too near, the leg is measured too short, and the
trajectory ends beside its start.

  open-loop end-point error (loop closing off):  5.256 on the CPU oracle (tests/host/build/oracle_runner), 5.299 on the MI355X
  -- inside the [2, 10] the drive was chosen for (twice the lower gate of loopclosing.cpp:226, two thirds of the upper).
  Other parameters of the one sweep on the GPU (fx, reach, factor -> open-loop error -> with loop closing): 450, 7, 1.5 -> 4.16 -> 1.19;
  250, 7, 1.5 -> 9.28 -> 0.02; 250, 7, 2.2 -> 10.03 (outside); 450, 4, 2.2 -> 1.56 (outside).  Chosen: 450, 7, 2.2 -> 5.30 -> 0.05.

What this scene cannot do, and what follows from it.  make_lateral_sequence slides ONE image-wide texture under a depth map that is fixed to
the image, so the world ends where that image ends and no leg can be longer than a view width: the view width at the scene's median depth
is 21.6 m, the reach 6.0 m.  "Half a view width" (assertion 1) is therefore 10.8 m, wider than the whole drive; the test asserts the sharper
fact that the loop keyframe of a correction is the keyframe that showed the SAME outbound image or its neighbour (centres < 0.5 m apart).

Loop.Threshold.Heigher = 0.5 for this drive and make_vocabulary(k=10, L=3), from the scores the first GPU runs logged (threshold 0.3, where
every candidate is reported):
  best score of a true revisit (the same outbound image, centres 0.00 m apart):  0.706 (keyframe 27 -> 19); the corrections close at 0.523 and 0.575
  best score of a pair more than 5 m apart (the farthest the drive offers):       0.498 (keyframe 28 -> 2, 5.22 m)
Loop.Min.Keyframe.Gap 8, Loop.Closig.Keyframe.Database.Min.Size 3, Pyramid.Level 4.
With them the first run closed twice (keyframe 38 -> 8 with error 3.96, 45 -> 1 with 1.35) and ended 0.048 from the truth."""
import os
import subprocess

import numpy as np
import pytest

import host_util
from tools import loop_drive, synth

pytestmark = pytest.mark.gpu

DRIVE = dict(n_leg=24, reach=7.0, right_factor=2.2, fx=450.0)
LOOP = {"Loop.Closing.Open": 1, "Loop.Show.Closing.Result": 0, "Loop.Threshold.Heigher": 0.5, "Loop.Threshold.Lower": 0.02, "Pyramid.Level": 4,
        "Loop.Closig.Keyframe.Database.Min.Size": 3, "Loop.Min.Keyframe.Gap": 8}


@pytest.fixture(scope="module")
def built():
    return host_util.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("loop_drive"))
    drive = loop_drive.make_loop_drive(root, **DRIVE)
    voc = os.path.join(root, "voc.txt")
    synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
    return dict(root=root, drive=drive, voc=voc)


def _run(built, world, tag, overrides, extra=(), loop=True, check=True):
    root, drive = world["root"], world["drive"]
    over = dict(LOOP, **{"DBOW2.VOC.Path": '"%s"' % world["voc"]}) if loop else {}
    over.update(overrides)
    cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), loop_drive.drive_settings(drive, over))
    traj, log = os.path.join(root, tag + ".traj"), os.path.join(root, tag + ".looplog")
    r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + drive["dir"], "--trajectory=" + traj, "--loop_log=" + log, *extra],
                       capture_output=True, text=True, timeout=120)
    if check:
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return dict(r=r, traj=traj, log=log)


def _lines(path):
    out = []
    for l in open(path):
        w = l.split()
        out.append(dict(zip(w[0::2], w[1::2])))
    return out


@pytest.fixture(scope="module")
def closed(built, world):
    return _run(built, world, "closed", {})


@pytest.fixture(scope="module")
def open_loop(built, world):
    return _run(built, world, "open", {"Loop.Closing.Open": 0})


def test_the_loop_is_closed(world, closed, open_loop):
    """1. the drift of the open-loop run (>= 2) is gone after a correction onto the keyframe of the same place (< 1: the gate under which the
    reference itself declines to correct)"""
    drive = world["drive"]
    e_open = loop_drive.end_point_error(open_loop["traj"], drive)[0]
    e_closed, _, _, frames = loop_drive.end_point_error(closed["traj"], drive)
    lines = _lines(closed["log"])
    print("open-loop end-point error", e_open, "with loop closing", e_closed)
    for l in lines:
        if l["found"] == "1":
            print({k: l[k] for k in ("kf", "loop", "score", "pairs", "pose", "with_point", "inliers", "error", "corrected", "fused", "same_point", "duplicate")})
    assert len(frames) == drive["n_frames"] and not os.path.exists(open_loop["log"])
    assert 2.0 <= e_open <= 10.0
    corrected = [l for l in lines if l["corrected"] == "1"]
    assert corrected, "no keyframe was corrected"
    for l in corrected:
        dist = float(np.linalg.norm(drive["centres"][int(l["kf"])] - drive["centres"][int(l["loop"])]))
        assert dist < 0.5 * drive["view_width"] and dist < 0.5, (l["kf"], l["loop"], dist)
        assert l["need_correct"] == "1" and 1.0 < float(l["error"]) < 15.0 and int(l["pg_iters"]) > 0 and int(l["moved_active"]) > 0 and int(l["moved_other"]) > 0
    assert e_closed < 1.0
    # a confirmed keyframe is not added to the database, and the five after it are not looked at
    ids = [int(l["kf"]) for l in lines]
    for a, b in zip(lines, lines[1:]):
        confirmed = a["pose"] == "0"
        assert int(b["db"]) == int(a["db"]) + (0 if confirmed else 1)
        assert int(b["kf"]) - int(a["kf"]) == (6 if confirmed else 1)
    assert ids[0] == 0


def test_resident_window_and_marshalled_map_agree(built, world, closed):
    """2. Backend.Window: 1 and 0 write the same bytes through a correction; Backend.Window.Check finds the window equal to the map"""
    w0 = _run(built, world, "window0", {"Backend.Window": 0})
    assert open(w0["traj"], "rb").read() == open(closed["traj"], "rb").read()
    assert open(w0["log"], "rb").read() == open(closed["log"], "rb").read()
    chk = _run(built, world, "check", {"Backend.Window.Check": 1})
    assert open(chk["traj"], "rb").read() == open(closed["traj"], "rb").read()
    assert any(l["corrected"] == "1" for l in _lines(chk["log"]))


def test_two_runs_are_identical(built, world, closed):
    """3."""
    again = _run(built, world, "again", {})
    assert open(again["traj"], "rb").read() == open(closed["traj"], "rb").read()
    assert open(again["log"], "rb").read() == open(closed["log"], "rb").read()


def test_loop_closing_off_is_the_system_without_it(built, world, open_loop):
    """4. Loop.Closing.Open: 0 and a settings file without any loop key"""
    bare = _run(built, world, "bare", {}, loop=False)
    assert open(bare["traj"], "rb").read() == open(open_loop["traj"], "rb").read()
    assert not os.path.exists(bare["log"]) and "loop closing" not in bare["r"].stdout


def test_both_threads(built, world):
    """5. the loop thread beside the backend's thread: finishes, every keyframe written with a unit quaternion, a loop found.  No bit claims."""
    a = _run(built, world, "async", {"Loop.Closing.Async": 1, "Backend.Async": 1})
    tum = np.loadtxt(a["traj"], ndmin=2)
    assert tum.shape == (world["drive"]["n_frames"], 8) and np.isfinite(tum).all()
    assert np.abs(np.linalg.norm(tum[:, 4:8], axis=1) - 1).max() < 1e-5
    assert any(l["found"] == "1" for l in _lines(a["log"]))
    assert "loop closing (own thread)" in a["r"].stdout


def test_misuse(built, world, closed):
    """6."""
    bad = _run(built, world, "novoc", {"DBOW2.VOC.Path": '"%s"' % os.path.join(world["root"], "no_such_vocabulary.txt")}, check=False)
    assert bad["r"].returncode != 0 and "DBOW2.VOC.Path" in bad["r"].stderr
    ref = _run(built, world, "batched", {}, extra=("--streams=2", "--batched=1"), check=False)
    assert ref["r"].returncode != 0 and "--batched" in ref["r"].stderr and "Loop.Closing.Open" in ref["r"].stderr
    # unbatched streams: each has its own LoopClosing and writes the single stream's bytes
    st = _run(built, world, "streams", {}, extra=("--streams=2",))
    for k in (0, 1):
        assert open(st["traj"] + f".{k}", "rb").read() == open(closed["traj"], "rb").read()
        assert open(st["log"] + f".{k}", "rb").read() == open(closed["log"], "rb").read()
