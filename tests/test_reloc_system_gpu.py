"""Relocalisation in the headless system, end to end on the GPU, through ssx_run_kitti (ssvio_amd/host/frontend.cpp: FrontEnd::Relocalize,
loopclosing.cpp: LoopClosing::Relocalize).

The drive (tools/reloc_drive.py): tools.synth.make_lateral_sequence at 320 x 200 with the camera and settings of the loop-closing drive
(fx = 450, a keyframe on every frame, Map.ActiveMap.Size 5), 16 frames a quarter baseline apart.  Frames 8, 9 and 10 are constant grey in
both images: tests/test_reloc_host.py shows on the CPU oracle that tracking is lost at frame 8 and that the run is over there.  Frame 11 shares
96 % of its view with the last keyframe (frame 7).  Loop closing is on with the settings of tests/test_loop_system_gpu.py and a keyframe gap
the drive never reaches: every keyframe enters the database, no loop is looked for.

The accuracy bar: over the keyframes after recovery the largest centre error may exceed that of the SAME drive uninterrupted
(the unblanked images, the key absent) on those frames by at most the translation 2 px of reprojection error mean at the scene's median
depth, 2 * z_med / fx = 2 * 30.35 / 450 = 0.135 m -- the relocalised pose rests on a few dozen keypoint matches at pixel precision, not on
LK's sub-pixel tracks.  Measured on the MI355X: 0.2163 relocalised against 0.2316 uninterrupted (profiles/reloc/drive.txt)."""
import os

import numpy as np
import pytest

import host_util
from tools import reloc_drive, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    return host_util.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("reloc_drive"))
    drive = reloc_drive.make_reloc_drive(root, **reloc_drive.TEST_DRIVE)
    clean = reloc_drive.make_reloc_drive(root, blank=None, tag="clean", **reloc_drive.TEST_DRIVE)
    voc = os.path.join(root, "voc.txt")
    synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
    return dict(root=root, drive=drive, clean=clean, voc=voc)


def _run(built, world, tag, overrides, extra=(), drive="drive"):
    out = reloc_drive.run_drive(built["run_kitti"], world["root"], world[drive], world["voc"], tag, overrides, extra)
    assert out["r"].returncode == 0, (out["r"].stdout[-1500:], out["r"].stderr[-1500:])
    return out


def _bytes(path):
    return open(path, "rb").read()


def _frames(traj, drive):
    return [int(f) for f in reloc_drive.centre_errors(traj, drive)[0]]


def _reloc_lines(path):
    out = []
    for l in open(path):
        w = l.split()
        if w[0] == "reloc_frame":
            out.append({k: int(v) for k, v in zip(w[0::2], w[1::2])})
    return out


@pytest.fixture(scope="module")
def absent(built, world):
    return _run(built, world, "absent", {})


@pytest.fixture(scope="module")
def on(built, world):
    return _run(built, world, "on", {"Relocalization.Open": 1})


def test_off_is_todays_run(built, world, absent):
    """the key absent and Relocalization.Open: 0 write the same bytes, and the run is over at frame b"""
    drive = world["drive"]
    b = drive["b"]
    zero = _run(built, world, "zero", {"Relocalization.Open": 0})
    assert _bytes(zero["traj"]) == _bytes(absent["traj"]) and _bytes(zero["log"]) == _bytes(absent["log"])
    for run in (absent, zero):
        assert "final status LOST" in run["r"].stdout and "frame %d: tracking lost" % b in run["r"].stderr
        assert "relocalisation" not in run["r"].stderr and "reloc_frame" not in open(run["log"]).read()
    assert _frames(absent["traj"], drive) == list(range(b))      # a keyframe per frame before b, none after


def test_the_front_end_recovers(world, on):
    drive = world["drive"]
    b, n, first = drive["b"], drive["n_frames"], drive["b"] + drive["n_blank"]
    err = on["r"].stderr
    assert "frame %d: tracking lost" % b in err
    rel = _reloc_lines(on["log"])
    print(err)
    # one attempt per frame from b + 1 on, until one is accepted: at the first restored frame, and not more than one frame later
    ok = [l for l in rel if l["accepted"] >= 0]
    assert len(ok) == 1 and ok[0]["reloc_frame"] in (first, first + 1), rel
    got = ok[0]["reloc_frame"]
    assert [l["reloc_frame"] for l in rel] == list(range(b + 1, got + 1))
    assert all(l["candidates"] == 0 for l in rel if l["reloc_frame"] < first)        # a grey image has no features to ask with
    assert ok[0]["inliers"] > 10 and ok[0]["poses"] >= 1 and 0 <= ok[0]["accepted"] < b   # more than numFeatures.trackingBad, against a keyframe from before the gap
    assert err.count("relocalisation succeeded") == 1 and err.count("relocalisation failed") == len(rel) - 1
    assert "final status LOST" not in on["r"].stdout
    # keyframes are inserted from the relocalised frame on
    assert _frames(on["traj"], drive) == list(range(b)) + list(range(got, n))
    tum = np.loadtxt(on["traj"], ndmin=2)
    assert np.isfinite(tum).all() and np.abs(np.linalg.norm(tum[:, 4:8], axis=1) - 1).max() < 1e-5


def test_accuracy_against_the_uninterrupted_drive(built, world, on):
    drive = world["drive"]
    clean = _run(built, world, "clean", {}, drive="clean")                           # the unblanked images, the key absent: the code as it stood
    assert _frames(clean["traj"], world["clean"]) == list(range(drive["n_frames"]))
    got = [l for l in _reloc_lines(on["log"]) if l["accepted"] >= 0][0]["reloc_frame"]
    e_reloc, e_clean, margin = reloc_drive.accuracy(on["traj"], clean["traj"], drive, got)
    print("largest centre error after recovery: relocalised %.4f, uninterrupted %.4f, margin %.4f" % (e_reloc, e_clean, margin))
    assert margin == pytest.approx(2 * drive["z_med"] / 450.0) and 0.1 < margin < 0.2
    assert e_reloc <= e_clean + margin


def test_window_and_map_agree_and_runs_repeat(built, world, on):
    """Backend.Window.Check: 1 stays silent (the resident window equals the re-marshalled map after the relocalised keyframe, whose map points
    come back into the window); Backend.Window: 1 and 0 write the same bytes; two runs are byte-identical"""
    for tag, over in (("check", {"Backend.Window.Check": 1}), ("window0", {"Backend.Window": 0}), ("again", {})):
        r = _run(built, world, tag, dict({"Relocalization.Open": 1}, **over))
        assert _bytes(r["traj"]) == _bytes(on["traj"]) and _bytes(r["log"]) == _bytes(on["log"]), tag


def test_the_loop_thread_and_unbatched_streams(built, world, on):
    drive = world["drive"]
    b, n = drive["b"], drive["n_frames"]
    # the loop thread beside the front-end: the keyframes may reach the database a little later, so no bit claims -- it recovers
    a = _run(built, world, "async", {"Relocalization.Open": 1, "Loop.Closing.Async": 1})
    frames = _frames(a["traj"], drive)
    assert "final status LOST" not in a["r"].stdout and frames[:b] == list(range(b)) and len(frames) > b and frames[-1] == n - 1
    assert any(l["accepted"] >= 0 for l in _reloc_lines(a["log"]))
    # unbatched streams: each has its own LoopClosing and writes the single stream's bytes
    st = _run(built, world, "streams", {"Relocalization.Open": 1}, extra=("--streams=2",))
    for k in (0, 1):
        assert _bytes(st["traj"] + ".%d" % k) == _bytes(on["traj"]) and _bytes(st["log"] + ".%d" % k) == _bytes(on["log"])
