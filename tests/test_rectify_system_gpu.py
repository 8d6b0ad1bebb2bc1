"""Camera.Rectify in the headless system, end to end on the GPU, through ssx_run_kitti (ssvio_amd/host/system.cpp: the raw rig rectified by
ssx_stereo_rectify; frontend.cpp: FrontEnd::GrabSteroImage; stream_batcher.cpp: the UND request kind).

The drive (tools/rectify_drive.py): host_util.write_sequence at 320 x 200, 12 frames a quarter baseline apart, rendered in the rectified
rig of a raw rig -- a kb4 left camera, a radtan right camera, rot(1.5, -2, 1 degrees) between them -- and warped out into what the raw
cameras see.  Run A reads the raw images with the key set; run B reads the contract's rectification of them with the rectified
intrinsics and the key off.  Their trajectories are the same bytes because both lens branches of the kernel write the model's bytes and
ssx_stereo_rectify returns the model's camera.

The accuracy bar of run A against the ground-truth centres (in the rectified left frame): the rectified drive's own largest centre error on
this build plus 2 * z_med / f (2 px at the median scene depth; the allowance of tests/test_undistort_system_gpu.py).  The figures
are in profiles/rectify/drive.txt."""
import os

import numpy as np
import pytest

import host_util as hu
from tools import rectify_drive as drv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    return hu.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("rectify_drive"))
    drives = drv.make_drives(root, hu.write_sequence, **drv.TEST_DRIVE)
    assert drives["all_taps_inside"]                                   # run B's images carry no black border
    assert drives["exact_baseline"]                                    # the two runs triangulate with one baseline
    return dict(root=root, drives=drives, on=dict({"Camera.Rectify": 1}, **drives["settings"]))


def _run(built, world, which, tag, overrides, extra=()):
    out = drv.run(built["run_kitti"], world["root"], world["drives"], which, tag, overrides, extra)
    assert out["r"].returncode == 0, (out["r"].stdout[-1500:], out["r"].stderr[-1500:])
    return out


def _bytes(path):
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def run_a(built, world):
    return _run(built, world, "raw", "a", world["on"])


def test_raw_input_with_the_key_equals_the_models_images_without(built, world, run_a):
    n = world["drives"]["n_frames"]
    run_b = _run(built, world, "model", "b", {})
    assert len(np.loadtxt(run_a["traj"], ndmin=2)) == n                # a keyframe per frame
    assert _bytes(run_a["traj"]) == _bytes(run_b["traj"])
    line = [l for l in run_a["r"].stdout.splitlines() if "undistort (pair)" in l]
    assert len(line) == 1 and int(line[0].split()[2]) == n             # one call per frame, timed under `undistort`
    note = [l for l in run_a["r"].stdout.splitlines() if l.startswith("Camera.Rectify:")]
    assert len(note) == 1 and "R_l = [" in note[0] and "Camera.Base.Line is ignored" in note[0]
    assert "Camera.Rectify:" not in run_b["r"].stdout and "undistort (pair)" not in run_b["r"].stdout
    # the raw images read as if they were rectified are another run altogether
    wrong = drv.run(built["run_kitti"], world["root"], world["drives"], "raw", "wrong", {})
    assert wrong["r"].returncode != 0 or not os.path.exists(wrong["traj"]) or _bytes(wrong["traj"]) != _bytes(run_a["traj"])


def test_accuracy_against_ground_truth(built, world, run_a):
    """Run A is held to the ground-truth centres: the rectified drive's own largest error plus 2 px at the median scene depth."""
    drives = world["drives"]
    rect = _run(built, world, "rect", "rect", {})
    _, ea = drv.centre_errors(run_a["traj"], drives)
    _, er = drv.centre_errors(rect["traj"], drives)
    bar = float(er.max()) + drives["margin"]
    print("largest centre error: raw + rectified on the device %.4f m, rectified drive %.4f m, margin %.4f m, bar %.4f m" % (ea.max(), er.max(), drives["margin"], bar))
    assert drives["margin"] == pytest.approx(2 * drives["z_med"] / 450.0)
    assert float(ea.max()) <= bar


def test_batched_streams_write_the_single_streams_bytes(built, world, run_a):
    out = _run(built, world, "raw", "batched", world["on"], ("--streams=2", "--batched=1", "--undistort_batched=1"))
    n = world["drives"]["n_frames"]
    for k in (0, 1):
        assert _bytes(out["traj"] + ".%d" % k) == _bytes(run_a["traj"]), k
    line = [l for l in out["r"].stdout.splitlines() if l.startswith("batched calls: undistort ")]
    assert len(line) == 1 and "und_jobs %d " % (2 * 2 * n) in line[0]  # two jobs per stream and frame through the stored maps


def test_batched_streams_without_the_flag_are_refused_with_a_message(built, world):
    out = drv.run(built["run_kitti"], world["root"], world["drives"], "raw", "refused", world["on"], ("--streams=2", "--batched=1"))
    assert out["r"].returncode == 2
    assert "Camera.Rectify" in out["r"].stderr and "--undistort_batched=1" in out["r"].stderr and "--batched=1" in out["r"].stderr
    assert not os.path.exists(out["traj"] + ".0")
