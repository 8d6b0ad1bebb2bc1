"""Camera.NeedUndistortion in the headless system, end to end on the GPU, through ssx_run_kitti (ssvio_amd/host/frontend.cpp:
FrontEnd::GrabSteroImage).

The drive (tools/undistort_drive.py): host_util.write_sequence at 320 x 200, 12 frames a quarter baseline apart, the camera of the loop
drives (fx = 450, a keyframe on every frame), warped by tools.undistort_model.distort_image with barrel coefficients that differ between
left and right.  Run A reads the distorted images with the key set; run B reads the model's undistorted images with the key 0.  Their
trajectories are the same bytes because the kernel writes the model's bytes.

The accuracy bar of run A against the ground-truth centres: the rectified drive's own largest centre error on this build plus
2 * z_med / fx (2 px at the median scene depth; the allowance of tests/test_reloc_system_gpu.py).  Measured on the MI355X: 0.1203 m against 0.1637 m + 0.1849 m
(profiles/undistort/drive.txt)."""
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import loop_drive
from tools import undistort_drive as drv

pytestmark = pytest.mark.gpu

ON = dict({"Camera.NeedUndistortion": 1}, **drv.coefficient_settings())
ZERO = {"Camera.NeedUndistortion": 1, "Camera1.k1": 0.0, "Camera1.k2": 0.0, "Camera1.p1": 0.0, "Camera1.p2": 0.0,
        "Camera2.k1": 0.0, "Camera2.k2": 0.0, "Camera2.p1": 0.0, "Camera2.p2": 0.0}


@pytest.fixture(scope="module")
def built():
    return hu.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("undistort_drive"))
    drives = drv.make_drives(root, hu.write_sequence, **drv.TEST_DRIVE)
    assert drives["all_taps_inside"]                                   # barrel: run B's images carry no black border
    return dict(root=root, drives=drives)


def _run(built, world, which, tag, overrides, extra=()):
    out = drv.run(built["run_kitti"], world["root"], world["drives"], which, tag, overrides, extra)
    assert out["r"].returncode == 0, (out["r"].stdout[-1500:], out["r"].stderr[-1500:])
    return out


def _bytes(path):
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def run_a(built, world):
    return _run(built, world, "dist", "a", ON)


@pytest.fixture(scope="module")
def run_b(built, world):
    return _run(built, world, "model", "b", {})


@pytest.fixture(scope="module")
def rect(built, world):
    return _run(built, world, "rect", "rect", {"Camera.NeedUndistortion": 0})


def test_zero_coefficients_write_the_rectified_runs_bytes(built, world, rect):
    zero = _run(built, world, "rect", "zero", ZERO)
    n = world["drives"]["n_frames"]
    assert len(np.loadtxt(rect["traj"], ndmin=2)) == n                 # a keyframe per frame
    assert _bytes(zero["traj"]) == _bytes(rect["traj"])
    assert "undistort (pair)" in zero["r"].stdout and "undistort (pair)" not in rect["r"].stdout
    # and with the key absent: a settings file of its own, the writer's default states the key
    settings = dict(hu.DEFAULT_CONFIG, **loop_drive.drive_settings(world["drives"]))
    assert settings.pop("Camera.NeedUndistortion") == 0
    cfg, traj = os.path.join(world["root"], "absent.yaml"), os.path.join(world["root"], "absent.traj")
    with open(cfg, "w") as f:
        f.write("%YAML:1.0\n" + "".join(f"{k}: {v}\n" for k, v in settings.items()))
    r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + world["drives"]["rect"], "--trajectory=" + traj],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert _bytes(traj) == _bytes(rect["traj"])


def test_distorted_input_with_the_key_equals_the_models_images_without(world, run_a, run_b, rect):
    n = world["drives"]["n_frames"]
    assert len(np.loadtxt(run_a["traj"], ndmin=2)) == n
    assert _bytes(run_a["traj"]) == _bytes(run_b["traj"])
    assert _bytes(run_a["traj"]) != _bytes(rect["traj"])               # the images were resampled: another run than the rectified one
    line = [l for l in run_a["r"].stdout.splitlines() if "undistort (pair)" in l]
    assert len(line) == 1 and int(line[0].split()[2]) == n             # one call per frame


def test_streams_and_the_remarshalling_backend(built, world, run_a):
    st = _run(built, world, "dist", "streams", ON, extra=("--streams=2",))
    for k in (0, 1):
        assert _bytes(st["traj"] + ".%d" % k) == _bytes(run_a["traj"]), k
    a0 = _run(built, world, "dist", "a_window0", dict(ON, **{"Backend.Window": 0}))
    b0 = _run(built, world, "model", "b_window0", {"Backend.Window": 0})
    assert _bytes(a0["traj"]) == _bytes(b0["traj"])


def test_accuracy_against_ground_truth(world, run_a, rect):
    """Run A is held to the ground-truth centres: the rectified drive's own largest error plus 2 px at the median scene depth."""
    drives = world["drives"]
    _, ea = drv.centre_errors(run_a["traj"], drives)
    _, er = drv.centre_errors(rect["traj"], drives)
    bar = float(er.max()) + drives["margin"]
    print("largest centre error: distorted + undistorted on the device %.4f m, rectified %.4f m, margin %.4f m, bar %.4f m" % (ea.max(), er.max(), drives["margin"], bar))
    assert drives["margin"] == pytest.approx(2 * drives["z_med"] / 450.0)
    assert float(ea.max()) <= bar


def test_batched_streams_are_refused_with_a_message(built, world):
    out = drv.run(built["run_kitti"], world["root"], world["drives"], "dist", "batched", ON, ("--streams=2", "--batched=1"))
    assert out["r"].returncode == 2
    assert "NeedUndistortion" in out["r"].stderr and "--batched=1" in out["r"].stderr
    assert not os.path.exists(out["traj"] + ".0")
