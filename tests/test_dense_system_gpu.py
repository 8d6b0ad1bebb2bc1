"""Dense.Open in the headless system, end to end on the GPU, through ssx_run_kitti (ssvio_amd/host/frontend.cpp: FrontEnd::InsertKeyFrame;
system.cpp: System::SaveDenseCloud).

The drive is the one the undistortion and rectification system tests render: host_util.write_sequence at 320 x 200, a quarter baseline
per frame, a keyframe on every frame (tools/loop_drive.drive_settings), here 8 frames -- the smallest size and a frame count the existing
system tests use, so that the model (0.6 s a pair at 64 disparities) stays a few seconds for all keyframes."""
import glob
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import dense_model as dm
from tools import loop_drive
from tools import synth

pytestmark = pytest.mark.gpu

H, W, FX = 200, 320, 450.0
N_FRAMES = 8
DENSE = {"Dense.Open": 1, "Dense.Disparities": 64, "Dense.Cloud.Stride": 4, "Dense.Cloud.Max.Depth": 30.0}


@pytest.fixture(scope="module")
def built():
    return hu.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dense_drive"))
    seq = hu.write_sequence(root, n_frames=N_FRAMES, step=0.25, seed=0, h=H, w=W)
    return dict(root=root, seq=seq, drive=dict(K=(FX, FX, W / 2.0, H / 2.0), bf=synth.KITTI_BF))


def _run(built, world, tag, overrides, dense_out=False):
    root = world["root"]
    cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), loop_drive.drive_settings(world["drive"], overrides))
    out = dict(traj=os.path.join(root, tag + ".traj"), dir=os.path.join(root, tag + "_maps"), ply=os.path.join(root, tag + ".ply"))
    extra = []
    if dense_out:
        os.makedirs(out["dir"])
        extra = ["--dense_dir=" + out["dir"], "--dense_ply=" + out["ply"]]
    r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + world["seq"]["dir"], "--trajectory=" + out["traj"], *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out["stdout"] = r.stdout
    return out


def _bytes(path):
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def run_on(built, world):
    return _run(built, world, "on", DENSE, dense_out=True)


def _maps(run):
    files = sorted(glob.glob(os.path.join(run["dir"], "kf_*.disp16")))
    return files, [np.fromfile(f, dtype="<i2").reshape(H, W) for f in files]


def test_the_trajectory_is_the_bytes_of_the_run_without_the_key(built, world, run_on):
    off = _run(built, world, "off", {})
    assert len(np.loadtxt(off["traj"], ndmin=2)) >= 3                                 # at least three keyframes
    assert _bytes(run_on["traj"]) == _bytes(off["traj"])
    assert "dense (keyframe pair)" not in off["stdout"]
    line = [l for l in run_on["stdout"].splitlines() if "dense (keyframe pair)" in l]
    assert len(line) == 1 and int(line[0].split()[3]) == len(np.loadtxt(run_on["traj"], ndmin=2))   # one call per keyframe, timed under `dense`


def test_every_keyframes_map_is_the_models_and_the_cloud_counts_its_samples(world, run_on):
    tum = np.loadtxt(run_on["traj"], ndmin=2)
    files, maps = _maps(run_on)
    assert [os.path.basename(f) for f in files] == ["kf_%06d.disp16" % k for k in range(len(tum))]      # named by keyframe id, one per keyframe
    frame = np.rint(tum[:, 0] / world["seq"]["dt"]).astype(int)                      # the trajectory is in keyframe-id order
    prm = dm.DenseParams(disparities=64)
    bf = float(np.float32(FX)) * float(np.float32(synth.KITTI_BF) / np.float32(FX))   # fx * baseline as System reads them: float, widened
    n_samples = 0
    for k, f in enumerate(frame):
        L, R = world["seq"]["frames"][f]
        want = dm.disparity(L, R, prm)
        assert np.array_equal(maps[k], want), (k, f, int((maps[k] != want).sum()))
        assert (want > 0).mean() > 0.5
        n_samples += len(dm.cloud_samples(maps[k], L, DENSE["Dense.Cloud.Stride"], bf, DENSE["Dense.Cloud.Max.Depth"]))
    raw = _bytes(run_on["ply"])
    head, body = raw.split(b"end_header\n", 1)
    assert b"element vertex %d\n" % n_samples in head and len(body) == 13 * n_samples and n_samples > 1000
    assert "dense cloud: %d points" % n_samples in run_on["stdout"]
    pts = np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("i", "u1")]))
    assert np.isfinite(pts["xyz"]).all() and pts["xyz"][:, 2].max() <= DENSE["Dense.Cloud.Max.Depth"] + 1.0     # the rig moves sideways: depth stays z


def test_a_second_run_writes_the_same_bytes(built, world, run_on):
    again = _run(built, world, "again", DENSE, dense_out=True)
    assert _bytes(again["traj"]) == _bytes(run_on["traj"]) and _bytes(again["ply"]) == _bytes(run_on["ply"])
    fa, fb = _maps(again)[0], _maps(run_on)[0]
    assert len(fa) == len(fb) >= 3
    for a, b in zip(fa, fb):
        assert _bytes(a) == _bytes(b), os.path.basename(a)
