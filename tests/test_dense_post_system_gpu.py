"""Dense.Speckle.Size and Dense.Cloud.OnDevice in the headless system, end to end on the GPU, through ssx_run_kitti
(ssvio_amd/host/frontend.cpp: FrontEnd::InsertKeyFrame), on the small drive of test_dense_system_gpu.py: 320 x 200, 8
frames, a keyframe on every frame, 64 disparities.

The samples made on the device must give the PLY bytes of the samples made on the host, the filter must leave the trajectory alone (nothing
reads a keyframe's map), and the maps it writes are the model's filter applied to the maps of the unfiltered run."""
import glob
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import dense_post_model as pm
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
    root = str(tmp_path_factory.mktemp("dense_post_drive"))
    seq = hu.write_sequence(root, n_frames=N_FRAMES, step=0.25, seed=0, h=H, w=W)
    return dict(root=root, seq=seq, drive=dict(K=(FX, FX, W / 2.0, H / 2.0), bf=synth.KITTI_BF))


def _run(built, world, tag, overrides, maps=False):
    root = world["root"]
    cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), loop_drive.drive_settings(world["drive"], overrides))
    out = dict(traj=os.path.join(root, tag + ".traj"), dir=os.path.join(root, tag + "_maps"), ply=os.path.join(root, tag + ".ply"))
    extra = ["--dense_ply=" + out["ply"]]
    if maps:
        os.makedirs(out["dir"])
        extra.append("--dense_dir=" + out["dir"])
    r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + world["seq"]["dir"], "--trajectory=" + out["traj"], *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out["stdout"] = r.stdout
    return out


def _bytes(path):
    return open(path, "rb").read()


def _maps(run):
    files = sorted(glob.glob(os.path.join(run["dir"], "kf_*.disp16")))
    return [np.fromfile(f, dtype="<i2").reshape(H, W) for f in files]


@pytest.fixture(scope="module")
def run_plain(built, world):
    return _run(built, world, "plain", DENSE, maps=True)


def test_samples_made_on_the_device_write_the_plys_bytes(built, world, run_plain):
    on = _run(built, world, "on_device", dict(DENSE, **{"Dense.Cloud.OnDevice": 1}))              # no --dense_dir: no map comes down
    assert _bytes(on["ply"]) == _bytes(run_plain["ply"]) and len(_bytes(on["ply"])) > 13 * 1000
    assert _bytes(on["traj"]) == _bytes(run_plain["traj"])
    with_maps = _run(built, world, "on_device_maps", dict(DENSE, **{"Dense.Cloud.OnDevice": 1}), maps=True)
    assert _bytes(with_maps["ply"]) == _bytes(run_plain["ply"])
    a, b = _maps(with_maps), _maps(run_plain)
    assert len(a) == len(b) >= 3 and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("on_device", [0, 1])
def test_the_filter_leaves_the_trajectory_and_writes_the_models_maps(built, world, run_plain, on_device):
    keys = dict(DENSE, **{"Dense.Speckle.Size": 100, "Dense.Cloud.OnDevice": on_device})
    run = _run(built, world, "speckle%d" % on_device, keys, maps=True)
    assert _bytes(run["traj"]) == _bytes(run_plain["traj"])
    got, raw = _maps(run), _maps(run_plain)
    assert len(got) == len(raw) >= 3
    bf = float(np.float32(FX)) * float(np.float32(synth.KITTI_BF) / np.float32(FX))               # fx * baseline as System reads them: float, widened
    bar = pm.min_disp16(bf, DENSE["Dense.Cloud.Max.Depth"])
    n_samples, changed = 0, 0
    for k in range(len(raw)):
        want = pm.filter_speckles(raw[k], 100, 16)                                                  # Dense.Speckle.Range: 16 by default
        assert np.array_equal(got[k], want), (k, int((got[k] != want).sum()))
        changed += int((want != raw[k]).sum())
        n_samples += len(pm.samples(want, world["seq"]["frames"][0][0], 4, bar))                    # (only counted: the image does not matter)
    assert changed > 0
    head, body = _bytes(run["ply"]).split(b"end_header\n", 1)
    assert b"element vertex %d\n" % n_samples in head and len(body) == 13 * n_samples
    print(f"on_device {on_device}: {changed} pixels filtered over {len(raw)} keyframes, {n_samples} samples")
    assert changed > 1000 and len(body) < len(_bytes(run_plain["ply"]).split(b"end_header\n", 1)[1])   # the speckles left the cloud
