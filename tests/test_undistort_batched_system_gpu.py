"""Camera.NeedUndistortion for batched streams, end to end on the GPU, through ssx_run_kitti --batched=C --undistort_batched=1
(ssvio_amd/host/stream_batcher.cpp: the UND request kind, one ssx_undistort_plan_apply per frame for a cohort).

The drive is tools/undistort_drive.py's (320 x 200, 12 frames, a keyframe on every frame).  Every stream of a batched cohort that
reads the distorted images with the key set writes the bytes of the single-stream run with the key, which are the bytes of the run on
the model's undistorted images with the key 0 (runs A and B of tests/test_undistort_system_gpu.py, made again here)."""
import os
import re

import numpy as np
import pytest

import host_util as hu
from tools import undistort_drive as drv

pytestmark = pytest.mark.gpu

ON = dict({"Camera.NeedUndistortion": 1}, **drv.coefficient_settings())


@pytest.fixture(scope="module")
def built():
    return hu.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("undistort_batched_drive"))
    return dict(root=root, drives=drv.make_drives(root, hu.write_sequence, **drv.TEST_DRIVE))


def _run(built, world, which, tag, overrides, extra=()):
    out = drv.run(built["run_kitti"], world["root"], world["drives"], which, tag, overrides, extra)
    assert out["r"].returncode == 0, (out["r"].stdout[-1500:], out["r"].stderr[-1500:])
    return out


def _bytes(path):
    return open(path, "rb").read()


@pytest.fixture(scope="module")
def run_a(built, world):
    """the single stream on the distorted images, the key set"""
    return _run(built, world, "dist", "a", ON)


@pytest.fixture(scope="module")
def run_b(built, world):
    """the single stream on the model's undistorted images, the key 0"""
    return _run(built, world, "model", "b", {})


def _undistort_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("batched calls: undistort ")]
    assert len(lines) == 1, stdout[-2000:]
    m = re.match(r"batched calls: undistort (\d+) \(([0-9.]+) jobs each\)", lines[0])
    assert m, lines[0]
    return int(m.group(1)), float(m.group(2)), int(re.search(r"und_jobs (\d+)", lines[0]).group(1))


@pytest.mark.parametrize("streams, cohorts", [(3, 1), (4, 2)])
def test_every_batched_stream_writes_the_single_streams_bytes(built, world, run_a, run_b, streams, cohorts):
    n = world["drives"]["n_frames"]
    assert _bytes(run_a["traj"]) == _bytes(run_b["traj"])                 # the kernel writes the model's bytes
    assert len(np.loadtxt(run_a["traj"], ndmin=2)) == n                   # not vacuous: a keyframe on every frame
    out = _run(built, world, "dist", "batched_%d_%d" % (streams, cohorts), ON,
               ("--streams=%d" % streams, "--batched=%d" % cohorts, "--undistort_batched=1"))
    for k in range(streams):
        assert _bytes(out["traj"] + ".%d" % k) == _bytes(run_a["traj"]), k
        assert len(np.loadtxt(out["traj"] + ".%d" % k, ndmin=2)) == n
    # the counters are reset after the streams' warm-up: they describe the frames alone, two jobs per stream and frame
    calls, each, jobs = _undistort_line(out["r"].stdout)
    assert jobs == 2 * streams * n and calls >= 1
    assert each == pytest.approx(jobs / calls, abs=0.051)
    assert "batched calls: LK " in out["r"].stdout                        # the line other tests parse keeps its text


def test_with_the_key_0_the_flag_changes_nothing(built, world):
    plain = _run(built, world, "model", "plain_batched", {}, ("--streams=2", "--batched=1"))
    flag = _run(built, world, "model", "flag_batched", {}, ("--streams=2", "--batched=1", "--undistort_batched=1"))
    for k in (0, 1):
        assert _bytes(flag["traj"] + ".%d" % k) == _bytes(plain["traj"] + ".%d" % k), k
    assert "batched calls: undistort" not in flag["r"].stdout


def test_the_flag_without_batched_is_refused(built, world):
    for extra in (("--undistort_batched=1",), ("--streams=2", "--undistort_batched=1"), ("--streams=2", "--batched=0", "--undistort_batched=1")):
        out = drv.run(built["run_kitti"], world["root"], world["drives"], "dist", "flag_alone", ON, extra)
        assert out["r"].returncode == 2, extra
        assert "--undistort_batched=1" in out["r"].stderr and "--batched" in out["r"].stderr
        assert not os.path.exists(out["traj"]) and not os.path.exists(out["traj"] + ".0")
