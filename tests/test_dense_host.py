"""CPU: the host path of Dense.Open on a Compute that records what it is asked (tests/host/test_dense_units.cpp): with the key on,
FrontEnd::InsertKeyFrame calls Compute::DenseDisparity once per keyframe with the frame's own pair and the settings' parameters, the
keyframe keeps exactly the stride, validity and depth-bar pixels, System::SaveDenseCloud writes the header count it writes rows for and
its points are the stated formula, a Compute without dense stereo is refused at construction, the runner refuses --batched=1 with the
key, and with no Dense.* key nothing new is called."""
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import dense_model as dm

ROWS, COLS = 64, 96
DENSE = {"Dense.Open": 1, "Dense.Disparities": 64, "Dense.P1": 5, "Dense.P2": 70, "Dense.Uniqueness": 15, "Dense.LR.Tolerance": 2, "Dense.Paths": 4,
         "Dense.Cloud.Stride": 3, "Dense.Cloud.Max.Depth": 25.5}
BASE = {"Backend.Open": 0, "Camera1.cx": 48.0, "Camera1.cy": 32.0, "Camera2.cx": 48.0, "Camera2.cy": 32.0}


def stub_disparity(call):
    v, u = np.mgrid[0:ROWS, 0:COLS]
    return np.where((u * 7 + v * 13 + call) % 11 == 0, -16, 16 + (u * 5 + v * 3 + 40 * call) % 900).astype(np.int16)


def stub_image(salt):
    i = np.arange(ROWS * COLS, dtype=np.int64)
    return ((i * 31 + salt * 17) % 251).astype(np.uint8).reshape(ROWS, COLS)


def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar intensity"]
    n = int(lines[2].split()[-1])
    assert lines[2] == f"element vertex {n}"
    return n, np.frombuffer(body, dtype=np.dtype([("xyz", "<f4", 3), ("i", "u1")]))


@pytest.fixture(scope="module")
def built():
    from ssvio_amd import build as b
    host_lib, run_kitti = b.build_host()
    return dict(b=b, host_lib=host_lib, run_kitti=run_kitti)


@pytest.fixture(scope="module")
def report(built, tmp_path_factory):
    b, host_lib = built["b"], built["host_lib"]
    root = str(tmp_path_factory.mktemp("dense_host"))
    exe = os.path.join(root, "test_dense_units")
    src = os.path.join(hu.ROOT, "tests", "host", "test_dense_units.cpp")
    rpath = ["-Wl,-rpath," + os.path.dirname(host_lib), "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(["g++", *b.HOST_FLAGS, "-I", hu.ROOT, src, host_lib, b.LIB, "-lpthread", *rpath, "-o", exe])
    on = hu.write_config(os.path.join(root, "on.yaml"), dict(BASE, **DENSE))
    off = hu.write_config(os.path.join(root, "off.yaml"), dict(BASE))
    ply_on, ply_off = os.path.join(root, "on.ply"), os.path.join(root, "off.ply")
    r = subprocess.run([exe, on, off, ply_on, ply_off], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = {}
    for l in r.stdout.splitlines():
        w = l.split()
        if w and w[0] in ("on_kf", "on_samples"):
            rep.setdefault(w[0], {})[int(w[1])] = w[2:]
        elif w:
            rep[w[0]] = w[1:]
    rep["ply_on"], rep["ply_off"] = ply_on, ply_off
    return rep


def test_refusals_name_the_key(report):
    assert report["refused"] == ["1"] and report["default_throws"] == ["1"]


def test_one_call_per_keyframe_with_the_frames_pair_and_the_settings_parameters(report):
    n = int(report["on_keyframes"][0])
    assert n == 4 and report["on_dense_calls"] == [str(n)] and report["on_stopwatch"] == [str(n)] and report["on_sink"] == [str(n), "1"]
    for c in range(n):
        assert report[f"on_call{c}"] == [str(1001 + 2 * c), str(1002 + 2 * c), "64", "5", "70", "15", "2", "4", "0", "0"], c
        assert report["on_kf"][c][0] == str(c)                                     # keyframe c is frame c: every frame became one
    assert report["on_cloud_config"] == ["3", "25.5"]
    assert report["on_warmup_calls"] == ["1"] and report["on_stopwatch_after_warmup"] == [str(n)]   # warmed outside the phase's clock


def _want_samples(report, c):
    fx, _, _, _, baseline = (float(v) for v in report["on_camera"])
    return dm.cloud_samples(stub_disparity(c), stub_image(c), 3, fx * baseline, 25.5)


def test_the_keyframe_keeps_exactly_the_stride_validity_and_depth_pixels(report):
    fx, _, _, _, baseline = (float(v) for v in report["on_camera"])
    assert fx == float(np.float32(718.856)) and baseline == float(np.float32(386.1448) / np.float32(718.856))
    kinds = set()
    for c in range(4):
        got = np.array([int(v) for v in report["on_samples"][c]], dtype=np.int64).reshape(-1, 4)
        want = _want_samples(report, c)
        assert np.array_equal(got, want), c
        assert len(got) > 50 and np.all(got[:, 0] % 3 == 0) and np.all(got[:, 1] % 3 == 0)
        d = stub_disparity(c)[::3, ::3]
        kinds |= {"invalid"} if (d == -16).any() else set()
        kinds |= {"too_far"} if ((d > 0) & (fx * baseline * 16.0 / np.where(d > 0, d, 1) > 25.5)).any() else set()
        assert len(got) < d.size
    assert kinds == {"invalid", "too_far"}                                            # both filters had something to remove


def test_the_cloud_is_the_stated_formula_with_the_final_poses(report):
    n, pts = read_ply(report["ply_on"])
    assert report["on_cloud_points"] == [str(n)] and len(pts) == n and n == sum(len(_want_samples(report, c)) for c in range(4))
    fx, fy, cx, cy, baseline = (np.float64(v) for v in report["on_camera"])
    bf = fx * baseline
    want_xyz, want_i = [], []
    for c in range(4):
        q = np.array([float(v) for v in report["on_kf"][c][1:]], dtype=np.float64)   # T_cw as it was when the cloud was written: qx qy qz qw tx ty tz
        x, y, z, w = q[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        s = _want_samples(report, c).astype(np.float64)
        zc = bf * 16.0 / s[:, 2]
        Xc = np.stack([(s[:, 0] - cx) * zc / fx, (s[:, 1] - cy) * zc / fy, zc], 1)
        want_xyz.append((Xc - q[4:]) @ R)                                             # T_wc Xc = R^T (Xc - t)
        want_i.append(s[:, 3])
    want = np.concatenate(want_xyz).astype(np.float32)
    assert np.array_equal(pts["i"], np.concatenate(want_i).astype(np.uint8))
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(pts["xyz"].astype(np.float64) - want.astype(np.float64)) <= ulp), "more than 1 ulp of float off the formula"
    assert np.abs(want).max() > 5.0


def test_without_the_keys_nothing_new_is_called(report):
    for can in "01":
        assert report[f"off{can}"] == ["4", "0", "0", "0", "0"], can
        assert report[f"off{can}_defaults"] == ["128", "7", "86", "10", "1", "8", "4", "40"], can
    n, pts = read_ply(report["ply_off"])
    assert n == 0 and len(pts) == 0


def test_the_runner_refuses_batched_streams_with_the_key(built, tmp_path):
    """before anything touches a device: the runner reads the settings and says why"""
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "seq", "image_0")); os.makedirs(os.path.join(root, "seq", "image_1"))
    open(os.path.join(root, "seq", "times.txt"), "w").write("")
    cfg = hu.write_config(os.path.join(root, "on.yaml"), {"Dense.Open": 1})
    r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + os.path.join(root, "seq"), "--streams=2", "--batched=1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "Dense.Open" in r.stderr and "--batched=1" in r.stderr
