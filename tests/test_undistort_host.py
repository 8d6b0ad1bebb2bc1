"""CPU: the host path of Camera.NeedUndistortion on a Compute that records what it is asked (tests/host/test_undistort_units.cpp): System
reads the coefficients as float and widens them, FrontEnd::GrabSteroImage replaces the frame's images before anything looks at them and
gives them fresh ids, System::Warmup makes the call once, a Compute that cannot undistort is refused naming the key, and with the key 0
nothing changes."""
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import undistort_model as um

COEFFS = {"Camera1.k1": -0.2, "Camera1.k2": 0.03, "Camera1.p1": 0.0008, "Camera1.p2": -0.0005,
          "Camera2.k1": -0.18, "Camera2.k2": 0.02, "Camera2.p1": -0.0006, "Camera2.p2": 0.0004}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    from ssvio_amd import build as b
    host_lib, _ = b.build_host()
    root = str(tmp_path_factory.mktemp("undistort_host"))
    exe = os.path.join(root, "test_undistort_units")
    src = os.path.join(hu.ROOT, "tests", "host", "test_undistort_units.cpp")
    rpath = ["-Wl,-rpath," + os.path.dirname(host_lib), "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(["g++", *b.HOST_FLAGS, "-I", hu.ROOT, src, host_lib, b.LIB, "-lpthread", *rpath, "-o", exe])
    on = hu.write_config(os.path.join(root, "on.yaml"), dict({"Camera.NeedUndistortion": 1}, **COEFFS))
    off = hu.write_config(os.path.join(root, "off.yaml"), dict({"Camera.NeedUndistortion": 0}, **COEFFS))
    r = subprocess.run([exe, on, off], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.strip()}


def test_a_compute_that_cannot_undistort_is_refused(report):
    assert report["refused"] == ["1"] and report["default_throws"] == ["1"]


def test_the_frame_is_replaced_before_anything_looks_at_it(report):
    assert report["on_undistort_calls"] == ["1"] and report["on_detect_calls"] == ["1"] and report["on_order_ok"] == ["1"]
    assert report["on_inputs"] == ["1001", "1002"]
    ids = [int(v) for v in report["on_frame_ids"]]
    assert len(set(ids)) == 2 and not set(ids) & {0, 1001, 1002}                    # fresh ids
    assert report["on_frame_bytes"] == ["245", "235"]                               # the Compute's marker: 255 - v
    assert report["on_detect"] == [str(ids[0]), "245"]                              # the detector saw the undistorted left image
    assert report["on_stopwatch"] == ["1"]
    assert report["on_second_frame_calls"] == ["2"]
    ids2 = [int(v) for v in report["on_second_frame_ids"]]
    assert len(set(ids + ids2)) == 4 and not set(ids2) & {0, 1003, 1004}
    assert report["on_warmup_calls"] == ["1"] and report["on_stopwatch_after_warmup"] == ["2"]


def test_the_parameters_are_the_settings_read_as_float(report):
    K = tuple(float(np.float32(hu.DEFAULT_CONFIG["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))
    for cam, key in (("Camera1", "on_left"), ("Camera2", "on_right")):
        got = np.array([float(v) for v in report[key]])
        dist = [float(np.float32(COEFFS[f"{cam}.{n}"])) for n in ("k1", "k2", "p1", "p2")] + [0.0]
        assert got[:4].tolist() == list(K)
        assert got[4:9].tolist() == dist
        assert got[9:].tobytes() == um.default_iR(K).tobytes()


def test_the_key_off_changes_nothing(report):
    for can in "01":
        assert report[f"off{can}_undistort_calls"] == ["0"] and report[f"off{can}_frame_ids"] == ["2001", "2002"] and report[f"off{can}_stopwatch"] == ["0"]
