"""CPU: the host path of Camera.Rectify on a Compute that records what it is asked (tests/host/test_rectify_units.cpp): System reads the raw
rig as doubles and calls ssx_stereo_rectify, both Camera objects are the common rectified camera with the right one a baseline to the
left's right, FrontEnd::GrabSteroImage hands the frame's pair to Compute::RectifyPair before anything looks at it -- with exactly the two
lenses ssx_stereo_rectify returns -- System::Warmup makes the call once, a Compute that cannot rectify and the two keys together are
refused naming the keys, and with the key 0 nothing new is called."""
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import rectify_model as rm

K_L, K_R = (360.0, 362.5, 158.25, 101.5), (371.0, 368.0, 163.0, 98.75)
KB_L, RT_R = (-0.02, 0.005, -0.001, 0.0002), (-0.05, 0.01, 0.0008, -0.0005, 0.002)
R21 = rm.rot(*np.deg2rad([1.5, -2.0, 1.0]))
T21 = (-0.11, 0.004, -0.003)


def raw_rig_settings():
    cfg = {"Camera1.Model": "kb4", "Camera2.Model": "radtan", "Camera.Rectified.f": 450.0}
    for cam, K in (("Camera1", K_L), ("Camera2", K_R)):
        cfg.update({f"{cam}.{n}": float(v) for n, v in zip(("fx", "fy", "cx", "cy"), K)})
    cfg.update({f"Camera1.{n}": v for n, v in zip(("k1", "k2", "k3", "k4"), KB_L)})
    cfg.update({f"Camera2.{n}": v for n, v in zip(("k1", "k2", "p1", "p2", "k3"), RT_R)})
    cfg.update({f"Stereo.R21.{i}": float(v) for i, v in enumerate(R21.reshape(9))})
    cfg.update({f"Stereo.t21.{i}": float(v) for i, v in enumerate(T21)})
    return cfg


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    from ssvio_amd import build as b
    host_lib, _ = b.build_host()
    root = str(tmp_path_factory.mktemp("rectify_host"))
    exe = os.path.join(root, "test_rectify_units")
    src = os.path.join(hu.ROOT, "tests", "host", "test_rectify_units.cpp")
    rpath = ["-Wl,-rpath," + os.path.dirname(host_lib), "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(["g++", *b.HOST_FLAGS, "-I", hu.ROOT, src, host_lib, b.LIB, "-lpthread", *rpath, "-o", exe])
    on = hu.write_config(os.path.join(root, "on.yaml"), dict({"Camera.Rectify": 1}, **raw_rig_settings()))
    same_K = {f"Camera2.{n}": float(v) for n, v in zip(("fx", "fy", "cx", "cy"), K_L)}          # (without the key the rig must be a rectified one)
    off = hu.write_config(os.path.join(root, "off.yaml"), dict({"Camera.Rectify": 0}, **dict(raw_rig_settings(), **same_K)))
    both = hu.write_config(os.path.join(root, "both.yaml"), dict({"Camera.Rectify": 1, "Camera.NeedUndistortion": 1}, **raw_rig_settings()))
    r = subprocess.run([exe, on, off, both], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rep = {l.split()[0]: l.split()[1:] for l in r.stdout.splitlines() if l.strip() and not l.startswith("Camera.Rectify:")}
    rep["note"] = [l for l in r.stdout.splitlines() if l.startswith("Camera.Rectify:")]
    return rep


@pytest.fixture(scope="module")
def want():
    """what ssx_stereo_rectify returns for the settings' rig (the library's own call; that it is the model's bits is test_rectify_abi's)"""
    from ssvio_amd import undistort as ud
    return ud.stereo_rectify([ud.make_lens_params(rm.KB4, K_L, KB_L), ud.make_lens_params(rm.RADTAN, K_R, RT_R)], R21, T21, f=450.0)


def test_refusals_name_their_keys(report):
    assert report["refused"] == ["1"] and report["both_refused"] == ["1"] and report["default_throws"] == ["1"]


def test_the_pair_is_rectified_before_anything_looks_at_it(report):
    assert report["on_rectify_calls"] == ["1"] and report["on_undistort_calls"] == ["0"] and report["on_detect_calls"] == ["1"] and report["on_order_ok"] == ["1"]
    assert report["on_inputs"] == ["1001", "1002"]
    ids = [int(v) for v in report["on_frame_ids"]]
    assert len(set(ids)) == 2 and not set(ids) & {0, 1001, 1002}                    # fresh ids
    assert report["on_frame_bytes"] == ["245", "235"]                               # the Compute's marker: 255 - v
    assert report["on_detect"] == [str(ids[0]), "245"]                              # the detector saw the rectified left image
    assert report["on_stopwatch"] == ["1"] and report["on_second_frame_calls"] == ["2"]
    assert report["on_warmup_calls"] == ["1"] and report["on_stopwatch_after_warmup"] == ["2"]


def test_the_lenses_are_exactly_what_ssx_stereo_rectify_returns(report, want):
    for side, key in ((0, "on_left"), (1, "on_right")):
        cam = want.cam[side]
        assert [int(v) for v in report[key][:2]] == [cam.model, 0]
        got = np.array([float(v) for v in report[key][2:]])
        assert got.tobytes() == np.array(list(cam.K) + list(cam.coeffs) + list(cam.iR)).tobytes(), key
    assert np.array([float(v) for v in report["on_R_l"]]).tobytes() == np.array(want.R_l[:]).tobytes()
    # and those are the model's, from the settings as written: every key was read as a double
    m = rm.rectify(dict(cam=[dict(model=rm.KB4, K=K_L, coeffs=KB_L), dict(model=rm.RADTAN, K=K_R, coeffs=RT_R)], R=R21, t=T21, f=450.0))
    assert np.array(want.cam[0].iR[:]).tobytes() == m["iR_l"].tobytes() and np.array(want.cam[1].iR[:]).tobytes() == m["iR_r"].tobytes()


def test_the_cameras_handed_on_are_the_rectified_ones(report, want):
    f, _, cx, cy = want.newK[:]
    left = [float(v) for v in report["on_left_camera"]]
    right = [float(v) for v in report["on_right_camera"]]
    assert left == [f, f, cx, cy, 0.0, 0.0, 0.0, 0.0]
    assert right == [f, f, cx, cy, want.baseline, -want.baseline, 0.0, 0.0]
    assert f == 450.0 and cx == (K_L[2] + K_R[2]) / 2 and abs(want.baseline - np.linalg.norm(T21)) < 1e-15
    assert report["on_rectified"] == ["1"]
    assert len(report["note"]) == 2 and all("Camera.Base.Line is ignored" in l and "R_l = [" in l for l in report["note"])   # once per System that got as far as its rig


def test_the_key_off_calls_nothing_new(report):
    bf, fx = np.float32(hu.DEFAULT_CONFIG["Camera.Base.Line"]), np.float32(K_L[0])
    for can in "01":
        assert report[f"off{can}_calls"] == ["0", "0"] and report[f"off{can}_frame_ids"] == ["2001", "2002"] and report[f"off{can}_rectified"] == ["0"]
        cam = [float(v) for v in report[f"off{can}_right_camera"]]
        assert cam[:4] == [float(np.float32(v)) for v in K_L] and cam[4] == float(bf / fx)     # the settings' camera, read as float, as ever
