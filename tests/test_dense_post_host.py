"""CPU: the host path of Dense.Speckle.Size / Dense.Speckle.Range / Dense.Cloud.OnDevice on a Compute that records what it is asked
(tests/host/test_dense_post_units.cpp): with the keys there is ONE Compute::DenseKeyframe call per keyframe, with the settings' post, the
depth bar as ssx_dense_min_disp16(fx * baseline, Dense.Cloud.Max.Depth) and want_map following the sink; the keyframe keeps exactly the
samples handed back; a Compute without CanDensePost is refused with the key's name; with the keys absent DenseKeyframe is never called."""
import os
import subprocess

import numpy as np
import pytest

import host_util as hu
from tools import dense_model as dm
from tools import dense_post_model as pm

ROWS, COLS = 64, 96
BASE = {"Backend.Open": 0, "Camera1.cx": 48.0, "Camera1.cy": 32.0, "Camera2.cx": 48.0, "Camera2.cy": 32.0, "Dense.Open": 1, "Dense.Disparities": 64,
        "Dense.Paths": 4, "Dense.Cloud.Stride": 3, "Dense.Cloud.Max.Depth": 25.5}
CONFIGS = {
    "both": {"Dense.Speckle.Size": 120, "Dense.Speckle.Range": 24, "Dense.Cloud.OnDevice": 1},
    "speckle": {"Dense.Speckle.Size": 100},
    "on_device": {"Dense.Cloud.OnDevice": 1},
    "classic": {"Dense.Speckle.Range": 8, "Dense.Speckle.Size": 0, "Dense.Cloud.OnDevice": 0},
}


def stub_disparity(call):
    v, u = np.mgrid[0:ROWS, 0:COLS]
    return np.where((u * 7 + v * 13 + call) % 11 == 0, -16, 16 + (u * 5 + v * 3 + 40 * call) % 900).astype(np.int16)


def stub_image(salt):
    i = np.arange(ROWS * COLS, dtype=np.int64)
    return ((i * 31 + salt * 17) % 251).astype(np.uint8).reshape(ROWS, COLS)


def stub_samples(call):
    return [v for i in range(5 + call) for v in (3 * i, call, 100 + i, 7 * i + call)]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    from ssvio_amd import build as b
    host_lib, _ = b.build_host()
    root = str(tmp_path_factory.mktemp("dense_post_host"))
    exe = os.path.join(root, "test_dense_post_units")
    src = os.path.join(hu.ROOT, "tests", "host", "test_dense_post_units.cpp")
    rpath = ["-Wl,-rpath," + os.path.dirname(host_lib), "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(["g++", *b.HOST_FLAGS, "-I", hu.ROOT, src, host_lib, b.LIB, "-lpthread", *rpath, "-o", exe])
    cfgs = [hu.write_config(os.path.join(root, name + ".yaml"), dict(BASE, **keys)) for name, keys in CONFIGS.items()]
    r = subprocess.run([exe, *cfgs], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return {w[0]: [int(v) if v.lstrip("-").isdigit() else float(v) for v in w[1:]] for w in (l.split() for l in r.stdout.splitlines()) if w}


def _bar(report):
    fx, baseline = report["camera"]
    return pm.min_disp16(fx * baseline, 25.5)


def test_a_compute_without_the_stage_is_refused_with_the_keys_name(report):
    assert report["refused_both"] == [1, 0] and report["refused_speckle"] == [1, 0] and report["refused_on_device"] == [0, 1]
    assert report["default_throws"] == [1]


def test_the_sample_record_is_the_keyframes(report):
    assert report["layout"] == [8, 8, 0, 2, 4, 6]


def test_one_call_per_keyframe_with_the_settings_post_and_the_derived_bar(report):
    bar = _bar(report)
    assert 1 < bar < 32768
    assert report["both_keyframes"] == [4] and report["both_plain_calls"] == [0] and report["both_post_calls"] == [4] and report["both_stopwatch"] == [4]
    for c in range(4):
        # the frame's own pair, the matcher's parameters, the settings' post, reserved zero, and no map: no sink is attached
        assert report[f"both_call{c}"] == [1001 + 2 * c, 1002 + 2 * c, 64, 4, 120, 24, 3, bar, 0, 0, 0, 0, 0], c
        assert report[f"both_samples{c}"] == stub_samples(c), c                 # exactly what was handed back
    assert report["both_warmup"] == [1, 0, 0, 4]                                # warmed as it will be called, outside the phase's clock


def test_want_map_follows_the_sink(report):
    bar = _bar(report)
    assert report["sink"] == [4, 1, 0]
    for c in range(4):
        assert report[f"sink_call{c}"] == [1001 + 2 * c, 1002 + 2 * c, 64, 4, 120, 24, 3, bar, 0, 0, 0, 0, 1], c
        assert report[f"sink_samples{c}"] == stub_samples(c), c


def test_the_filter_alone_keeps_the_hosts_sampling(report):
    bar = _bar(report)
    fx, baseline = report["camera"]
    assert report["speckle_plain_calls"] == [0]
    for c in range(4):
        assert report[f"speckle_call{c}"] == [1001 + 2 * c, 1002 + 2 * c, 64, 4, 100, 16, 0, bar, 0, 0, 0, 0, 1], c
        want = dm.cloud_samples(stub_disparity(c), stub_image(c), 3, fx * baseline, 25.5)
        assert report[f"speckle_samples{c}"] == want.ravel().tolist() and len(want) > 50, c
    assert report["speckle_warmup"] == [1, 1, 0]
    assert report["on_device_plain_calls"] == [0]
    for c in range(2):
        assert report[f"on_device_call{c}"] == [1001 + 2 * c, 1002 + 2 * c, 64, 4, 0, 16, 3, bar, 0, 0, 0, 0, 0], c


def test_with_the_keys_absent_or_off_the_call_is_never_made(report):
    fx, baseline = report["camera"]
    for can in (0, 1):
        assert report[f"classic{can}"] == [5, 0, 0], can                        # 4 keyframes + the warm-up on the old call, none on the new
        for c in range(4):
            want = dm.cloud_samples(stub_disparity(c), stub_image(c), 3, fx * baseline, 25.5)
            assert report[f"classic{can}_samples{c}"] == want.ravel().tolist(), (can, c)
