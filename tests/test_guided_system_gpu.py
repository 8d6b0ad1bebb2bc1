"""The guided search of relocalisation in the headless system, end to end on the GPU, through ssx_run_kitti (loopclosing.cpp:
LoopClosing::GuidedStep), on the drive of tools/reloc_drive.py as tests/test_reloc_system_gpu.py runs it.

With Relocalization.Guided.Open absent or 0 the run writes the bytes of a run that never names the key.  With it on, the first pass still
decides where and against which keyframe the front-end recovers -- by construction: the guided search runs behind an accepted candidate --
and the second step adds matches to map points of the candidate's neighbourhood.  The accuracy bar is the one of
test_reloc_system_gpu.py::test_accuracy_against_the_uninterrupted_drive, with the same margin 2 * z_med / fx derived there.
Measured on the MI355X (profiles/reloc_guided/drive.txt): 349 points gathered, 18 matched, inliers 28 -> 34, matches 20 -> 34; largest centre
error after recovery 0.2516 m with the key on, 0.2163 m with it off, 0.2316 m uninterrupted (the bar: 0.2316 + 0.1349 m)."""
import os

import numpy as np
import pytest

import host_util
from tools import reloc_drive, synth
from tools.reloc_guided_drive import parse_guided, reloc_lines

pytestmark = pytest.mark.gpu

RELOC = {"Relocalization.Open": 1}
GUIDED = {"Relocalization.Open": 1, "Relocalization.Guided.Open": 1}


@pytest.fixture(scope="module")
def built():
    return host_util.build_test_binaries()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("reloc_guided_drive"))
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


@pytest.fixture(scope="module")
def off(built, world):
    """Relocalization.Open: 1 in a run that never names the guided key"""
    return _run(built, world, "off", RELOC)


@pytest.fixture(scope="module")
def on(built, world):
    return _run(built, world, "on", GUIDED)


def test_the_key_absent_or_zero_is_the_run_that_never_names_it(built, world, off):
    zero = _run(built, world, "zero", dict(RELOC, **{"Relocalization.Guided.Open": 0}))
    # (the other keys of the group are not looked at while it is off)
    other = _run(built, world, "other", dict(RELOC, **{"Relocalization.Guided.Open": 0, "Relocalization.Guided.Radius": 3.0, "Relocalization.Guided.Neighbours": 4}))
    for run in (zero, other):
        assert _bytes(run["traj"]) == _bytes(off["traj"]) and _bytes(run["log"]) == _bytes(off["log"])
        assert "guided" not in run["r"].stderr and "guided" not in open(run["log"]).read()
    assert any(l["accepted"] >= 0 for l in reloc_lines(off["log"]))


def test_the_guided_search_adds_matches(world, off, on):
    drive = world["drive"]
    a, b = reloc_lines(off["log"]), reloc_lines(on["log"])
    # the first pass decides where and against which keyframe the front-end recovers: the attempts are the same, field by field
    first = ("reloc_frame", "candidates", "pairs", "poses", "inliers", "accepted")
    assert [[l[k] for k in first] for l in a] == [[l[k] for k in first] for l in b] and all(set(l) == set(first) for l in a)
    ok = [l for l in b if l["accepted"] >= 0]
    assert len(ok) == 1 and all((l["guided_points"], l["guided_matches"], l["guided_inliers"]) == (0, 0, 0) for l in b if l["accepted"] < 0)
    g = parse_guided(on["r"].stderr)
    print(on["r"].stderr)
    assert len(g) == 1 and g[0]["frame"] == ok[0]["reloc_frame"]
    g = g[0]
    assert (g["points"], g["matched"], g["inliers_after"]) == (ok[0]["guided_points"], ok[0]["guided_matches"], ok[0]["guided_inliers"])
    print("guided search: %(points)d points gathered, %(matched)d matched, inliers %(inliers_before)d -> %(inliers_after)d, matches %(matches_before)d -> %(matches_after)d" % g)
    assert g["points"] > 0 and g["matched"] >= 1
    assert g["inliers_before"] == ok[0]["inliers"]
    assert g["matches_after"] >= g["matches_before"]            # (the key off: the first pass's matches, by construction)
    assert g["accepted"] == (g["inliers_after"] >= g["inliers_before"]) and (g["accepted"] or g["matches_after"] == g["matches_before"])
    # keyframes are inserted from the relocalised frame on, as with the key off
    fr_on, fr_off = reloc_drive.centre_errors(on["traj"], drive)[0], reloc_drive.centre_errors(off["traj"], drive)[0]
    assert list(fr_on) == list(fr_off) and "final status LOST" not in on["r"].stdout
    tum = np.loadtxt(on["traj"], ndmin=2)
    assert np.isfinite(tum).all() and np.abs(np.linalg.norm(tum[:, 4:8], axis=1) - 1).max() < 1e-5


def test_accuracy_against_the_uninterrupted_drive(built, world, off, on):
    drive = world["drive"]
    clean = _run(built, world, "clean", {}, drive="clean")
    got = [l for l in reloc_lines(on["log"]) if l["accepted"] >= 0][0]["reloc_frame"]
    e_on, e_clean, margin = reloc_drive.accuracy(on["traj"], clean["traj"], drive, got)
    e_off = reloc_drive.accuracy(off["traj"], clean["traj"], drive, got)[0]
    print("largest centre error after recovery: guided %.4f, key off %.4f, uninterrupted %.4f, margin %.4f" % (e_on, e_off, e_clean, margin))
    assert margin == pytest.approx(2 * drive["z_med"] / 450.0) and 0.1 < margin < 0.2
    assert e_on <= e_clean + margin


def test_window_check_repeat_and_streams(built, world, on):
    """Backend.Window.Check: 1 stays silent with the added matches in the window; two runs and --streams=2 write identical bytes"""
    for tag, over in (("check", {"Backend.Window.Check": 1}), ("again", {})):
        r = _run(built, world, tag, dict(GUIDED, **over))
        assert _bytes(r["traj"]) == _bytes(on["traj"]) and _bytes(r["log"]) == _bytes(on["log"]), tag
    st = _run(built, world, "streams", GUIDED, extra=("--streams=2",))
    for k in (0, 1):
        assert _bytes(st["traj"] + ".%d" % k) == _bytes(on["traj"]) and _bytes(st["log"] + ".%d" % k) == _bytes(on["log"])
