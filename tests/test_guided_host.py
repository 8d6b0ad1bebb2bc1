"""CPU: the guided search of relocalisation in the host layer (LoopClosing::Relocalize behind Relocalization.Guided.Open: 1) against a
scripted LoopCompute (tests/host/test_guided_units.cpp): what is gathered and in which order (tools.guided_model.gather_points), which
features are taken, the pose as a matrix, the refinement's pairs, acceptance and fall-back (tools.guided_model.refine_accept), that
nothing new is called with the key absent or 0, and the combinations that are refused."""
import os
import subprocess

import pytest

import host_util
from tools import guided_model as gm
from tools import synth

BASE = {"ORBextractor.nNewFeatures": 100, "ORBextractor.scaleFactor": 1.2, "ORBextractor.nLevels": 8, "ORBextractor.iniThFAST": 20, "ORBextractor.minThFAST": 7,
        "Loop.Threshold.Heigher": 0.5, "Pyramid.Level": 4, "Loop.Closig.Keyframe.Database.Min.Size": 3, "numFeatures.trackingBad": 5, "Relocalization.Open": 1,
        "Relocalization.Guided.Open": 1}
# the map, keyframe by keyframe: one token per feature ("-": no map point, "n!": condemned, "n~": gone from the map).  Keyframe 1 is the
# accepted one; its first 12 features are the first pass's pairs
MAP = [["100", "101", "-", "102"],
       [str(i) for i in range(12)] + ["200", "201!", "202~", "-", "100", "203"],
       ["200", "300", "8", "301"],
       ["400", "0", "401"],
       ["500"]]
ACCEPTED, PAIRS, INLIERS = 1, 12, 8


@pytest.fixture(scope="module")
def built():
    return host_util.build_test_binaries()


@pytest.fixture(scope="module")
def units(built):
    """tests/host/build/test_guided_units, linked like test_reloc_units"""
    from ssvio_amd import build as b
    src = os.path.join(host_util.ROOT, "tests", "host", "test_guided_units.cpp")
    exe = os.path.join(host_util.OUT, "test_guided_units")
    if not (os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(src), os.path.getmtime(built["host_lib"]))):
        rpath = ["-Wl,-rpath," + os.path.dirname(built["host_lib"]), "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib"]
        subprocess.check_call(["g++", *b.HOST_FLAGS, "-I", host_util.ROOT, src, built["host_lib"], b.LIB, "-lpthread", *rpath, "-o", exe])
    return exe


def run(units, tmp_path, settings, runs, kfs=MAP, name="scenario.txt"):
    """runs = [(accepted, pairs, inliers, matched, found, after)] -> per run the dict of its printed lines"""
    lines = ["reset"] + ["setting %s %s" % kv for kv in settings.items()]
    for r in runs:
        lines += ["kf " + " ".join(k) for k in kfs] + ["run %d %d %d %d %d %d" % r]
    path = os.path.join(str(tmp_path), name)
    open(path, "w").write("\n".join(lines) + "\n")
    p = subprocess.run([units, path], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    out = []
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "run":
            out.append({})
        elif w[0] in ("keyframes", "pose", "gather", "error"):
            out[-1][w[0]] = w[1:]
        elif w[0] == "taken":
            out[-1]["taken"] = w[1] if len(w) > 1 else ""
        elif w[0] == "refine":
            out[-1]["refine"] = dict(fx=float(w[2]), tx=float(w[4]), M=int(w[6]), pairs=w[8:])
        elif w[0] == "result":
            at = w.index("list")
            out[-1]["result"] = dict(zip(w[1:at:2], w[2:at:2]), list=w[at + 1:], line=line)
        elif w[0] in ("guided", "record", "calls"):
            out[-1][w[0]] = dict(zip(w[1::2], w[2::2]))
    return out


def model_gather(ids, neighbours, kfs=MAP):
    feats = {}
    for kf_id, toks in zip(ids, kfs):
        feats[kf_id] = [None if t == "-" else (int(t.rstrip("!~")), not t.endswith("~"), t.endswith("!")) for t in toks]
    return gm.gather_points(ids, ids[ACCEPTED], neighbours, feats, first_points=range(INLIERS))


def test_the_gather_the_taken_features_and_the_refinements_pairs(units, tmp_path):
    d = run(units, tmp_path, BASE, [(ACCEPTED, PAIRS, INLIERS, 5, 1, 10)])[0]
    ids = [int(x) for x in d["keyframes"]]
    assert ids == sorted(ids) and len(ids) == 5
    want = model_gather(ids, 2)
    # by hand, as a check on the check: the accepted keyframe, then the one before it, the one after it, and the one two after it
    assert [w[0] for w in want] == [8, 9, 10, 11, 200, 100, 203, 101, 102, 300, 301, 400, 401]
    assert d["gather"] == ["%d:%d:%d" % w for w in want]
    assert d["taken"] == "1" * INLIERS + "0" * (48 - INLIERS)
    # the settings' defaults, the extractor and the levels of the loop step, the camera
    g = d["guided"]
    assert (float(g["radius"]), int(g["max_distance"]), int(g["ratio"]), int(g["levels"]), int(g["nfeatures"]), float(g["fx"]), int(g["features"])) == (10.0, 50, 90, 4, 100, 450.0, 48)
    # the first pass's pose (a quarter turn about z, t = (1, 2, 3)) as 12 doubles, row-major [R|t]
    assert [float(x) for x in d["pose"]] == pytest.approx([0, -1, 0, 1, 1, 0, 0, 2, 0, 0, 1, 3], abs=1e-6)
    # the refinement starts from the first pose, over the first pass's surviving pairs followed by the new ones (point:pixel)
    first = ["%d:%.1f" % (i, i + 0.5) for i in range(INLIERS)]
    new = ["%d:%.1f" % (w[0], INLIERS + k + 0.5) for k, w in enumerate(want[:5])]
    assert d["refine"] == dict(fx=450.0, tx=1.0, M=13, pairs=first + new)
    assert d["calls"] == dict(guided="1", refine="1")
    assert (int(d["record"]["guided_points"]), int(d["record"]["guided_matches"]), int(d["record"]["guided_inliers"])) == (13, 5, 10)


def test_neighbours(units, tmp_path):
    for nb in (0, 1, 3):
        d = run(units, tmp_path, dict(BASE, **{"Relocalization.Guided.Neighbours": nb}), [(ACCEPTED, PAIRS, INLIERS, 0, 1, 8)])[0]
        ids = [int(x) for x in d["keyframes"]]
        assert d["gather"] == ["%d:%d:%d" % w for w in model_gather(ids, nb)], nb
    assert any(w.startswith("500:") for w in d["gather"])                                             # three away: only now
    over = dict(BASE, **{"Relocalization.Guided.Radius": 6.5, "Relocalization.Guided.Max.Distance": 64, "Relocalization.Guided.Ratio": 75})
    g = run(units, tmp_path, over, [(ACCEPTED, PAIRS, INLIERS, 0, 1, 8)])[0]["guided"]
    assert (float(g["radius"]), int(g["max_distance"]), int(g["ratio"])) == (6.5, 64, 75)


FIRST = dict(ok="1", tx="1.0", qz="0.70710678118654757", inliers=str(INLIERS), matches=str(INLIERS))
FIRST_LIST = ["%d:%d" % (i, i) for i in range(INLIERS)]


@pytest.mark.parametrize("found,after", [(1, 10), (1, 8), (1, 13), (1, 7), (1, 0), (0, 13), (0, 0)])
def test_acceptance_follows_refine_accept(units, tmp_path, found, after):
    d = run(units, tmp_path, BASE, [(ACCEPTED, PAIRS, INLIERS, 5, found, after)])[0]
    res = d["result"]
    assert d["calls"] == dict(guided="1", refine="1")
    assert int(d["record"]["guided_inliers"]) == (after if found else -1) and int(d["record"]["inliers"]) == INLIERS
    if gm.refine_accept(INLIERS, after, found=bool(found)):
        # the refinement's pose and inliers; the surviving pairs of both groups (the script keeps the LAST `after` of the 13)
        pairs = FIRST_LIST + ["%d:%d" % (INLIERS + k, p) for k, p in enumerate((8, 9, 10, 11, 200))]
        assert (res["ok"], res["tx"], res["inliers"], res["matches"]) == ("1", "77.0", str(after), str(after)) and res["list"] == pairs[13 - after:]
    else:
        # the first result, bit for bit
        assert {k: res[k] for k in FIRST} == FIRST and res["list"] == FIRST_LIST
    assert (res["tx"] == "77.0") == (found == 1 and after >= INLIERS)                                  # by hand: the bar is inclusive


def test_the_key_absent_or_zero_calls_nothing_new(units, tmp_path):
    absent = {k: v for k, v in BASE.items() if k != "Relocalization.Guided.Open"}
    a = run(units, tmp_path, absent, [(ACCEPTED, PAIRS, INLIERS, 5, 1, 13)])[0]
    z = run(units, tmp_path, dict(BASE, **{"Relocalization.Guided.Open": 0}), [(ACCEPTED, PAIRS, INLIERS, 5, 1, 13)])[0]
    # (out-of-range values of the other keys are not looked at while the key is off)
    o = run(units, tmp_path, dict(absent, **{"Relocalization.Guided.Ratio": 101, "Relocalization.Guided.Radius": -1}), [(ACCEPTED, PAIRS, INLIERS, 5, 1, 13)])[0]
    for d in (a, z, o):
        assert d["calls"] == dict(guided="0", refine="0") and "guided" not in d and "refine" not in d
        assert {k: d["result"][k] for k in FIRST} == FIRST and d["result"]["list"] == FIRST_LIST and d["result"]["guided"] == "0"
        assert (d["record"]["guided_points"], d["record"]["guided_matches"], d["record"]["guided_inliers"]) == ("0", "0", "0")
    assert a["result"]["line"] == z["result"]["line"] == o["result"]["line"]


def test_settings_out_of_range_are_refused(units, tmp_path):
    for kv in ({"Relocalization.Guided.Neighbours": -1}, {"Relocalization.Guided.Radius": -0.5}, {"Relocalization.Guided.Max.Distance": 257},
               {"Relocalization.Guided.Max.Distance": -1}, {"Relocalization.Guided.Ratio": 101}, {"Relocalization.Guided.Ratio": -1}):
        d = run(units, tmp_path, dict(BASE, **kv), [(ACCEPTED, PAIRS, INLIERS, 5, 1, 13)])[0]
        assert "Relocalization.Guided.Max.Distance" in " ".join(d["error"]) and "result" not in d, kv
    for kv in ({"Relocalization.Guided.Neighbours": 0}, {"Relocalization.Guided.Radius": 0}, {"Relocalization.Guided.Max.Distance": 256},
               {"Relocalization.Guided.Max.Distance": 0}, {"Relocalization.Guided.Ratio": 100}, {"Relocalization.Guided.Ratio": 0}):
        assert "error" not in run(units, tmp_path, dict(BASE, **kv), [(ACCEPTED, PAIRS, INLIERS, 5, 1, 13)])[0], kv


def test_batched_streams_with_the_guided_search_are_refused(built, tmp_path):
    """before anything touches a device: the runner reads the settings and names the key"""
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "seq", "image_0")); os.makedirs(os.path.join(root, "seq", "image_1"))
    open(os.path.join(root, "seq", "times.txt"), "w").write("")
    for flags in (("--streams=2", "--batched=1"), ("--streams=2", "--batched=1", "--loop_batched=1")):
        cfg = synth.write_settings(os.path.join(root, "cfg.yaml"), {"Relocalization.Open": 1, "Loop.Closing.Open": 1, "Relocalization.Guided.Open": 1})
        r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + os.path.join(root, "seq"), *flags], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and "--batched" in r.stderr and "Relocalization.Guided.Open" in r.stderr and "not supported" in r.stderr, (r.returncode, r.stderr)
