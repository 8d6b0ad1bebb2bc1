"""LoopClosing of the host layer (ssvio_amd/host/loopclosing.cpp) on the CPU: tests/host/test_loop_units.cpp replays a scenario of
tools/mapmodel.make_window_scenario on a real Map + Backend with a SCRIPTED LoopCompute and a recording BaWindow, runs the loop step
on every keyframe, and prints what happened; this file compares it with tools/mapmodel.ActiveMap -- the reference's bookkeeping
restated in Python (loopclosing.cpp:43-66, 427-453, 495-529, 657-669).

The scenario: 14 keyframes (ids 0 .. 13), a window of 5.
  kf 0-5   nothing found: each is added to the database
  kf 6     a loop with 7 pairs: fewer than 10, ComputePose is skipped, the keyframe is added
  kf 7     a loop to kf 1, confirmed with need_correct = 0: the loop edge is recorded, nothing moves, the keyframe is NOT added
  kf 8-12  dropped by the "> 5 ids after a closure" rule
  kf 13    a loop to kf 5, confirmed with need_correct = 1: the correction.  Its pairs hold fusions, pairs whose loop map point has
           expired (one of them kept by the scripted ComputePose: the null branch of :451), pairs whose current feature has no map
           point, one pair whose two sides name the SAME map point, and one pair that would put a second feature of the keyframe on
           a map point another feature already got."""
import os
import subprocess

import numpy as np
import pytest

import host_util
from tools import mapmodel

ROOT = host_util.ROOT
N_ACTIVE, CUR, LOOP, KEEP = 5, 13, 5, 12
CORRECTED = [0.0, 0.0, 0.0, 1.0, 0.3125, 0.0, -10.5]
RELATIVE = [0.0, 0.0, 0.0, 1.0, 0.0625, 0.0, -6.25]


def _binary(kind=None):
    """the stand-alone program: the three host sources it needs + libssx.so for ssx_ba_default_options (never a GPU call)"""
    from ssvio_amd import build as b
    b.build()
    out = os.path.join(host_util.OUT, kind or "")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_loop_units")
    srcs = [os.path.join(ROOT, "tests", "host", "test_loop_units.cpp")] + [os.path.join(b.HOST, f) for f in ("map.cpp", "backend.cpp", "loopclosing.cpp")]
    deps = srcs + [os.path.join(b.HOST, f) for f in os.listdir(b.HOST) if f.endswith(".hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    san = {None: [], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"], "tsan": ["-fsanitize=thread", "-g"]}[kind]
    flags = [f for f in b.HOST_FLAGS if kind is None or f != "-O2"] + (["-O1"] if kind else []) + san
    subprocess.check_call(["g++", *flags, "-I", ROOT, *srcs, b.LIB, "-lpthread", "-Wl,-rpath," + os.path.dirname(b.LIB), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def _scenario():
    """-> (command lines without setup, expectations)"""
    frames = mapmodel.make_window_scenario(n_kf=14, n_active=N_ACTIVE, new_per_kf=40, track_len=9, seed=3)
    am = mapmodel.ActiveMap(N_ACTIVE)
    lines, exp = [], {}
    for i, fr in enumerate(frames):
        kf = fr["kf_id"] - 100
        if kf == CUR:
            # before the last keyframe: map points the loop keyframe observes die (expired weak_ptr)
            loop_lms = [f.lm for f in am.kfs[LOOP]["feats"] if f.lm in am.mps and not am.mps[f.lm].active_obs]
            for lm in loop_lms[:6]:
                am.condemn(lm)
                lines.append(f"condemn {lm}")
        for lm in fr["condemn"]:
            am.condemn(lm)
            lines.append(f"condemn {lm}")
        if kf == CUR:
            am.apply([], [], [], [], [], [])                                          # they are gone before the keyframe comes
            lines.append("flush")
        for lm, xyz in fr["new_points"].items():
            lines.append(f"point {lm} {float(xyz[0])!r} {float(xyz[1])!r} {float(xyz[2])!r}")
        # (the oldest active keyframe leaves: the drive moves forward, so the real Map's farthest keyframe is the oldest one)
        am.insert_keyframe(kf, fr["pose"], fr["obs"], fr["new_points"], victim=None)
        feats = am.kfs[kf]["feats"]
        if kf == CUR:                                                                 # two features that carry no map point
            feats += [mapmodel._Feature(kf, None, (31.5, 40.25)), mapmodel._Feature(kf, None, (300.0, 90.5))]
        lines.append(f"kf {kf} {kf - 1} " + " ".join(repr(float(v)) for v in fr["pose"]) + f" {len(feats)}")
        lines += [f"{-1 if f.lm is None else f.lm} {float(f.uv[0])!r} {float(f.uv[1])!r}" for f in feats]
        am.apply([], [], [], [], [], [])                                              # the end of an optimisation: condemned points go
        lines.append("flush")
    cur_feats, loop_feats = am.kfs[CUR]["feats"], am.kfs[LOOP]["feats"]
    unlinked = [i for i, f in enumerate(cur_feats) if f.lm is None]
    alive = lambda f: f.lm is not None and f.lm in am.mps
    loop_alive = [j for j, f in enumerate(loop_feats) if alive(f)]
    loop_dead = [j for j, f in enumerate(loop_feats) if f.lm is not None and f.lm not in am.mps]
    cur_lm = {f.lm: i for i, f in enumerate(cur_feats) if alive(f)}
    same = [(cur_lm[loop_feats[j].lm], j) for j in loop_alive if loop_feats[j].lm in cur_lm]
    assert same and len(loop_dead) >= 3 and len(unlinked) == 2, (len(same), len(loop_dead))
    same_pair = same[0]
    free_loop = [j for j in loop_alive if loop_feats[j].lm not in cur_lm]
    fresh_cur = [i for i, f in enumerate(cur_feats) if alive(f) and i != same_pair[0] and f.lm not in {loop_feats[j].lm for j in loop_alive}]
    assert len(free_loop) >= 8 and len(fresh_cur) >= 10
    fusions = list(zip(fresh_cur[:5], free_loop[:5]))                                 # both alive, different map points
    no_cur = list(zip(unlinked, free_loop[5:7]))                                      # the current feature has no map point
    dead = list(zip(fresh_cur[5:8], loop_dead[:3]))                                   # the loop map point has expired
    duplicate = (fresh_cur[8], free_loop[0])                                          # a second feature for the loop map point of fusions[0]
    pairs = sorted(fusions + no_cur + dead + [same_pair, duplicate])
    has = [1 if alive(loop_feats[j]) else 0 for _, j in pairs]
    kept = [1 if (h or (i, j) == dead[0]) else 0 for (i, j), h in zip(pairs, has)]    # ComputePose erases the expired ones -- all but one here
    flat = lambda ps: " ".join(f"{i} {j}" for i, j in ps)
    seven = lambda v: " ".join(repr(x) for x in v)
    ident = "0.0 0.0 0.0 1.0 0.0 0.0 0.0"
    p6 = [(i, i) for i in range(7)]
    p7 = [(i, i) for i in range(12)]
    scripts = [f"script 6 1 2 0.5 {len(p6)} {flat(p6)} 0 0 0.0 {ident} {ident} " + " ".join("1" * len(p6)),
               f"script 7 1 1 0.625 {len(p7)} {flat(p7)} 0 0 0.25 {ident} {seven(RELATIVE)} " + " ".join("1" * len(p7)),
               f"script {CUR} 1 {LOOP} 0.75 {len(pairs)} {flat(pairs)} 0 1 3.5 {seven(CORRECTED)} {seven(RELATIVE)} " + " ".join(str(k) for k in kept)]
    # what the problem must hold, from the model as it stands before the correction
    kf_ids = sorted(am.kfs)
    row = {k: i for i, k in enumerate(kf_ids)}
    lm_ids = sorted(am.mps)
    edges = []
    for k in kf_ids:
        if k - 1 in row:
            edges.append((row[k], row[k - 1]))
        if k == 7:
            edges.append((row[7], row[1]))
        if k == CUR:
            edges.append((row[CUR], row[LOOP]))
    anchors = []
    for l in lm_ids:
        mp = am.mps[l]
        obs = mp.active_obs if l in am.active_mps else mp.obs
        anchors.append(row.get(obs[0].kf, -1) if obs else -1)
    exp.update(kf_ids=kf_ids, lm_ids=lm_ids, kf_active=[1 if k in am.active_kfs else 0 for k in kf_ids], edges=edges, anchors=anchors,
               point_active=[1 if l in am.active_mps else 0 for l in lm_ids], has=has, n_pairs=len(pairs),
               pose_ty={k: float(am.kfs[k]["pose"][5]) for k in kf_ids}, point_y={l: float(am.mps[l].pos[1]) for l in lm_ids})
    # the fusion on the model: the pairs ComputePose kept, without the two the host layer skips on purpose
    model_pairs = [p for p, k in zip(pairs, kept) if k and p != same_pair and p != duplicate]
    out = am.loop_correct(CUR, CORRECTED, model_pairs, LOOP)
    exp.update(fused=out["fused"], feats={k: [(-1 if f.lm is None else f.lm) for f in am.kfs[k]["feats"]] for k in kf_ids},
               obs={l: [(f.kf, am.kfs[f.kf]["feats"].index(f)) for f in mp.obs] for l, mp in am.mps.items()}, active=sorted(am.active_kfs))
    return lines + scripts, exp


@pytest.fixture(scope="module")
def scenario():
    return _scenario()


def _run(exe, tmp_path, scenario, loop_async=0, backend_async=0, env=None):
    path = os.path.join(str(tmp_path), f"scenario_{loop_async}{backend_async}.txt")
    with open(path, "w") as f:
        f.write(f"setup {N_ACTIVE} {loop_async} {backend_async} {KEEP}\n" + "\n".join(scenario[0]) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def sync_run(tmp_path_factory, scenario):
    return _run(_binary(), tmp_path_factory.mktemp("loop_units"), scenario)


def _records(out):
    recs = []
    for l in out:
        w = l.split()
        if w[0] == "record":
            recs.append({k: v for k, v in zip(w[1:29:2], w[2:29:2])} | {"moved": w[30:33]})
    return recs


def test_queue_and_gating(sync_run, scenario):
    """(a) which keyframes reach the loop step, which are added to the database, which calls are made"""
    out, exp = sync_run, scenario[1]
    calls = [l.split() for l in out if l.startswith("call ")]
    processed = [int(c[3]) for c in calls if c[1] == "process"]
    assert processed == [0, 1, 2, 3, 4, 5, 6, 7, 13]                                  # 8 .. 12: fewer than 6 ids after the closure at 7
    assert [int(c[3]) for c in calls if c[1] == "add_pending"] == [0, 1, 2, 3, 4, 5, 6]   # 7 and 13 are confirmed: not added
    assert [int(c[3]) for c in calls if c[1] == "compute_pose"] == [7, 13]            # kf 6 has 7 pairs (< 10): skipped
    p = [l for l in out if l.startswith("call process kf 13 ")][0]
    assert "image 16x8" in p and f"features {len(exp['feats'][13])} first_class 0 nfeatures 100 levels 4 min_db 3 gap 6 thr 0.375" in p
    recs = _records(out)
    assert [int(r["kf"]) for r in recs] == processed
    assert [int(r["db"]) for r in recs] == [0, 1, 2, 3, 4, 5, 6, 7, 7]
    r6, r7, r13 = recs[6], recs[7], recs[8]
    assert (r6["found"], r6["pairs"], r6["pose"], r6["corrected"]) == ("1", "7", "-1", "0")
    assert (r7["found"], r7["loop"], r7["pose"], r7["need_correct"], r7["corrected"], r7["fused"]) == ("1", "1", "0", "0", "0", "0")
    assert (r13["loop"], r13["need_correct"], r13["corrected"], r13["pg_iters"], r13["moved"]) == (str(LOOP), "1", "1", "7", ["11", "13", "17"])
    assert out[-1] == "stats steps 9 corrections 1 dropped 5 paused 0"
    kf = {int(l.split()[1]): l.split() for l in out if l.startswith("keyframe ")}
    assert all(w[5] == "0" for w in kf.values()), "every keyframe's image is released: after its step, or when it is dropped"
    assert kf[7][7] == "1" and float(kf[7][9]) == RELATIVE[4] and kf[13][7] == str(LOOP) and all(kf[k][7] == "-1" for k in kf if k not in (7, 13))
    # need_correct = 0 moved nothing; the one correction moved every keyframe and every map point by the scripted amount, once
    assert all(float(kf[k][11]) == exp["pose_ty"][k] + 0.25 for k in kf)
    mp = {int(l.split()[1]): float(l.split()[5]) for l in out if l.startswith("mappoint ")}
    assert all(mp[l] == exp["point_y"][l] + 0.125 for l in mp)


def test_marshalled_problem(sync_run, scenario):
    """(b) the ssx_loop_correct_problem field by field"""
    out, exp = sync_run, scenario[1]
    prob = {l.split()[1]: l.split()[2:] for l in out if l.startswith("problem ")}
    row = {k: i for i, k in enumerate(exp["kf_ids"])}
    head = dict(zip(prob["n_keyframes"][1::2], prob["n_keyframes"][2::2]))
    assert int(prob["n_keyframes"][0]) == len(exp["kf_ids"]) == 14
    assert (int(head["n_edges"]), int(head["n_points"])) == (len(exp["edges"]), len(exp["lm_ids"]))
    assert (int(head["cur"]), int(head["loop"]), int(head["initial"]), int(head["keep"])) == (row[CUR], row[LOOP], row[0], row[KEEP])
    assert float(head["corrected_tx"]) == CORRECTED[4]
    assert [int(v) for v in prob["kf_active"]] == exp["kf_active"] and sum(exp["kf_active"]) == N_ACTIVE
    assert [float(v) for v in prob["pose_tx"]] == [float(am) for am in [_pose_tx(scenario, k) for k in exp["kf_ids"]]]     # ascending ids
    got_edges = [tuple(int(x) for x in e.split(":")[:2]) for e in prob["edges"]]
    assert got_edges == exp["edges"]                                                   # per keyframe: the last-keyframe edge, then the loop edge
    assert (row[7], row[1]) in got_edges and got_edges[-1] == (row[CUR], row[LOOP])
    loop_meas = [float(e.split(":")[2]) for e in prob["edges"] if tuple(int(x) for x in e.split(":")[:2]) in ((row[7], row[1]), (row[CUR], row[LOOP]))]
    assert loop_meas == [RELATIVE[4], RELATIVE[4]]
    assert [int(v) for v in prob["anchors"]] == exp["anchors"]
    assert [int(v) for v in prob["point_active"]] == exp["point_active"]
    assert -1 not in exp["anchors"] and 0 in exp["point_active"] and 1 in exp["point_active"]
    cp = [l for l in out if l.startswith("call compute_pose kf 13 ")][0].split()
    assert int(cp[5]) == exp["n_pairs"] and [int(v) for v in cp[7:7 + exp["n_pairs"]]] == exp["has"] and 0 in exp["has"]


def _pose_tx(scenario, kf):
    for l in scenario[0]:
        w = l.split()
        if w[0] == "kf" and int(w[1]) == kf:
            return float(w[7])
    raise KeyError(kf)


def _check_fusion(out, exp):
    kf = {int(l.split()[1]): l.split() for l in out if l.startswith("keyframe ")}
    assert sorted(k for k in kf if kf[k][3] == "1") == exp["active"]
    for k, w in kf.items():
        assert [int(v) for v in w[w.index("feats") + 1:]] == exp["feats"][k], f"map points of keyframe {k}'s features"
    mps = {int(l.split()[1]): l for l in out if l.startswith("mappoint ")}
    assert sorted(mps) == sorted(exp["obs"])
    for l, line in mps.items():
        obs = line.split(" obs", 1)[1].split("|")[0].split()
        assert [tuple(int(x) for x in o.split(":")) for o in obs] == exp["obs"][l], f"observations of map point {l}"
    win = [l.split() for l in out if l.startswith("window_loop_correct ")]
    assert len(win) == 1 and int(win[0][2]) == CUR and float(win[0][4]) == CORRECTED[4]
    assert [int(v) for v in win[0][6:]] == exp["fused"] and len(exp["fused"]) == 5
    assert all(l not in mps for l in exp["fused"])


def test_fusion_equals_the_model(sync_run, scenario):
    """(c) every feature's map point, every map point's observation list in order, the removed ids, the ids handed to the window;
    (d) the same-point pair and the pair that would duplicate a map point in the keyframe are skipped and counted"""
    out, exp = sync_run, scenario[1]
    _check_fusion(out, exp)
    r13 = _records(out)[-1]
    assert (r13["fused"], r13["same_point"], r13["duplicate"]) == ("5", "1", "1")


@pytest.mark.parametrize("loop_async,backend_async", [(1, 0), (1, 1), (0, 1)])
def test_threads(tmp_path, scenario, loop_async, backend_async):
    """the loop step on its own thread and / or behind the backend's thread: the correction of the last keyframe sees the same map,
    so the fusion is the same; the backend is running again afterwards"""
    out = _run(_binary(), tmp_path, scenario, loop_async, backend_async)
    _check_fusion(out, scenario[1])
    # (with a thread between them the keyframes 8 .. 12 may reach the queue before the closure at 7 is known: how many are dropped is timing)
    assert " corrections 1 " in out[-1] and out[-1].endswith("paused 0")
