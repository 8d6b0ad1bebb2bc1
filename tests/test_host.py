"""The host layer of SURVEY.md §8-F N4 (ssvio_amd/host: settings, KITTI listing, grey-PNG reader, map bookkeeping,
front-end / backend state machines, TUM writer) WITHOUT a GPU: C++ unit checks, and the whole state machine run on the
CPU oracle over a synthetic KITTI-layout sequence written to disk.  tests/test_host_gpu.py runs the same sequence
through libssx.so and compares trajectories."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import host_util as hu


@pytest.fixture(scope="module")
def built():
    return hu.build_test_binaries()


def _chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def _png(w, h, depth, ctype, rows_bytes, filters, interlace=0):
    raw = b"".join(bytes([f]) + r for f, r in zip(filters, rows_bytes))
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) +
            _chunk(b"IDAT", zlib.compress(raw)[:40]) + _chunk(b"IDAT", zlib.compress(raw)[40:]) + _chunk(b"IEND", b""))


def _filtered(rows, bpp, ft):
    """apply PNG filter type ft to every scanline (so the reader has to undo it)"""
    out, prev = [], bytes(len(rows[0]))
    for r in rows:
        f = bytearray(len(r))
        for i in range(len(r)):
            a = r[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 0: pred = 0
            elif ft == 1: pred = a
            elif ft == 2: pred = b
            elif ft == 3: pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            f[i] = (r[i] - pred) & 255
        out.append(bytes(f)); prev = r
    return out


def test_png_reader_survives_malformed_files(built, tmp_path):
    """300 structurally valid-looking PNG files (correct signature and CRCs, so the reader gets past the chunk layer)
    with random headers, filter bytes, truncated / oversized / garbage pixel streams: every file is either decoded to
    the right size or refused with a message -- the process never crashes; well-formed ones match PIL"""
    rng = np.random.default_rng(7)
    from PIL import Image
    files, expect = [], {}
    for i in range(300):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        depth = int(rng.choice([8, 16, 1, 2, 4, 3])); ctype = int(rng.choice([0, 4, 2, 3, 6, 1])); interlace = int(rng.random() < 0.1)
        if rng.random() < 0.35: depth, ctype, interlace = 8, 0, 0                      # a good share of plain grey files
        bpp = max(1, depth // 8) * {0: 1, 4: 2, 2: 3, 3: 1, 6: 4}.get(ctype, 1)
        rows = [bytes(rng.integers(0, 256, w * bpp, dtype=np.uint8)) for _ in range(h)]
        filters = rng.integers(0, 5 if rng.random() < 0.8 else 8, h).tolist()
        raw = b"".join(bytes([f]) + r for f, r in zip(filters, rows))
        mode = 0 if rng.random() < 0.4 else int(rng.integers(1, 6))
        if mode == 1: raw = raw[:int(rng.integers(0, len(raw)))]                       # too few pixels
        if mode == 2: raw = raw + bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))   # too many
        z = zlib.compress(raw)
        if mode == 3: z = z[:int(rng.integers(0, len(z)))]                             # truncated deflate stream
        if mode == 4: z = bytes(rng.integers(0, 256, len(z), dtype=np.uint8))          # garbage instead of deflate
        chunks = [_chunk(b"IHDR", struct.pack(">IIBBBBB", w if mode != 5 else 0, h, depth, ctype, 0, 0, interlace))]
        if rng.random() < 0.3: chunks.append(_chunk(b"tEXt", b"Comment\0fuzz"))
        cut = int(rng.integers(0, len(z) + 1))
        chunks += [_chunk(b"IDAT", z[:cut]), _chunk(b"IDAT", z[cut:])]
        if rng.random() < 0.9: chunks.append(_chunk(b"IEND", b""))
        path = os.path.join(str(tmp_path), f"f{i:04d}.png")
        open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + b"".join(chunks))
        files.append(path)
        if mode == 0 and interlace == 0 and depth == 8 and ctype == 0 and max(filters) <= 4:
            expect[path] = np.asarray(Image.open(path))                               # PIL agrees it is well-formed
    r = subprocess.run([built["units"], "--decode", *files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(files)
    n_ok = 0
    for path, line in zip(files, lines):
        w_ = line.split()
        assert w_[0] == path and w_[1] in ("ok", "error"), line
        if path in expect:
            e = expect[path]
            assert w_[1] == "ok" and (int(w_[2]), int(w_[3]), int(w_[4])) == (e.shape[0], e.shape[1], int(e.sum())), line
            n_ok += 1
    assert n_ok >= 5


def test_host_units(built, tmp_path):
    d = str(tmp_path)
    hu.write_config(os.path.join(d, "cfg.yaml"), {"Map.ActiveMap.Size": 3, "Trajectory.Save.Path": '"%s/traj #1.txt"' % d})
    os.makedirs(os.path.join(d, "seq"))
    open(os.path.join(d, "seq", "times.txt"), "w").write("0.000000e+00\n1.037000e-01\n\n2.075000e-01\n")
    png = os.path.join(d, "png"); os.makedirs(png)
    rng = np.random.default_rng(0)
    from PIL import Image
    names = []

    def put(name, img8, data):
        open(os.path.join(png, name + ".png"), "wb").write(data)
        img8.tofile(os.path.join(png, name + ".raw"))
        names.append((name, img8.shape[0], img8.shape[1]))

    smooth = (np.add.outer(np.arange(37), np.arange(53)) * 3 % 256).astype(np.uint8)
    noise = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    for ft in range(5):                                     # every scanline filter, hand-built files with two IDAT chunks
        for nm, img in (("smooth", smooth), ("noise", noise)):
            rows = [bytes(r) for r in img]
            put(f"{nm}_f{ft}", img, _png(53, 37, 8, 0, _filtered(rows, 1, ft), [ft] * 37))
    img16 = rng.integers(0, 65536, (20, 31), dtype=np.uint16)
    rows16 = [r.astype(">u2").tobytes() for r in img16]
    put("grey16_paeth", (img16 >> 8).astype(np.uint8), _png(31, 20, 16, 0, _filtered(rows16, 2, 4), [4] * 20))
    ga = rng.integers(0, 256, (20, 31, 2), dtype=np.uint8)
    put("grey_alpha", ga[:, :, 0].copy(), _png(31, 20, 8, 4, _filtered([r.tobytes() for r in ga], 2, 3), [3] * 20))
    kitti = rng.integers(0, 256, (376, 1241), dtype=np.uint8)                  # a PIL-written file (adaptive filters)
    Image.fromarray(kitti).save(os.path.join(png, "pil.png"), optimize=True)
    kitti.tofile(os.path.join(png, "pil.raw")); names.append(("pil", 376, 1241))
    open(os.path.join(png, "list.txt"), "w").write("".join(f"{n} {r} {c}\n" for n, r, c in names))
    Image.fromarray(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)).save(os.path.join(png, "rgb.png"))
    Image.fromarray(smooth).convert("P").save(os.path.join(png, "palette.png"))
    open(os.path.join(png, "interlaced.png"), "wb").write(_png(53, 37, 8, 0, [bytes(r) for r in smooth], [0] * 37, interlace=1))
    good = _png(53, 37, 8, 0, [bytes(r) for r in smooth], [0] * 37)
    open(os.path.join(png, "truncated.png"), "wb").write(good[:len(good) // 2])
    bad = bytearray(good); bad[60] ^= 0x55
    open(os.path.join(png, "corrupt.png"), "wb").write(bytes(bad))            # CRC mismatch
    r = subprocess.run([built["units"], d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


REF_YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_00.yaml")


def test_reads_the_reference_settings_file(built):
    """the runner takes ssvio's own config/kitti_00.yaml (tests/golden/kitti_00.yaml: an unmodified copy of that settings file):
    every key System / FrontEnd / Map read parses to the value cv::FileStorage would return"""
    want = {"Camera1.fx": 718.856, "Camera1.cy": 185.2157, "Camera2.cx": 607.1928, "Camera.Base.Line": 386.1448,
            "Camera.NeedUndistortion": 0, "Map.ActiveMap.Size": 12, "numFeatures.initGood": 100, "numFeatures.trackingGood": 50,
            "numFeatures.trackingBad": 10, "ORBextractor.nInitFeatures": 300, "ORBextractor.nNewFeatures": 100,
            "ORBextractor.scaleFactor": 1.2, "ORBextractor.nLevels": 8, "ORBextractor.iniThFAST": 20, "ORBextractor.minThFAST": 7,
            "Min.Init.Landmark.Num": 200, "Backend.Open": 1, "Viewer.ViewpointY": 1000}
    r = subprocess.run([built["units"], "--dump-setting", REF_YAML, *want, "Trajectory.Save.Path", "Backend.Jacobian.Numeric"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(line.split("=", 1) for line in r.stdout.splitlines())
    for k, v in want.items():
        text, as_int, as_double, numeric = got[k].split("|")
        assert numeric == "1", k
        assert float(as_double) == pytest.approx(v, abs=0, rel=1e-12), k
        assert int(as_int) == int(round(v)), k
    assert got["Trajectory.Save.Path"].split("|")[0].endswith(".txt") and got["Trajectory.Save.Path"].split("|")[3] == "0"   # a quoted string
    assert got["Backend.Jacobian.Numeric"].split("|")[:2] == ["", "0"]          # our extra key: absent -> 0 (analytic)


def _run(built, tmp_path, overrides, n_frames=12, step=0.6):
    seq = hu.write_sequence(str(tmp_path), n_frames=n_frames, step=step)
    cfg = os.path.join(str(tmp_path), "cfg.yaml")
    traj = os.path.join(str(tmp_path), "traj.txt")
    hu.write_config(cfg, dict(overrides, **{"Trajectory.Save.Path": f'"{traj}"'}))
    r = subprocess.run([built["oracle_runner"], cfg, seq["dir"], traj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    log = hu.parse_runner_log(r.stdout)
    assert len(log) == n_frames
    return seq, log, traj


def test_state_machine_on_the_oracle(built, tmp_path):
    """12 frames of a fast lateral-motion sequence through System::RunStep on the CPU oracle with a keyframe on every
    frame (numFeatures.trackingGood above any feature count => TRACKING_BAD): initialisation, LK tracking, pose-only
    LM, masked detection, stereo LK, triangulation, a sliding window of 3 keyframes with local BA, the TUM file."""
    seq, log, traj = _run(built, tmp_path, {"Map.ActiveMap.Size": 3, "numFeatures.trackingGood": 100000})
    assert log[0]["status"] == 1 and log[0]["keyframes"] == 1 and log[0]["points"] >= 200        # initialised on frame 0
    assert all(f["status"] == 2 for f in log[1:]), "every later frame must be TRACKING_BAD (keyframe), none LOST"
    assert [f["keyframes"] for f in log] == list(range(1, 13))
    assert [f["active_kfs"] for f in log] == [1, 2] + [3] * 10                                    # Map.ActiveMap.Size
    assert log[-1]["active_points"] < log[-1]["points"]                                           # old points left the window
    assert all(b["features"] > a["features"] for a, b in zip(log, log[1:]))                       # ~100 new features per keyframe
    tum = np.loadtxt(traj, ndmin=2)
    assert tum.shape == (12, 8)
    assert np.allclose(tum[:, 0], seq["dt"] * np.arange(12), atol=1e-6)                           # keyframe timestamps, id order
    first = open(traj).readline().split()
    assert len(first) == 8 and all(len(w.split(".")[1]) == 6 for w in first)                      # fixed notation, 6 decimals
    assert np.abs(np.linalg.norm(tum[:, 4:8], axis=1) - 1).max() < 1e-5
    # ground truth: the camera centre moves along +x by step * baseline per frame (the local BA is gauge-free like the
    # reference's, so compare relative to the first keyframe)
    err = np.abs((tum[:, 1:4] - tum[0, 1:4]) - seq["centres"])
    assert err.max() < 0.03, err.max()


def test_tracking_between_keyframes_on_the_oracle(built, tmp_path):
    """the reference's own thresholds (trackingGood 50 / trackingBad 10) with a raised keyframe threshold: frames are
    tracked against the last keyframe until the inlier count falls below it"""
    seq, log, traj = _run(built, tmp_path, {"numFeatures.trackingGood": 280})
    assert log[0]["keyframes"] == 1 and 2 <= log[-1]["keyframes"] <= 4
    kf_frames = [i for i in range(1, 12) if log[i]["keyframes"] > log[i - 1]["keyframes"]]
    assert all(log[i]["status"] == 2 for i in kf_frames) and all(log[i]["status"] == 1 for i in range(1, 12) if i not in kf_frames)
    assert all(log[i]["features"] <= 280 + 101 for i in kf_frames)
    tum = np.loadtxt(traj, ndmin=2)
    frame_of_kf = np.rint(tum[:, 0] / seq["dt"]).astype(int)
    assert list(frame_of_kf) == [0] + kf_frames
    err = np.abs((tum[:, 1:4] - tum[0, 1:4]) - seq["centres"][frame_of_kf])
    assert err.max() < 0.03, err.max()


def test_forward_drive_with_the_reference_thresholds(built, tmp_path):
    """BASELINE configs[0] shape: the rig drives forward 0.8 m per frame through a rendered corridor, settings exactly
    as config/kitti_00.yaml (300 / 100 features, keyframe when <= 50 inliers remain).  Frame-to-frame tracking against
    the initial stereo map stays within 0.5 % of the ground truth; a keyframe is inserted when the features run out."""
    seq = hu.write_corridor_sequence(str(tmp_path), n_frames=22)
    cfg = hu.write_config(os.path.join(str(tmp_path), "cfg.yaml"), {})
    traj = os.path.join(str(tmp_path), "traj.txt")
    r = subprocess.run([built["oracle_runner"], cfg, seq["dir"], traj], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    log = hu.parse_runner_log(r.stdout)
    assert len(log) == 22 and all(f["status"] in (1, 2) for f in log)
    first_new_kf = next(i for i in range(1, 22) if log[i]["keyframes"] > 1)
    assert 10 <= first_new_kf <= 21 and log[first_new_kf]["status"] == 2
    feats = [f["features"] for f in log[:first_new_kf]]
    assert feats[0] >= 290 and all(b <= a for a, b in zip(feats, feats[1:])) and feats[-1] <= 60     # features leave the view
    for i in range(1, first_new_kf):                                             # pose-only tracking against the stereo map
        err = np.abs(np.array(log[i]["centre"]) - seq["centres"][i]).max()
        assert err < 0.005 * seq["centres"][i][2] + 0.01, (i, err)
    assert log[first_new_kf]["features"] > feats[-1] + 50                        # ~100 new features at the keyframe


def test_asynchronous_backend_on_the_oracle(built, tmp_path):
    """Backend.Async: 1 -- the reference's thread layout (keyframe queue + worker, map mutex): results depend on timing,
    so only what must hold is asserted: every keyframe is inserted, nothing is lost, the trajectory stays on the
    ground truth; three runs to shake out ordering problems"""
    for rep in range(3):
        seq, log, traj = _run(built, tmp_path, {"Map.ActiveMap.Size": 3, "numFeatures.trackingGood": 100000, "Backend.Async": 1})
        assert all(f["status"] == 2 for f in log[1:]) and log[0]["status"] == 1
        tum = np.loadtxt(traj, ndmin=2)
        assert tum.shape == (12, 8) and np.allclose(tum[:, 0], seq["dt"] * np.arange(12), atol=1e-6)
        err = np.abs((tum[:, 1:4] - tum[0, 1:4]) - seq["centres"])
        assert err.max() < 0.05, err.max()
        assert np.abs(np.linalg.norm(tum[:, 4:8], axis=1) - 1).max() < 1e-5


def test_runner_reports_bad_input(built, tmp_path):
    cfg = os.path.join(str(tmp_path), "cfg.yaml")
    hu.write_config(cfg, {})
    r = subprocess.run([built["oracle_runner"], cfg, str(tmp_path / "no_such_sequence"), str(tmp_path / "t.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "times.txt" in r.stderr
    seq = hu.write_sequence(str(tmp_path), n_frames=1)
    hu.write_config(cfg, {"Camera.NeedUndistortion": 1})
    r = subprocess.run([built["oracle_runner"], cfg, seq["dir"], str(tmp_path / "t.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "NeedUndistortion" in r.stderr
