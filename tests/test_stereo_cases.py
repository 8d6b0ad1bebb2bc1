"""CPU: the constructed matcher cases of tests/stereo_cases.py and the 60-digit triangulation fixture, before any GPU sees them.

  * the oracle (orc_stereo_match / orc_bf_match) equals the plain numpy restatement on every case, index and distance;
  * every case contains what it claims -- ties, distances and disparities exactly on their limits, rows exactly on the band;
  * the model of k_match's row window visits every pair the predicate accepts, over an adversarial float32 sweep, and the window
    the kernel had before (lower_margin = 0) does not: that is the divergence the margin closes;
  * the oracle's triangulation meets the stored per-decade bars against the 60-digit values and reproduces every decision.
"""
import importlib.util
import os

import numpy as np
import pytest

import stereo_cases as sc
from stereo_cases import F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_tri_hp", os.path.join(GOLDEN, "make_tri_hp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- matcher cases
@pytest.mark.parametrize("name", list(sc.MATCH_CASES))
def test_oracle_equals_numpy_matcher(po, name):
    c = sc.match_case(name)
    idx, dist, _ = sc.reference(name)
    oi, od = po.stereo_match(c["kL"], c["dL"], c["kR"], c["dR"], po.match_params(**c["prm"]))
    assert np.array_equal(oi, idx) and np.array_equal(od, dist)


@pytest.mark.parametrize("name", list(sc.BF_CASES))
def test_oracle_equals_numpy_brute_force(po, name):
    c = sc.bf_case(name)
    idx, dist, _ = sc.reference(name)
    oi, od = po.bf_match(c["dq"], c["dt"])
    assert np.array_equal(oi, idx) and np.array_equal(od, dist)


def test_tie_cases_tie():
    c = sc.match_case("ties")
    idx, dist, ties = sc.reference("ties")
    assert (ties >= 2).sum() >= 100 and (idx >= 0).all()
    assert sorted(set(dist.tolist())) == [0, 5, 9]
    # the winner is the lowest index of its group -- also where that copy lies in the LAST row of the band
    assert (idx % 192 == 5).all()
    low_is_last_row = c["kR"]["y"][idx] > c["kL"]["y"]
    assert low_is_last_row.sum() >= 30
    # copies one lane apart (64) and on neighbouring lanes both occur
    assert {(5, 69, 133), (5, 6, 12)} == {tuple(np.nonzero((c["dR"][g * 192:(g + 1) * 192] == c["dR"][g * 192 + 5]).all(1))[0]) for g in range(40)}
    _, _, t = sc.reference(f"big-{sc.BIG[0]}x{sc.BIG[1]}")
    assert (t >= 2).sum() >= 10


def test_distance_edge_cases_sit_on_the_edges():
    want = [0, 80, 81, 255, 256, 0, 80, 81, 256, 257]
    for name, accepted in (("dist-default", 80), ("dist-256", 256), ("dist-300", 256)):
        idx, dist, ties = sc.reference(name)
        assert dist.tolist() == want
        assert ((idx >= 0) == (dist <= accepted)).all()          # above max_dist: the distance is reported, the index is -1
        assert ties[8] == 2 and ties[9] == 0                      # two complements; no admissible candidate at all


def test_bit_position_cases_cover_every_bit():
    c = sc.match_case("bits")
    idx, dist, ties = sc.reference("bits")
    x = c["dR"][:256] ^ c["dL"][0]
    assert sorted(int(np.nonzero(np.unpackbits(r, bitorder="little"))[0][0]) for r in x) == list(range(256)) and (sc.POP[x].sum(1) == 1).all()
    assert idx[0] == 0 and dist[0] == 1 and ties[0] == 256
    assert (dist[1:261] == 1).all() and dist[261] == 4 and np.array_equal(idx[1:], 256 + np.arange(261))
    b = sc.bf_case("bf-bits")
    bi, bd, bt = sc.reference("bf-bits")
    assert bd[0] == 1 and bi[0] == 0 and bt[0] == 256 and (bd[1:] == 1).all() and (bt[1:] == 2).all() and len(b["dt"]) == 256


@pytest.mark.parametrize("band_px", [2.0, 0.5, 3.3])
def test_band_cases_sit_on_the_band(band_px):
    c = sc.match_case(f"band-{band_px}")
    idx, _, _ = sc.reference(f"band-{band_px}")
    ay, by, band = c["ay"], c["by"], c["band"]
    dv = ay - by
    assert dv.dtype == F
    acc = sc.predicate_rows(ay, band, by)
    assert np.array_equal(idx >= 0, acc) and np.array_equal(idx[acc], c["partner"][acc])
    octave = c["kL"]["octave"]
    up, down = np.nextafter(band, F(np.inf)), np.nextafter(band, F(0))
    for o in range(8):
        m = octave == o
        for v in (dv, -dv):
            assert (m & (v == band)).sum() >= 2 and (m & (v == up)).sum() >= 2 and (m & (v == down)).sum() >= 2, o
        assert (m & (ay - band < 0) & (ay != np.floor(ay))).sum() >= 4
    assert (ay == 0).sum() >= 16 and (by == 0).sum() >= 16 and (ay == F(-0.5)).sum() >= 16 and (by == F(-0.5)).sum() >= 16
    rows = sc.bucket_rows(c["kL"], c["kR"])
    assert sc.window_model(ay, band, by, rows)[acc].all()
    missed = acc & ~sc.window_model(ay, band, by, rows, lower_margin=0)
    print(f"band_px {band_px}: {int(acc.sum())} of {len(acc)} pairs accepted, {int(missed.sum())} of them outside the window without the margin")
    if band_px != 2.0:
        assert missed.sum() >= {0.5: 1, 3.3: 8}[band_px]      # (an integer row k below the band: only k = 1 from octave 4 up at 0.5 px)
        for bp, o, k in sc.WINDOW_EXAMPLES:
            if bp == band_px:
                b = F(bp) * sc.scales(1.2)[o]
                assert (missed & (ay == F(k) + b) & (by == np.nextafter(F(k), F(0))) & (octave == o)).sum() == 1


def test_band_clamp_case_is_above_the_buckets():
    c = sc.match_case("band-clamp")
    idx, _, _ = sc.reference("band-clamp")
    assert sc.bucket_rows(c["kL"], c["kR"]) == sc.BUCKET_ROWS_MAX - 2
    acc = sc.predicate_rows(c["ay"], c["band"], c["by"])
    assert np.array_equal(idx >= 0, acc) and 5 <= acc.sum() <= len(acc) - 5
    assert ((c["ay"] > 4096) & (c["by"] > 4096) & acc).sum() >= 3 and ((c["ay"] > 4096) & (c["by"] > 4096) & ~acc).sum() >= 2
    assert sc.window_model(c["ay"], c["band"], c["by"], sc.BUCKET_ROWS_MAX - 2)[acc].all()


@pytest.mark.parametrize("name", ["disp-default", "disp-derived"])
def test_disparity_cases_sit_on_the_limits(name):
    c = sc.match_case(name)
    idx, _, _ = sc.reference(name)
    mn, mx, d = F(c["prm"]["min_disp"]), F(c["prm"]["max_disp"]), c["disp"]
    assert d.dtype == F
    assert np.array_equal(idx >= 0, (d >= mn) & (d <= mx))
    assert (d == mn).sum() >= 2 and (d == mx).sum() >= 2
    assert ((d < mn) & (d >= np.nextafter(mn, F(-np.inf)))).sum() >= 1 and (d == np.nextafter(mx, F(np.inf))).sum() >= 1


@pytest.mark.parametrize("name,limit", [("octave-1", 1), ("octave-0", 0), ("octave-2", 2)])
def test_octave_cases_sit_on_the_limit(name, limit):
    c = sc.match_case(name)
    idx, _, _ = sc.reference(name)
    n = 7 * 7
    assert np.array_equal(idx[:n] >= 0, c["doct"][:n] <= limit)
    assert (c["doct"][:n] == limit).sum() >= 7 and (c["doct"][:n] == limit + 1).sum() >= 7
    assert set(c["kL"]["octave"][:n].tolist()) == {-1, 0, 3, 7, 31, 32, 40}
    assert (idx[n:] >= 0).tolist() == [True, True, False, False] * 2       # the band of octave 40 is that of 31, of -1 that of 0


def test_size_cases_cover_the_sizes():
    sizes = set()
    for name in sc.MATCH_CASES:
        if name.startswith("size-"):
            c = sc.match_case(name)
            idx, dist, _ = sc.reference(name)
            sizes.add((len(c["kL"]), len(c["kR"])))
            assert len(idx) == len(c["kL"])
    assert sizes == set(sc.SIZES) and {n for s in sizes for n in s} == {1, 3, 4, 5, 63, 64, 65, 255, 257, 1025}
    assert any(a > b for a, b in sizes) and any(a < b for a, b in sizes)
    idx, dist, _ = sc.reference("size-1025x257")
    assert (idx >= 0).sum() > 100 and (idx < 0).sum() > 100 and (dist == 257).sum() > 10
    c = sc.match_case("one-row-65x257")
    assert len(set(c["kR"]["y"].tolist())) == 1 and (sc.reference("one-row-65x257")[0] >= 0).sum() > 10
    c = sc.match_case(f"big-{sc.BIG[0]}x{sc.BIG[1]}")
    idx, dist, _ = sc.reference(f"big-{sc.BIG[0]}x{sc.BIG[1]}")
    assert (len(c["kL"]), len(c["kR"])) == (260, 65535) and set(c["kR"]["y"].tolist()) == {10.0, 11.0, 12.0}
    assert (idx == 65534).sum() >= 8 and (idx >= 0).sum() > 200


def test_brute_force_cases_cover_the_sizes():
    seen = set()
    for name in sc.BF_CASES:
        c = sc.bf_case(name)
        seen.add((len(c["dq"]), len(c["dt"])))
    assert {q for q, _ in seen} >= set(sc.BF_NQ) and {t for _, t in seen} >= set(sc.BF_NT)
    for q in (1, 5, 260):
        idx, dist, ties = sc.reference(f"bf-{q}x65535")
        assert idx[0] == 65534 and dist[0] == 0
    assert (sc.reference("bf-260x65535")[2] >= 3).sum() >= 100 and (sc.reference("bf-260x65535")[0] % 200 == 0).sum() >= 100
    idx, dist, ties = sc.reference("bf-complement")
    assert (dist == 256).all() and (idx == 0).all() and (ties == 65).all()
    idx, dist, _ = sc.reference("bf-5x0")
    assert (idx == -1).all() and (dist == 257).all()


# ---------------------------------------------------------------- the row window
def _sweep():
    """(a.y, band, b.y) float32: five band_px, octaves 0..7, a.y random / integer + fraction / integer x scale / k + band +- few
    ulps, b.y = a.y -+ band moved by -4..+4 ulps and, in a second copy, snapped to the nearest integer"""
    rng = np.random.default_rng(77)
    scale = sc.scales(1.2)
    n = 600
    ays, bands, bys = [], [], []
    for band_px in (0.5, 1.0, 2.0, 3.3, 7.25):
        for o in range(8):
            band = F(band_px) * scale[o]
            kb = np.where(np.arange(n) % 3 > 0, rng.integers(0, 40, n), rng.integers(0, 4090, n)).astype(F) + band
            lo1, hi1 = np.nextafter(kb, F(-np.inf)), np.nextafter(kb, F(np.inf))
            ay = np.concatenate([rng.uniform(0, 500, n).astype(F), rng.uniform(0, 4200, n // 2).astype(F),
                                 rng.integers(0, 500, n).astype(F) + rng.integers(0, 16, n).astype(F) * F(0.0625),
                                 rng.integers(0, 120, n).astype(F) * scale[rng.integers(0, 8, n)],
                                 kb, lo1, hi1, np.nextafter(lo1, F(-np.inf)), np.nextafter(hi1, F(np.inf))])
            for edge in (ay - band, ay + band):
                for u in range(-4, 5):
                    by = edge.copy()
                    for _ in range(abs(u)):
                        by = np.nextafter(by, F(np.inf) if u > 0 else F(-np.inf))
                    for b in (by, np.rint(by)):
                        ays.append(ay); bands.append(np.full(len(ay), band)); bys.append(b)
    return np.concatenate(ays), np.concatenate(bands), np.concatenate(bys)


def test_window_model_visits_what_the_predicate_accepts():
    ay, band, by = _sweep()
    assert ay.dtype == band.dtype == by.dtype == F and len(ay) > 2_000_000
    acc = sc.predicate_rows(ay, band, by)
    for rows in (sc.BUCKET_ROWS_MAX - 2, 300):
        vis = sc.window_model(ay, band, by, rows)
        assert not (acc & ~vis).any(), f"{int((acc & ~vis).sum())} accepted pairs outside the window (rows {rows})"
    old = sc.window_model(ay, band, by, sc.BUCKET_ROWS_MAX - 2, lower_margin=0)
    missed = acc & ~old
    print(f"window sweep: {len(ay)} pairs, {int(acc.sum())} accepted; without the margin {int(missed.sum())} of them are not visited")
    # the window before the fix: misses, all of them at the LOWER edge with b.y just under an integer below the band
    assert missed.sum() > 100
    assert (by[missed] < ay[missed]).all() and (by[missed] < band[missed]).all() and (np.ceil(by[missed]) - by[missed] < 1e-6).all()


# ---------------------------------------------------------------- triangulation at 60 digits
@pytest.fixture(scope="module")
def hp():
    return dict(np.load(os.path.join(GOLDEN, "tri_hp.npz")))


def test_tri_hp_fixture_is_not_marginal(hp):
    gen = _load_generator()
    uvL, uvR, rig_id, decade = gen.inputs()
    assert np.array_equal(uvL, hp["uvL"]) and np.array_equal(uvR, hp["uvR"]) and np.array_equal(rig_id, hp["rig_id"]) and np.array_equal(decade, hp["decade"])
    T, on = gen.poses()
    assert np.array_equal(T, hp["poses"]) and np.array_equal(on, hp["pose_on"]) and np.array_equal(gen.RIGS, hp["rigs"])
    disp = uvL[:, 0] - uvR[:, 0]
    assert ((disp <= 0) | (disp >= 1e-6)).all() and (disp == 0).sum() >= 3 and (disp < 0).sum() >= 3
    assert (np.abs(hp["ratio"] / 1e-2 - 1) > 1e-6).all()
    assert ((hp["ratio"] >= 1e-2) & (disp > 1)).sum() >= 6 and ((hp["ratio"] < 1e-2) & (disp > 1) & (np.abs(uvL[:, 1] - uvR[:, 1]) > 1)).sum() >= 6
    assert np.array_equal(hp["bar_by_decade"], np.maximum(1e-9, 4 * hp["oracle_worst_by_decade"])) and len(hp["xyz"][0]) < 1000


def test_oracle_meets_the_tri_hp_bars(po, hp):
    gen = _load_generator()
    xyz, ok = gen.oracle_xyz(po, hp["uvL"], hp["uvR"], hp["rig_id"], hp["poses"], hp["pose_on"])
    assert (ok == hp["ok"][None]).all()
    err = gen.rel_err(xyz, hp["xyz"])
    none = hp["decade"] == gen.NO_DECADE
    assert (err[:, none] == 0).all()                       # zeroed, or exactly the camera centre
    for k, bar, worst in zip(hp["decades"], hp["bar_by_decade"], hp["oracle_worst_by_decade"]):
        e = err[:, hp["decade"] == k].max()
        print(f"disparity 1e{k:+d} px: oracle {e:.2e} (stored {worst:.2e})  bar {bar:.2e}")
        assert e <= bar
    # the project's own 1e-9 holds for the oracle from 1e-3 px up; below, the bar is the oracle's own error
    assert (hp["bar_by_decade"][hp["decades"] >= -3] == 1e-9).all() and (hp["bar_by_decade"][hp["decades"] < -4] > 1e-9).all()


def test_tri_hp_subset_regenerates(hp):
    pytest.importorskip("mpmath")
    gen = _load_generator()
    pick = [0, 5, 31, 54, 56, 70, 95 + 17, 2 * 95 + 3, 2 * 95 + 60]
    for i in pick:
        xyz, ratio, ok = gen.solve_hp(hp["uvL"][i], hp["uvR"][i], hp["rigs"][hp["rig_id"][i]], hp["poses"], hp["pose_on"])
        assert np.array_equal(xyz, hp["xyz"][:, i]) and ratio == hp["ratio"][i] and ok == hp["ok"][i], i
