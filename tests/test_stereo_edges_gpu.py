"""GPU: ssx_stereo_match, ssx_bf_match, ssx_triangulate and ssx_triangulate_batch at their edges.

The matchers run the constructed cases of tests/stereo_cases.py (ties, distances / disparities / rows exactly on their limits, the
top rows, 65 535 candidates in three row buckets; tests/test_stereo_cases.py checks on the CPU that each case contains what it
claims) and must return the arrays of the oracle AND of the plain numpy restatement, bit for bit.  The triangulation is held to the
60-digit fixture tests/golden/tri_hp.npz: every decision, and every point within its disparity decade's bar -- the project's 1e-9
where the CPU oracle itself meets it against the 60-digit values, 4 x the oracle's own worst error below (make_tri_hp.py).

Measured on MI355X (test_triangulate_against_60_digits prints the table of the run at hand), disparity decade: kernel's worst
error | bar | oracle's worst error --
  1e-6 px 5.4e-8 | 5.7e-7 | 1.4e-7     1e-5 px 1.8e-8 | 4.7e-8 | 1.2e-8     1e-4 px 6.8e-10 | 3.9e-9 | 9.7e-10
  1e-3 px 1.8e-10 | 1e-9 | 1.3e-10     1e-2 px 8.7e-12 | 1e-9 | 5.2e-12     1e-1 px 1.4e-12 | 1e-9 | 1.4e-12
  1e+0 px 1.2e-13 | 1e-9 | 1.1e-13     1e+1 px 1.4e-14 | 1e-9 | 1.0e-14     1e+2 px 1.5e-15 | 1e-9 | 2.1e-15

With k_match's window as it was before the one-row margin (floorf(a.y - band) .. floorf(a.y + band)) the cases band-2.0, band-0.5
and band-3.3 fail with 32, 2 and 48 left keypoints unmatched -- the counts tests/test_stereo_cases.py derives from the window model.
"""
import importlib.util
import os

import numpy as np
import pytest

import ssvio_amd
import stereo_cases as sc
from ssvio_amd import _lib
from ssvio_amd import orb as sorb
from ssvio_amd._lib import SsxError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gpu_match(ctx, c):
    return sorb.stereo_match(ctx, c["kL"], c["dL"], c["kR"], c["dR"], sorb.match_params(**c["prm"]))


def _mismatches(c, got, want):
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]))[0]
    lines = [f"{len(bad)} of {len(want[0])} left keypoints differ"]
    for i in bad[:12]:
        lines.append(f"  left {i}: y {c['kL']['y'][i]!r} octave {c['kL']['octave'][i]}  got ({got[0][i]}, {got[1][i]})  want ({want[0][i]}, {want[1][i]})"
                     + (f"  right y {c['kR']['y'][want[0][i]]!r}" if want[0][i] >= 0 else ""))
    return "\n".join(lines)


@pytest.mark.parametrize("name", list(sc.MATCH_CASES))
def test_stereo_match_cases(ctx, po, name):
    c = sc.match_case(name)
    idx, dist, _ = sc.reference(name)
    oi, od = po.stereo_match(c["kL"], c["dL"], c["kR"], c["dR"], po.match_params(**c["prm"]))
    assert np.array_equal(oi, idx) and np.array_equal(od, dist)
    gi, gd = _gpu_match(ctx, c)
    assert gi.dtype == idx.dtype and gd.dtype == dist.dtype
    assert gi.tobytes() == idx.tobytes() and gd.tobytes() == dist.tobytes(), _mismatches(c, (gi, gd), (idx, dist))
    if name == "ties":          # the order inside a row bucket comes from atomics: the winner must not depend on it
        for _ in range(3):
            ri, rd = _gpu_match(ctx, c)
            assert ri.tobytes() == idx.tobytes() and rd.tobytes() == dist.tobytes()


@pytest.mark.parametrize("name", list(sc.BF_CASES))
def test_bf_match_cases(ctx, po, name):
    c = sc.bf_case(name)
    idx, dist, _ = sc.reference(name)
    oi, od = po.bf_match(c["dq"], c["dt"])
    assert np.array_equal(oi, idx) and np.array_equal(od, dist)
    gi, gd = sorb.bf_match(ctx, c["dq"], c["dt"])
    assert gi.tobytes() == idx.tobytes() and gd.tobytes() == dist.tobytes()


def test_more_than_65535_candidates_are_refused(ctx):
    """the reduction key carries the index in 16 bits: 65 536 right keypoints / train descriptors are refused with a message, and the
    context answers the next call"""
    big = sc.match_case(f"big-{sc.BIG[0]}x{sc.BIG[1]}")
    kR = np.concatenate([big["kR"], big["kR"][:1]]); dR = np.concatenate([big["dR"], big["dR"][:1]])
    assert len(kR) == 65536
    with pytest.raises(SsxError) as e:
        sorb.stereo_match(ctx, big["kL"][:4], big["dL"][:4], kR, dR)
    assert e.value.status == _lib.SSX_ERR_UNSUPPORTED and "65535" in str(e.value)
    with pytest.raises(SsxError) as e:
        sorb.stereo_match(ctx, kR, dR, big["kL"][:4], big["dL"][:4])
    assert e.value.status == _lib.SSX_ERR_UNSUPPORTED and "65535" in str(e.value)
    with pytest.raises(SsxError) as e:
        sorb.bf_match(ctx, big["dL"][:4], dR)
    assert e.value.status == _lib.SSX_ERR_UNSUPPORTED and "65535" in str(e.value)
    small = sc.match_case("size-4x5")
    gi, gd = _gpu_match(ctx, small)
    assert np.array_equal(gi, sc.reference("size-4x5")[0]) and np.array_equal(gd, sc.reference("size-4x5")[1])
    b = sc.bf_case("bf-5x64")
    bi, bd = sorb.bf_match(ctx, b["dq"], b["dt"])
    assert np.array_equal(bi, sc.reference("bf-5x64")[0]) and np.array_equal(bd, sc.reference("bf-5x64")[1])


def test_workspace_reuse_across_entry_points(ctx, po):
    """one context: ssx_stereo_frame on a small pair, then ssx_stereo_match large -> tiny -> large, then ssx_bf_match -- each the result
    of the same call made alone (a context of its own for the frame; the session's for the rest).  Stale row_ptr / sorted / counts of a
    larger call, or of the frame path that shares the buffers, would show in the smaller one after it."""
    from tools.synth import make_stereo_pair
    L, R, _ = make_stereo_pair(seed=7, h=160, w=260, n_blobs=260)
    prm = sorb.OrbParams(300, 1.2, 4, 20, 7)
    with ssvio_amd.Context(0) as alone:
        want_frame = sorb.stereo_frame(alone, L, R, orb=prm)
    large, tiny, other = "size-1025x257", "size-1x3", "band-clamp"
    with ssvio_amd.Context(0) as c:
        got_frame = sorb.stereo_frame(c, L, R, orb=prm)
        seq = [(n, _gpu_match(c, sc.match_case(n))) for n in (large, tiny, other, tiny, large)]
        b = sc.bf_case("bf-3x63")
        bf = sorb.bf_match(c, b["dq"], b["dt"])
        again = sorb.stereo_frame(c, L, R, orb=prm)
    assert want_frame["n_matched"] > 20
    for got in (got_frame, again):
        for k, v in want_frame.items():
            assert np.array_equal(got[k], v), k
    for n, (gi, gd) in seq:
        si, sd = _gpu_match(ctx, sc.match_case(n))
        assert np.array_equal(gi, si) and np.array_equal(gd, sd) and np.array_equal(gi, sc.reference(n)[0]) and np.array_equal(gd, sc.reference(n)[1]), n
    assert np.array_equal(bf[0], sc.reference("bf-3x63")[0]) and np.array_equal(bf[1], sc.reference("bf-3x63")[1])


# ---------------------------------------------------------------- triangulation at 60 digits
def _generator():
    spec = importlib.util.spec_from_file_location("make_tri_hp", os.path.join(GOLDEN, "make_tri_hp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def hp():
    return dict(np.load(os.path.join(GOLDEN, "tri_hp.npz")))


@pytest.fixture(scope="module")
def single_calls(ctx, hp):
    """ssx_triangulate per rig and pose over the fixture -> xyz [P, N, 3], ok [P, N] (shared, read-only)"""
    P, N = len(hp["poses"]), len(hp["uvL"])
    xyz = np.zeros((P, N, 3)); ok = np.zeros((P, N), np.uint8)
    for r, rig in enumerate(hp["rigs"]):
        m = hp["rig_id"] == r
        for k in range(P):
            x, o = sorb.triangulate(ctx, hp["uvL"][m], hp["uvR"][m], rig=sorb.stereo_rig(rig[:4], rig[4]), T_wc=hp["poses"][k] if hp["pose_on"][k] else None)
            xyz[k, m], ok[k, m] = x, o
    xyz.setflags(write=False); ok.setflags(write=False)
    return xyz, ok


def test_triangulate_against_60_digits(hp, single_calls):
    gen = _generator()
    xyz, ok = single_calls
    assert (ok == hp["ok"][None]).all(), np.nonzero(ok != hp["ok"][None])
    none = hp["decade"] == gen.NO_DECADE
    for k, on in enumerate(hp["pose_on"]):          # no positive disparity: zeroed, or exactly the camera centre
        assert (xyz[k, none] == (hp["poses"][k, 4:] if on else 0.0)).all()
    assert np.array_equal(xyz[:, none], hp["xyz"][:, none])
    err = gen.rel_err(xyz, hp["xyz"])
    over = []
    for k, bar, worst in zip(hp["decades"], hp["bar_by_decade"], hp["oracle_worst_by_decade"]):
        e = err[:, hp["decade"] == k].max()
        print(f"disparity 1e{k:+d} px: kernel worst {e:.3e}  bar {bar:.3e}  kernel / bar {e / bar:.3f}  (oracle worst {worst:.3e})")
        if not e <= bar:
            over.append((int(k), float(e), float(bar)))
    assert not over, over


def test_triangulate_batch_with_its_own_rig_and_pose_per_job(ctx, hp, single_calls):
    """the fixture cut into uneven jobs (one of them empty), rig and pose changing from job to job: per job the bytes of the single call"""
    xyz, ok = single_calls
    jobs, where = [], []
    for r, rig in enumerate(hp["rigs"]):
        at = np.nonzero(hp["rig_id"] == r)[0]
        cuts = [0, 1, 1, 34, 35, len(at)]               # 1, 0, 33, 1 and the rest
        for j in range(len(cuts) - 1):
            sel = at[cuts[j]:cuts[j + 1]]
            k = (j + r) % len(hp["poses"])
            jobs.append(dict(uvL=hp["uvL"][sel], uvR=hp["uvR"][sel], rig=sorb.stereo_rig(rig[:4], rig[4]), T_wc=hp["poses"][k] if hp["pose_on"][k] else None))
            where.append((k, sel))
    order = np.random.default_rng(9).permutation(len(jobs))          # rigs interleaved
    got = sorb.triangulate_batch(ctx, [jobs[i] for i in order])
    assert any(len(w[1]) == 0 for w in where) and len({len(w[1]) for w in where}) >= 4
    for i, (gx, go) in zip(order, got):
        k, sel = where[i]
        assert gx.tobytes() == xyz[k, sel].tobytes() and go.tobytes() == ok[k, sel].tobytes(), (i, k)
