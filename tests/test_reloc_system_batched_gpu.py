"""Relocalisation under the batched many-streams mode, end to end on the GPU through ssx_run_kitti --streams=3 --batched=C --loop_batched=1:
the candidate queries of the streams that lost tracking go to the GPU as ssx_kfdb_relocalize_query_batch calls on the cohort's loop context
(a stream's pending keyframe is committed inside the call: it is the keyframe the recovery lands on) and the poses of their candidates as
packed ssx_pnp_pose_batch calls (ssvio_amd/host/stream_batcher.cpp), and every stream still writes, byte for byte, the trajectory and the
loop log of the single-stream unbatched run of its drive, reloc_frame lines included.

Drive A is reloc_drive.TEST_DRIVE (lost at frame 8, three grey frames).  Drive B has the same camera and image size, another scene
(seed 1) and is lost at frame 6 for two frames: its streams are lost and recover at other frames than A's."""
import os
import re

import pytest

from test_reloc_system_gpu import _bytes, _reloc_lines, built  # noqa: F401 (built: fixture)
from tools import reloc_drive, synth

pytestmark = pytest.mark.gpu

ON = {"Relocalization.Open": 1}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("reloc_batched"))
    voc = os.path.join(root, "voc.txt")
    synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
    a = reloc_drive.make_reloc_drive(root, **reloc_drive.TEST_DRIVE)
    b = reloc_drive.make_reloc_drive(root, **dict(reloc_drive.TEST_DRIVE, seed=1, b=6, n_blank=2, tag="seq_b"))
    return dict(root=root, voc=voc, drives=[a, b])


@pytest.fixture(scope="module")
def singles(built, world):
    """the single-stream unbatched run of either drive with relocalisation on; both lose tracking and recover"""
    out = []
    for k, drive in enumerate(world["drives"]):
        r = reloc_drive.run_drive(built["run_kitti"], world["root"], drive, world["voc"], "single_%d" % k, ON)
        assert r["r"].returncode == 0, (r["r"].stdout[-1500:], r["r"].stderr[-1500:])
        rel = _reloc_lines(r["log"])
        assert "frame %d: tracking lost" % drive["b"] in r["r"].stderr and "final status LOST" not in r["r"].stdout, k
        assert sum(l["accepted"] >= 0 for l in rel) == 1 and rel[-1]["accepted"] >= 0, (k, rel)
        out.append(r)
    lost = [[l["reloc_frame"] for l in _reloc_lines(r["log"])] for r in out]
    assert lost[0] != lost[1]                                     # the two drives' streams are lost at other frames
    return out


def _streams(built, world, tag, extra):
    a, b = world["drives"]
    both = dict(a, dir=a["dir"] + "," + b["dir"])                # stream k runs drive k mod 2
    return reloc_drive.run_drive(built["run_kitti"], world["root"], both, world["voc"], tag, ON, extra)


@pytest.mark.parametrize("cohorts", [1, 2])
def test_batched_streams_write_the_single_streams_bytes(built, world, singles, cohorts):
    assert world["drives"][0]["K"] == world["drives"][1]["K"]
    b = _streams(built, world, "cohort%d" % cohorts, ("--streams=3", "--batched=%d" % cohorts, "--loop_batched=1"))
    assert b["r"].returncode == 0, (b["r"].stdout[-1500:], b["r"].stderr[-1500:])
    for k in range(3):
        ref = singles[k % 2]
        assert _bytes(b["traj"] + ".%d" % k) == _bytes(ref["traj"]), k
        assert _bytes(b["log"] + ".%d" % k) == _bytes(ref["log"]), k
        assert any(l["accepted"] >= 0 for l in _reloc_lines(b["log"] + ".%d" % k))
    m = re.search(r"reloc_calls (\d+) reloc_jobs (\d+) pose_calls (\d+) pose_jobs (\d+)", b["r"].stdout)
    assert m, b["r"].stdout[-1500:]
    calls, jobs, pose_calls, pose_jobs = map(int, m.groups())
    print("cohorts", cohorts, "reloc_calls", calls, "reloc_jobs", jobs, "pose_calls", pose_calls, "pose_jobs", pose_jobs)
    assert jobs >= calls > 0 and pose_jobs >= pose_calls >= 1
    if cohorts == 1:
        assert jobs > calls > 0                                   # streams 0 and 2 run the same drive and shared calls


def test_relocalisation_is_refused_without_the_batched_loop_step(built, world):
    bad = _streams(built, world, "refused", ("--streams=3", "--batched=1"))
    assert bad["r"].returncode != 0 and "--loop_batched" in bad["r"].stderr and "--batched" in bad["r"].stderr
    assert "Relocalization.Open" in bad["r"].stderr
