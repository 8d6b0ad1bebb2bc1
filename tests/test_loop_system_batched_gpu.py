"""Loop closing under the batched many-streams mode, end to end on the GPU through ssx_run_kitti --streams=3 --batched=C --loop_batched=1:
the streams' inline keyframe steps go to the GPU as ssx_kfdb_process_keyframe_batch calls on one loop context with one vocabulary per
cohort (ssvio_amd/host/stream_batcher.cpp), and every stream still writes, byte for byte, the trajectory and the loop log of the
single-stream unbatched run of its drive.  The drive, the settings and the helpers are those of test_loop_system_gpu.py; a second drive
with the same camera and image size, another scene and a shorter leg (39 frames against 47) puts the streams out of phase and lets one
end early."""
import os
import re
import subprocess

import pytest

from test_loop_system_gpu import DRIVE, LOOP, _lines, _run, built, world  # noqa: F401 (built, world: fixtures)
from tools import loop_drive, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world_b(tmp_path_factory, world):
    root = str(tmp_path_factory.mktemp("loop_drive_b"))
    return dict(root=root, drive=loop_drive.make_loop_drive(root, **dict(DRIVE, n_leg=20, seed=1)), voc=world["voc"])


@pytest.fixture(scope="module")
def singles(built, world, world_b):
    """the single-stream unbatched run of either drive"""
    return [_run(built, world, "single_a", {}), _run(built, world_b, "single_b", {})]


def _streams(built, world, world_b, tag, overrides, extra, check=True):
    root = world["root"]
    over = dict(LOOP, **{"DBOW2.VOC.Path": '"%s"' % world["voc"]})
    over.update(overrides)
    cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), loop_drive.drive_settings(world["drive"], over))
    traj, log = os.path.join(root, tag + ".traj"), os.path.join(root, tag + ".looplog")
    r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + world["drive"]["dir"] + "," + world_b["drive"]["dir"],
                        "--trajectory=" + traj, "--loop_log=" + log, *extra], capture_output=True, text=True, timeout=120)
    if check:
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return dict(r=r, traj=traj, log=log)


@pytest.mark.parametrize("tag,cohorts,overrides", [("cohort1", 1, {}), ("cohort2", 2, {}), ("window0", 1, {"Backend.Window": 0})])
def test_batched_streams_write_the_single_streams_bytes(built, world, world_b, singles, tag, cohorts, overrides):
    """(Backend.Window: 0 is held to the single runs with the resident window: the two write the same bytes, test_loop_system_gpu.py)"""
    assert world["drive"]["n_frames"] == 47 and world_b["drive"]["n_frames"] == 39 and world["drive"]["K"] == world_b["drive"]["K"]
    b = _streams(built, world, world_b, tag, overrides, ("--streams=3", "--batched=%d" % cohorts, "--loop_batched=1"))
    corrected = 0
    for k in range(3):                                            # stream k runs drive k mod 2
        ref = singles[k % 2]
        assert open(b["traj"] + f".{k}", "rb").read() == open(ref["traj"], "rb").read(), k
        assert open(b["log"] + f".{k}", "rb").read() == open(ref["log"], "rb").read(), k
        corrected += sum(l["corrected"] == "1" for l in _lines(b["log"] + f".{k}"))
    assert corrected >= 1
    m = re.search(r"loop_calls (\d+) loop_jobs (\d+)", b["r"].stdout)
    assert m, b["r"].stdout[-1500:]
    print(tag, "loop_calls", m.group(1), "loop_jobs", m.group(2))
    assert int(m.group(2)) > int(m.group(1)) > 0                  # steps of several streams did share calls


def test_the_loop_thread_is_refused(built, world, world_b):
    bad = _streams(built, world, world_b, "async", {"Loop.Closing.Async": 1}, ("--streams=3", "--batched=1", "--loop_batched=1"), check=False)
    assert bad["r"].returncode != 0 and "--loop_batched" in bad["r"].stderr and "Loop.Closing.Async" in bad["r"].stderr
