"""CPU: how the stream batcher packs the pose jobs of the streams that lost tracking into ssx_pnp_pose_batch calls (PackPoseCalls of
ssvio_amd/host/batch_dispatch.{hpp,cpp}: grouped by the bytes of K4, cut at SSX_PNP_BATCH_MAX jobs per call), and the keyframe dispatcher
serving a relocalisation request that a stream's thread files while it holds its map mutex.  tests/host/test_reloc_dispatch_units.cpp holds
the cases; the program links the dispatch core alone (no libssx.so).  A mistake in the protocol is a hang: the run has a time limit."""
import os
import subprocess

import host_util

ROOT = host_util.ROOT


def _binary():
    from ssvio_amd import build as b
    os.makedirs(host_util.OUT, exist_ok=True)
    exe = os.path.join(host_util.OUT, "test_reloc_dispatch_units")
    srcs = [os.path.join(ROOT, "tests", "host", "test_reloc_dispatch_units.cpp"), os.path.join(b.HOST, "batch_dispatch.cpp")]
    deps = srcs + [os.path.join(b.HOST, "batch_dispatch.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", *srcs, "-lpthread", "-o", exe])
    return exe


def test_pose_packing_and_the_lost_stream_under_its_map_mutex():
    r = subprocess.run([_binary()], capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines()[-1] == "reloc dispatch units: ok"
