"""The stream batcher's dispatch core (ssvio_amd/host/batch_dispatch.{hpp,cpp}) on the CPU: tests/host/test_dispatch_units.cpp drives it
with fake request kinds and threads whose order is determined, and compares the log of dispatches exactly -- what is served first, who
is waited for, the 2 ms rule of the backend slots, error isolation, the slot rule.  The program links the core alone (no libssx.so),
once plain and once under ThreadSanitizer.  A mistake in this protocol is a hang: every run has a time limit.

The ThreadSanitizer build uses the clang++ that hipcc drives, not g++: the keyframe dispatcher's timed wait (condition_variable::wait_for
on the steady clock) is pthread_cond_clockwait, which the runtime of g++ 11 does not intercept -- it then believes the dispatcher never
let go of its mutex and reports "double lock of a mutex" for correct code."""
import os
import subprocess

import pytest

import host_util

ROOT = host_util.ROOT


def _clangxx():
    from ssvio_amd import build as b
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(b.hipcc())))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("the clang++ of the ROCm installation was not found beside hipcc")


def _binary(kind=None):
    from ssvio_amd import build as b
    out = os.path.join(host_util.OUT, kind or "")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_dispatch_units")
    srcs = [os.path.join(ROOT, "tests", "host", "test_dispatch_units.cpp"), os.path.join(b.HOST, "batch_dispatch.cpp")]
    deps = srcs + [os.path.join(b.HOST, "batch_dispatch.hpp")]
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(d) for d in deps):
        return exe
    cxx, flags = {None: ("g++", ["-O2"]), "tsan": (_clangxx(), ["-O1", "-g", "-fsanitize=thread"])}[kind]
    subprocess.check_call([cxx, "-std=c++17", "-Wall", *flags, *srcs, "-lpthread", "-o", exe])
    return exe


@pytest.mark.parametrize("kind", [None, "tsan"])
def test_dispatch_units(kind):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([_binary(kind)], capture_output=True, text=True, timeout=20, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.splitlines()[-1] == "dispatch units: ok"
    assert "ThreadSanitizer" not in r.stderr
