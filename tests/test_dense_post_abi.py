"""CPU: the ABI of the speckle filter and the keyframe's samples -- the three structs have the header's sizes and offsets, the symbols
are declared and exported and the hook stays out of ssx.h, the version stays, the defaults are the contract's, ssx_dense_min_disp16 is
the model's min_disp16 (host code: no device), a null context is refused, and the shim's overloads compile and link."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tools import dense_post_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_offsets_match_the_header():
    from ssvio_amd import _lib
    names = {"ssx_dense_post": _lib.DensePostC, "ssx_dense_sample": _lib.DenseSample, "ssx_dense_cloud": _lib.DenseCloud}
    fields = [(n, f[0]) for n, cls in names.items() for f in cls._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ssx.h"\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
            + "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, f in fields)
            + 'printf("params %zu\\n", sizeof(ssx_dense_params)); printf("job %zu\\n", sizeof(ssx_dense_job)); printf("version %d\\n", SSX_VERSION);'
            + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert got[n] == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    for n, f in fields:
        assert got[n + "." + f] == getattr(names[n], f).offset, (n, f)
    assert (got["ssx_dense_post"], got["ssx_dense_sample"], got["ssx_dense_cloud"]) == (32, 8, 16)
    assert got["params"] == 32 and got["job"] == 48 and got["version"] == _lib.SSX_VERSION == 120      # what was there stays


def test_symbols_are_declared_exported_and_the_version_stays():
    import ssvio_amd
    from ssvio_amd import _lib
    lib = ssvio_amd.load()
    for sym in ("ssx_dense_default_post", "ssx_dense_min_disp16", "ssx_dense_postprocess", "ssx_stereo_dense_post", "ssx_dense_debug_components",
                "ssx_dense_debug_last_call", "ssx_stereo_dense", "ssx_dense_default_params"):
        assert hasattr(lib, sym), sym
    assert lib.ssx_version() == _lib.SSX_VERSION == 120
    header = open(os.path.join(ROOT, "include", "ssx.h")).read()
    hooks = open(os.path.join(ROOT, "include", "ssx_test_hooks.h")).read()
    for sym in ("ssx_dense_default_post(", "ssx_dense_min_disp16(", "ssx_dense_postprocess(", "ssx_stereo_dense_post("):
        assert "SSX_API" in header.split(sym)[0].splitlines()[-1], sym
    assert "ssx_dense_debug_components(" in hooks and "ssx_dense_debug_components" not in header          # the tap is a test hook only


def test_default_post_is_everything_off():
    from ssvio_amd import dense as dn
    p = dn.default_post()                                             # host code: no device
    m = pm.DensePost()
    assert (p.speckle_size, p.speckle_range, p.cloud_stride, p.cloud_min_disp16) == (m.speckle_size, m.speckle_range, m.cloud_stride, m.cloud_min_disp16) == (0, 16, 0, 1)
    assert tuple(p.reserved) == (0, 0, 0, 0)
    assert bytes(dn.DensePost()) == bytes(p)
    dn._fns(dn.load()).ssx_dense_default_post(None)                   # a null pointer is no fault


def test_min_disp16_equals_the_model():
    from ssvio_amd import dense as dn
    rng = np.random.default_rng(11)
    sweep = [(25.0, 40.0), (25.0, 39.999), (25.0, 40.001), (386.1448, 40.0), (200.0, 10.0), (200.0, 1e9), (200.0, 1e-3), (60.0, 3.7), (2048.0, 1.0), (2047.9375, 1.0),
             (379.8145, 0.0001), (1.0, 1e9)]
    sweep += [(float(rng.uniform(1, 3000)), float(rng.uniform(0.01, 200))) for _ in range(200)]
    for bf, z in sweep:
        assert dn.min_disp16(bf, z) == pm.min_disp16(bf, z), (bf, z)
    assert dn.min_disp16(25.0, 40.0) == 10 and dn.min_disp16(200.0, 1e9) == 1 and dn.min_disp16(200.0, 1e-3) == 32768


def test_a_null_context_is_refused():
    from ssvio_amd import _lib
    from ssvio_amd import dense as dn
    lib = dn._fns(dn.load())
    prm, post = dn.DenseParams(), dn.DensePost()
    assert lib.ssx_dense_postprocess(None, 0, None, None, 40, 48, C.byref(post), 0) == _lib.SSX_ERR_INVALID_ARG
    assert lib.ssx_stereo_dense_post(None, 0, None, None, 40, 48, C.byref(prm), C.byref(post), 0) == _lib.SSX_ERR_INVALID_ARG


def test_the_shim_and_the_host_record_compile_and_link():
    from ssvio_amd import build
    lib = build.build()
    src = r'''
#include <cstddef>
#include "ssx_shim.hpp"
#include "ssvio_amd/host/map.hpp"
using ssx::host::DenseSample;
static_assert(sizeof(ssx_dense_sample) == sizeof(DenseSample) && sizeof(DenseSample) == 8, "the keyframe's record");
static_assert(offsetof(ssx_dense_sample, u) == offsetof(DenseSample, u) && offsetof(ssx_dense_sample, v) == offsetof(DenseSample, v), "u, v");
static_assert(offsetof(ssx_dense_sample, disp16) == offsetof(DenseSample, disp16) && offsetof(ssx_dense_sample, intensity) == offsetof(DenseSample, intensity), "disp16, intensity");
int main(int argc, char**) {
  ssx_dense_post q;
  ssx_dense_default_post(&q);                                       // host code: runs without a device
  if (!(q.speckle_size == 0 && q.speckle_range == 16 && q.cloud_stride == 0 && q.cloud_min_disp16 == 1 && q.reserved[0] == 0 && q.reserved[3] == 0)) return 1;
  if (ssx_dense_min_disp16(25.0, 40.0) != 10) return 2;
  ssx_dense_params p;
  ssx_dense_default_params(&p);
  if (ssx_stereo_dense_post(nullptr, 0, nullptr, nullptr, 40, 48, &p, &q, 0) != SSX_ERR_INVALID_ARG) return 3;
  if (ssx_dense_postprocess(nullptr, 0, nullptr, nullptr, 40, 48, &q, 0) != SSX_ERR_INVALID_ARG) return 4;
  if (argc > 100) {   // never executed here (no GPU): only has to compile and link
    ssx::Context ctx(0);
    std::vector<uint8_t> a(48 * 64), b(a.size());
    std::vector<int16_t> d(a.size());
    std::vector<ssx_dense_sample> s;
    q.speckle_size = 100; q.cloud_stride = 4;
    ssx::DenseDisparity(ctx, a.data(), 64, b.data(), 64, d.data(), 64, 48, 64, p, q, &s);
    ssx::DenseDisparity(ctx, a.data(), 64, b.data(), 64, nullptr, 0, 48, 64, p, q, &s);
    ssx::DensePostprocess(ctx, d.data(), 64, a.data(), 64, 48, 64, q, &s);
    q.cloud_stride = 0;
    ssx::DensePostprocess(ctx, d.data(), 64, nullptr, 0, 48, 64, q);
    return d[0] + (int)s.size();
  }
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", ROOT, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               os.path.join(d, "t.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        assert subprocess.call([exe]) == 0
