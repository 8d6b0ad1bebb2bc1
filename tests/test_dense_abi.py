"""CPU: the ABI of dense stereo -- the symbols are declared and exported, the ctypes mirrors have the header's sizes and offsets, the
version stays, the defaults are the contract's, and the shim compiles and links against the library."""
import ctypes as C
import os
import subprocess
import tempfile

from tools import dense_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_offsets_match_the_header():
    from ssvio_amd import _lib
    names = {"ssx_dense_params": _lib.DenseParamsC, "ssx_dense_job": _lib.DenseJob}
    fields = [(n, f[0]) for n, cls in names.items() for f in cls._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ssx.h"\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
            + "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, f in fields)
            + 'printf("max_jobs %d\\n", SSX_DENSE_MAX_JOBS); printf("cap %llu\\n", (unsigned long long)SSX_DENSE_WORKSPACE_CAP); printf("version %d\\n", SSX_VERSION);'
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
    assert C.sizeof(_lib.DenseParamsC) == 32 and C.sizeof(_lib.DenseJob) == 48
    assert got["max_jobs"] == _lib.SSX_DENSE_MAX_JOBS == 1024 and got["cap"] == _lib.SSX_DENSE_WORKSPACE_CAP
    assert got["version"] == _lib.SSX_VERSION == 120


def test_symbols_are_declared_exported_and_the_version_stays():
    import ssvio_amd
    from ssvio_amd import _lib
    lib = ssvio_amd.load()
    for sym in ("ssx_stereo_dense", "ssx_dense_default_params", "ssx_dense_debug_last_call", "ssx_dense_debug_stages"):
        assert hasattr(lib, sym), sym
    assert lib.ssx_version() == _lib.SSX_VERSION == 120
    header = open(os.path.join(ROOT, "include", "ssx.h")).read()
    hooks = open(os.path.join(ROOT, "include", "ssx_test_hooks.h")).read()
    for sym in ("ssx_stereo_dense(", "ssx_dense_default_params("):
        assert "SSX_API" in header.split(sym)[0].splitlines()[-1], sym
    for sym in ("ssx_dense_debug_last_call(", "ssx_dense_debug_stages("):
        assert sym in hooks and sym not in header, sym          # the taps are test hooks only


def test_default_params_are_the_contracts():
    from ssvio_amd import dense as dn
    p = dn.default_params()                                       # host code: no device
    m = dm.DenseParams()
    assert (p.disparities, p.p1, p.p2, p.uniqueness, p.lr_tolerance, p.paths) == (m.disparities, m.p1, m.p2, m.uniqueness, m.lr_tolerance, m.paths) \
        == (128, 7, 86, 10, 1, 8)
    assert tuple(p.reserved) == (0, 0)
    q = dn.DenseParams()
    assert bytes(q) == bytes(p)
    dn._fns(dn.load()).ssx_dense_default_params(None)             # a null pointer is no fault


def test_shim_dense_disparity_compiles_and_links():
    from ssvio_amd import build
    lib = build.build()
    src = r'''
#include "ssx_shim.hpp"
int main(int argc, char**) {
  ssx_dense_params p;
  ssx_dense_default_params(&p);                                   // host code: runs without a device
  if (!(p.disparities == 128 && p.p1 == 7 && p.p2 == 86 && p.uniqueness == 10 && p.lr_tolerance == 1 && p.paths == 8 && p.reserved[0] == 0 && p.reserved[1] == 0)) return 1;
  if (ssx_stereo_dense(nullptr, 0, nullptr, 40, 48, &p, 0) != SSX_ERR_INVALID_ARG) return 2;
  if (argc > 100) {   // never executed here (no GPU): only has to compile and link
    ssx::Context ctx(0);
    std::vector<uint8_t> a(48 * 64), b(a.size());
    std::vector<int16_t> d(a.size());
    ssx::DenseDisparity(ctx, a.data(), 64, b.data(), 64, d.data(), 64, 48, 64);
    p.disparities = 64;
    ssx::DenseDisparity(ctx, a.data(), 64, b.data(), 64, d.data(), 64, 48, 64, &p, true);
    return d[0];
  }
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp"), lib,
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        assert subprocess.call([exe]) == 0
