"""CPU: the ABI of image undistortion -- the ctypes mirrors of its two structs have the header's sizes, the shim's methods compile and
link, and ssx_undistort_default (host code, no device) returns tools/undistort_model.py's default_iR bit for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tools import undistort_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_match_the_header():
    from ssvio_amd import _lib
    names = {"ssx_undistort_params": _lib.UndistortParams, "ssx_undistort_job": _lib.UndistortJob}
    prog = '#include <stdio.h>\n#include "ssx.h"\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert sizes[n] == C.sizeof(cls), (n, sizes[n], C.sizeof(cls))
    assert C.sizeof(_lib.UndistortParams) == 18 * 8


def test_symbols_are_exported_and_the_version_stays():
    import ssvio_amd
    from ssvio_amd import _lib
    lib = ssvio_amd.load()
    for sym in ("ssx_undistort", "ssx_undistort_default", "ssx_undistort_debug_last_call"):
        assert hasattr(lib, sym), sym
    assert lib.ssx_version() == _lib.SSX_VERSION == 120


def test_shim_camera_compiles_and_links():
    from ssvio_amd import build
    lib = build.build()
    src = r'''
#include "ssx_shim.hpp"
int main(int argc, char**) {
  if (argc > 100) {   // never executed here (no GPU): only has to compile and link
    ssx::Context ctx(0);
    ssx::Camera left(ctx, 718.856f, 718.856f, 607.1928f, 185.2157f, -0.2f, 0.05f, 0.001f, -0.001f), right(ctx, 718.856f, 718.856f, 607.1928f, 185.2157f);
    std::vector<uint8_t> a(376 * 1241), b(a.size()), c(a.size()), d(a.size());
    left.UndistortImage(a.data(), 1241, b.data(), 1241, 376, 1241);
    ssx::Camera::UndistortPair(left, a.data(), 1241, b.data(), 1241, right, c.data(), 1241, d.data(), 1241, 376, 1241, false);
    return left.params().iR[8] == 1.0 ? 0 : 3;
  }
  ssx_undistort_params p;
  const double K[4] = {2.0, 4.0, 1.0, 2.0}, dist[5] = {0.1, 0.2, 0.3, 0.4, 0.5};
  ssx_undistort_default(K, dist, &p);       // host code: runs without a device
  return (p.iR[0] == 0.5 && p.iR[2] == -0.5 && p.iR[4] == 0.25 && p.iR[5] == -0.5 && p.iR[8] == 1.0 && p.dist[4] == 0.5 && p.K[3] == 2.0) ? 0 : 1;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp"), lib,
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        assert subprocess.call([exe]) == 0


def test_default_params_are_the_models_bits():
    from ssvio_amd import undistort as ud
    rng = np.random.default_rng(5)
    cases = [(718.856, 718.856, 607.1928, 185.2157), tuple(float(np.float32(v)) for v in (718.856, 718.856, 607.1928, 185.2157)), (40.0, 40.0, 31.5, 23.5),
             (38.0, 41.0, 30.2, 20.7)] + [tuple(rng.uniform(1.0, 2000.0, 4)) for _ in range(50)]
    for K in cases:
        dist = tuple(rng.normal(size=5))
        p = ud.make_params(K, dist)
        assert np.array(p.iR[:], dtype=np.float64).tobytes() == um.default_iR(K).tobytes(), K
        assert tuple(p.K[:]) == tuple(float(v) for v in K) and tuple(p.dist[:]) == dist
    # four coefficients: k3 = 0; a caller's iR replaces the default
    p = ud.make_params((40.0, 40.0, 31.5, 23.5), (0.1, 0.2, 0.3, 0.4), iR=np.arange(9.0))
    assert p.dist[4] == 0.0 and list(p.iR[:]) == list(range(9))
