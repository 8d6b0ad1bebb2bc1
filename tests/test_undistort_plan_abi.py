"""CPU: the ABI of the undistortion plan (ssx_undistort_plan_*) -- the ctypes mirror of its job struct has the header's size, the symbols
are exported, the shim's class compiles and links, and the version stays."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_size_and_limits_match_the_header():
    from ssvio_amd import _lib
    prog = ('#include <stdio.h>\n#include "ssx.h"\nint main(){printf("%zu %d %d %d\\n", sizeof(ssx_undistort_plan_job), SSX_UNDISTORT_MAX_JOBS, '
            "SSX_UNDISTORT_PLAN_MAX_MAPS, SSX_VERSION);return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        size, max_jobs, max_maps, version = map(int, subprocess.check_output([os.path.join(d, "t")]).decode().split())
    assert size == C.sizeof(_lib.UndistortPlanJob) == 32
    assert max_jobs == _lib.SSX_UNDISTORT_MAX_JOBS and max_maps == _lib.SSX_UNDISTORT_PLAN_MAX_MAPS
    assert version == 120


def test_symbols_are_exported_and_the_version_stays():
    import ssvio_amd
    from ssvio_amd import _lib
    from ssvio_amd import undistort as ud
    lib = ud._fns(ssvio_amd.load())
    for sym in ("ssx_undistort_plan_create", "ssx_undistort_plan_add", "ssx_undistort_plan_apply", "ssx_undistort_plan_size", "ssx_undistort_plan_destroy",
                "ssx_undistort_plan_debug_map", "ssx_undistort_plan_debug_last_call"):
        assert hasattr(lib, sym), sym
    assert lib.ssx_version() == _lib.SSX_VERSION == 120
    # a null plan is refused by every entry point, and destroying nothing is nothing (host code: no device)
    assert lib.ssx_undistort_plan_apply(None, 0, None, 0) == _lib.SSX_ERR_INVALID_ARG
    assert lib.ssx_undistort_plan_size(None, None, None, None) == _lib.SSX_ERR_INVALID_ARG
    assert lib.ssx_undistort_plan_create(None, 4, 4, C.byref(C.c_void_p())) == _lib.SSX_ERR_INVALID_ARG
    lib.ssx_undistort_plan_destroy(None)
    assert hasattr(ud, "UndistortPlan")


def test_shim_plan_compiles_and_links():
    from ssvio_amd import build
    lib = build.build()
    src = r'''
#include "ssx_shim.hpp"
int main(int argc, char**) {
  if (argc > 100) {   // never executed here (no GPU): only has to compile and link
    ssx::Context ctx(0);
    ssx::Camera left(ctx, 718.856f, 718.856f, 607.1928f, 185.2157f, -0.2f, 0.05f, 0.001f, -0.001f), right(ctx, 718.856f, 718.856f, 607.1928f, 185.2157f);
    ssx::UndistortPlan plan(ctx, 376, 1241);
    const int ml = plan.Add(left), mr = plan.Add(right.params());
    std::vector<uint8_t> a(376 * 1241), b(a.size()), c(a.size()), d(a.size());
    plan.Apply({{a.data(), 1241, b.data(), 1241, ml}, {c.data(), 1241, d.data(), 1241, mr}});
    plan.Apply({}, true);
    return plan.maps() == 2 && plan.get() ? 0 : 3;
  }
  ssx_undistort_plan_job job{};
  return sizeof job == 32 && ssx_undistort_plan_apply(nullptr, 1, &job, 0) == SSX_ERR_INVALID_ARG ? 0 : 1;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp"), lib,
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        assert subprocess.call([exe]) == 0
