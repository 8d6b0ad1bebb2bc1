"""CPU: the keyframe database surface (ssx_kfdb_*, ssvio_amd.loop, ssx::KeyframeDatabase) is built, bound and linkable.
No compute call is made (there is no GPU here and no CPU fallback)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KFDB_SYMBOLS = ("ssx_kfdb_create", "ssx_kfdb_destroy", "ssx_kfdb_size", "ssx_kfdb_add", "ssx_kfdb_detect_loop", "ssx_kfdb_match_features")


def test_loop_module_imports_and_finds_its_symbols():
    from ssvio_amd import build
    build.build()
    import ssvio_amd
    from ssvio_amd import loop
    lib = ssvio_amd.load()
    missing = [s for s in KFDB_SYMBOLS if not hasattr(lib, s)]
    assert not missing, missing
    loop._bind(lib)                                           # the argument types of every call the class makes
    assert all(getattr(lib, s).argtypes for s in KFDB_SYMBOLS)
    for name in ("add", "detect_loop", "match_features", "size", "close"):
        assert callable(getattr(loop.KeyframeDatabase, name))
    hdr = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert all(s + "(" in hdr for s in KFDB_SYMBOLS)


def test_cpp_shim_keyframe_database_compiles_and_links():
    """ssx::KeyframeDatabase of include/ssx_shim.hpp with the reference's method names, against libssx.so with plain g++"""
    from ssvio_amd import build
    lib = build.build()
    src = r'''
#include "ssx_shim.hpp"
int main(int argc, char**) {
  if (argc > 100) {   // never executed here (no GPU): only has to compile and link
    ssx::Context ctx(0);
    ssx::KeyframeDatabase db(ctx);
    ssx::BowVector bow; bow.ids = {1, 5}; bow.values = {0.5, 0.5};
    std::vector<uint8_t> desc(64, 0); std::vector<int32_t> cls = {0, 1};
    db.AddToKeyframeDatabase(0, bow, desc, cls);
    unsigned long loop_id = 0; float score = 0.f;
    if (db.DetectLoop(25, bow, 0.05f, loop_id, &score)) {
      std::set<std::pair<int, int>> valid = db.MatchFeatures(loop_id, desc, cls);
      return valid.size() < 10 ? 2 : 3;
    }
    return db.size();
  }
  return ssx_version() == SSX_VERSION ? 0 : 1;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp"), lib,
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        assert subprocess.call([exe]) == 0
