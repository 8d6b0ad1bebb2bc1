"""CPU: the guided search of relocalisation in the C ABI -- include/ssx.h declares both calls and the status enum, the library exports
them, the ctypes signatures of ssvio_amd/loop.py load, and the refusals that need no device are refused.  No compute call is made."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_both_calls_and_the_enum():
    names = ["MATCHED", "BEHIND", "OUTSIDE", "NO_DESCRIPTOR", "NO_FEATURE", "DISTANCE", "RATIO", "CLAIMED"]
    prog = ('#include <stdio.h>\n#include "ssx.h"\nint main(){ssx_status (*a)(ssx_kf_database*, const double*, const double*, int32_t, int32_t, int32_t, const float*, '
            'const uint8_t*, int32_t, const uint8_t*, const int32_t*, int32_t, const int64_t*, const int32_t*, const double*, double, int32_t, int32_t, int32_t*, '
            'int32_t*, int32_t*, int32_t*, double*, int32_t*) = ssx_kfdb_project_match;\n'
            'ssx_status (*b)(ssx_kf_database*, const uint8_t*, int32_t, int32_t, int32_t, const ssx_orb_params*, int32_t, const ssx_keypoint*, int32_t, const uint8_t*, '
            'const double*, const double*, int32_t, const int64_t*, const int32_t*, const double*, double, int32_t, int32_t, int32_t*, int32_t*, int32_t*, int32_t*, '
            'double*, int32_t*) = ssx_kfdb_guided_search;\n(void)a; (void)b;' +
            "".join(f'printf("{n} %d\\n", (int)SSX_GUIDED_{n});' for n in names) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t.o")])
        # the enum's values, from the compiler: a program that only prints them needs no library
        vals = "".join(f'printf("{n} %d\\n", (int)SSX_GUIDED_{n});' for n in names)
        open(os.path.join(d, "v.c"), "w").write('#include <stdio.h>\n#include "ssx.h"\nint main(){' + vals + "return 0;}")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "v.c"), "-o", os.path.join(d, "v")])
        out = subprocess.check_output([os.path.join(d, "v")]).decode().split()
    from tools import guided_model as gm
    assert dict(zip(out[0::2], map(int, out[1::2]))) == {n: i for i, n in enumerate(names)} == {n: getattr(gm, n) for n in names}
    assert list(gm.STATUS_NAMES) == names
    header = open(os.path.join(ROOT, "include", "ssx.h")).read()
    at = {name: header.index("SSX_API ssx_status " + name) for name in ("ssx_kfdb_relocalize_query_batch", "ssx_kfdb_project_match", "ssx_kfdb_guided_search")}
    assert at["ssx_kfdb_relocalize_query_batch"] < at["ssx_kfdb_project_match"] < at["ssx_kfdb_guided_search"]   # behind the relocalisation block
    assert re.search(r"\bGuidedSearch\(", open(os.path.join(ROOT, "include", "ssx_shim.hpp")).read()) and "ssx_kfdb_guided_search" in open(os.path.join(ROOT, "include", "ssx_shim.hpp")).read()


def test_the_library_exports_them_and_refuses_without_a_device():
    import ssvio_amd
    from ssvio_amd import build
    from ssvio_amd import loop as sloop
    build.build()
    lib = ssvio_amd.load()
    assert hasattr(lib, "ssx_kfdb_project_match") and hasattr(lib, "ssx_kfdb_guided_search")
    sloop._bind(lib)                                            # the ctypes signatures load
    assert len(lib.ssx_kfdb_project_match.argtypes) == 24 and len(lib.ssx_kfdb_guided_search.argtypes) == 25
    dp, ip, up = sloop.dbl_p, sloop.i32_p, sloop.u8_p
    K4, T = np.array([1.0, 1.0, 0.0, 0.0]), np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    out = np.full(4, 77, np.int32)
    n = np.full(1, 77, np.int32)
    # a null database is refused before anything is looked at: no device is needed, and nothing is written
    st = lib.ssx_kfdb_project_match(None, K4.ctypes.data_as(dp), T.ctypes.data_as(dp), 200, 320, 0, None, None, 0, None, None, 0, None, None, None, 10.0, 50, 90,
                                    out.ctypes.data_as(ip), out.ctypes.data_as(ip), out.ctypes.data_as(ip), out.ctypes.data_as(ip), None, n.ctypes.data_as(ip))
    assert st == -1 and (out == 77).all() and n[0] == 77
    img = np.zeros((200, 320), np.uint8)
    prm = sloop.OrbParams(2000, 1.2, 8, 20, 7)
    st = lib.ssx_kfdb_guided_search(None, img.ctypes.data_as(up), 320, 200, 320, C.byref(prm), 0, None, 8, None, K4.ctypes.data_as(dp), T.ctypes.data_as(dp), 0, None, None,
                                    None, 10.0, 50, 90, None, None, None, None, None, n.ctypes.data_as(ip))
    assert st == -1 and n[0] == 77
    assert lib.ssx_kfdb_project_match(None, None, None, 0, 0, 0, None, None, 0, None, None, 0, None, None, None, 0.0, 0, 0, None, None, None, None, None, None) == -1
    assert lib.ssx_kfdb_guided_search(None, None, 0, 0, 0, None, 0, None, 0, None, None, None, 0, None, None, None, 0.0, 0, 0, None, None, None, None, None, None) == -1
