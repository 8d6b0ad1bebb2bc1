"""CPU: the ctypes mirror of ssx_reloc_query_job (ssvio_amd/loop.py) has the size and the field offsets of the C struct of include/ssx.h,
and the library exports the batched candidate query.  No compute call is made."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reloc_query_job_layout_matches_ctypes():
    from ssvio_amd import loop as sloop
    fields = [name for name, _ in sloop.RelocQueryJob._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ssx.h"\nint main(){printf("sizeof %zu\\n", sizeof(ssx_reloc_query_job));' +
            "".join(f'printf("{f} %zu\\n", offsetof(ssx_reloc_query_job, {f}));' for f in fields) +
            'printf("result %zu\\n", sizeof(ssx_reloc_query_result));return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    c = dict(zip(out[0::2], map(int, out[1::2])))
    assert c.pop("sizeof") == C.sizeof(sloop.RelocQueryJob)
    assert c.pop("result") == C.sizeof(sloop.RelocQueryResult)
    assert len(c) == len(fields) == 10
    for f in fields:
        assert c[f] == getattr(sloop.RelocQueryJob, f).offset, (f, c[f], getattr(sloop.RelocQueryJob, f).offset)


def test_the_library_exports_the_batched_query():
    import ssvio_amd
    from ssvio_amd import build
    build.build()
    lib = ssvio_amd.load()
    assert hasattr(lib, "ssx_kfdb_relocalize_query_batch")
    # n == 0 is answered before anything is looked at, n < 0 refused: neither needs a device
    zero = C.c_float(0)
    assert lib.ssx_kfdb_relocalize_query_batch(None, 0, None, 0, 0, None, 0, 0, zero, zero, 0) == 0
    assert lib.ssx_kfdb_relocalize_query_batch(None, -1, None, 0, 0, None, 0, 0, zero, zero, 0) == -1
