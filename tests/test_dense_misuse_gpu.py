"""GPU: every misuse of ssx_stereo_dense returns SSX_ERR_INVALID_ARG with a message in ssx_last_error, launches nothing and leaves the
output untouched; a valid call right after still gives the model's bytes."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import dense as dn
from tools import dense_model as dm
from tools.synth import make_stereo_pair

pytestmark = pytest.mark.gpu
ROWS, COLS = 40, 48


def _call(ctx, left, right, disp, prm, n=1, rows=ROWS, cols=COLS, strides=(COLS, COLS, COLS), jobs_null=False, prm_null=False):
    lib = dn._fns(ctx.lib)
    job = _lib.DenseJob(left, strides[0], right, strides[1], disp, strides[2])
    arr = (_lib.DenseJob * 1)(job)
    return lib.ssx_stereo_dense(ctx.handle, n, None if jobs_null else arr, rows, cols, None if prm_null else C.byref(prm), 0)


def test_every_refusal_is_invalid_arg_with_a_message_and_an_untouched_output(ctx):
    L, R, _ = make_stereo_pair(seed=2, h=ROWS, w=COLS, n_blobs=20, bf=60.0)
    disp = np.full((ROWS, COLS), 0x5a5a, dtype=np.int16)
    l, r, d = L.ctypes.data, R.ctypes.data, disp.ctypes.data
    ok = dict(disparities=64)

    def prm(**kw):
        p = dn.DenseParams(**{**ok, **{k: v for k, v in kw.items() if k != "reserved"}})
        if "reserved" in kw:
            p.reserved[kw["reserved"]] = 1
        return p

    cases = {
        "disparities 32": dict(prm=prm(disparities=32)),
        "disparities 96": dict(prm=prm(disparities=96)),
        "disparities 256": dict(prm=prm(disparities=256)),
        "p1 0": dict(prm=prm(p1=0)),
        "p2 below p1": dict(prm=prm(p1=20, p2=19)),
        "p2 193": dict(prm=prm(p2=193)),
        "uniqueness -1": dict(prm=prm(uniqueness=-1)),
        "uniqueness 100": dict(prm=prm(uniqueness=100)),
        "lr_tolerance -2": dict(prm=prm(lr_tolerance=-2)),
        "paths 5": dict(prm=prm(paths=5)),
        "paths 16": dict(prm=prm(paths=16)),
        "reserved 0": dict(prm=prm(reserved=0)),
        "reserved 1": dict(prm=prm(reserved=1)),
        "null prm": dict(prm=prm(), prm_null=True),
        "null jobs": dict(prm=prm(), jobs_null=True),
        "null left": dict(prm=prm(), left=None),
        "null right": dict(prm=prm(), right=None),
        "null disp": dict(prm=prm(), disp=None),
        "left stride": dict(prm=prm(), strides=(COLS - 1, COLS, COLS)),
        "right stride": dict(prm=prm(), strides=(COLS, COLS - 1, COLS)),
        "disp stride": dict(prm=prm(), strides=(COLS, COLS, COLS - 1)),
        "n -1": dict(prm=prm(), n=-1),
        "n above the limit": dict(prm=prm(), n=_lib.SSX_DENSE_MAX_JOBS + 1),
        "rows 39": dict(prm=prm(), rows=39),
        "cols 4001": dict(prm=prm(), cols=4001, strides=(4001, 4001, 4001)),
    }
    for name, kw in cases.items():
        args = dict(left=l, right=r, disp=d)
        args.update(kw)
        st = _call(ctx, args.pop("left"), args.pop("right"), args.pop("disp"), args.pop("prm"), **args)
        assert st == _lib.SSX_ERR_INVALID_ARG, name
        msg = ctx.lib.ssx_last_error(ctx.handle).decode()
        assert msg.startswith("ssx_stereo_dense:") and len(msg) > 20, (name, msg)
        assert np.all(disp == 0x5a5a), name
        assert dn.last_call(ctx) == dict(launches=0, syncs=0, bytes_up=0, bytes_down=0, groups=0), name
    # a null context has nowhere to leave a message
    assert dn._fns(ctx.lib).ssx_stereo_dense(None, 0, None, ROWS, COLS, None, 0) == _lib.SSX_ERR_INVALID_ARG
    # a valid call right after: the model's bytes
    got = dn.dense_disparity(ctx, L, R, prm())
    assert np.array_equal(got, dm.disparity(L, R, dm.DenseParams(disparities=64)))
    # and no pair at all is no error
    assert _call(ctx, l, r, d, prm(), n=0) == _lib.SSX_OK and np.all(disp == 0x5a5a)
