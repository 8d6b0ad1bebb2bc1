"""GPU: the minimal solver of ssvio_amd/csrc/pnp.hip (p3p_solve, rot_to_quat) through its tap ssx_pnp_debug_p3p, one launch over the
whole of tests/golden/p3p_hp.npz: against the model (tools/pnp_model.py) to the byte -- the documented contract -- and, independently
of the model, against the 60-digit reference of the fixture alone (complete, accurate, sound: tests/p3p_cases.py::check)."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd._lib import SSX_ERR_INVALID_ARG, dbl_p, i32_p, ptr

import p3p_cases as pc

pytestmark = pytest.mark.gpu


def _lib(ctx):
    ctx.lib.ssx_pnp_debug_p3p.argtypes = [C.c_void_p, dbl_p, C.c_int32, dbl_p, dbl_p, i32_p, dbl_p, dbl_p, dbl_p]
    return ctx.lib


def _tap(ctx, K, X, uv):
    n = len(X)
    X, uv = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(uv, dtype=np.float64)
    valid, R, t, pose = np.full((n, 4), -1, np.int32), np.full((n, 4, 3, 3), np.nan), np.full((n, 4, 3), np.nan), np.full((n, 4, 7), np.nan)
    ctx.check(_lib(ctx).ssx_pnp_debug_p3p(ctx.handle, ptr(np.ascontiguousarray(K, dtype=np.float64), dbl_p), n, ptr(X, dbl_p), ptr(uv, dbl_p),
                                          ptr(valid, i32_p), ptr(R, dbl_p), ptr(t, dbl_p), ptr(pose, dbl_p)))
    return valid, R, t, pose


@pytest.fixture(scope="module")
def tap(ctx):
    """the one launch, shared (read-only)"""
    fx = pc.fixture()
    return _tap(ctx, fx["K"], fx["X"], fx["uv"])


def test_tap_equals_the_model_to_the_byte(tap):
    fx = pc.fixture()
    valid, R, t, pose = tap
    m_valid, m_R, m_t, m_pose = pc.model_output()
    assert set(np.unique(valid)) <= {0, 1}
    diff = np.nonzero((valid != m_valid).any(axis=1))[0]
    assert len(diff) == 0, [(str(fx["names"][i]), valid[i].tolist(), m_valid[i].tolist()) for i in diff]
    for name, a, b in (("R", R, m_R), ("t", t, m_t), ("pose", pose, m_pose)):
        bad = [str(fx["names"][i]) for i in range(len(a)) if a[i].tobytes() != b[i].tobytes()]
        worst = np.abs(a - b).max()
        assert not bad, (name, len(bad), bad[:8], worst)


def test_tap_is_complete_accurate_and_sound_against_the_reference(tap):
    """the kernel against the fixture alone: bar per class = max(1e-9, 4 x the model's worst error), measured by the generator"""
    fx = pc.fixture()
    valid, R, t, pose = tap
    worst = pc.check(fx, valid, R, t, pose, fx["bar"], zero_invalid=True)
    print("kernel worst per class:", {str(c): (float(w), float(b)) for c, w, b in zip(fx["classes"], worst, fx["bar"])})


def test_tap_does_not_depend_on_the_batch(ctx, tap):
    """one thread per triple: a triple alone, and the last 65 (two workgroups, one of a single thread), give the bytes of the whole launch"""
    fx = pc.fixture()
    for sl in (slice(0, 1), slice(len(fx["n"]) - 65, None)):
        part = _tap(ctx, fx["K"], fx["X"][sl], fx["uv"][sl])
        for a, b in zip(part, tap):
            assert a.tobytes() == b[sl].tobytes()


def test_misuse_is_refused_and_the_context_stays_usable(ctx, tap):
    fx = pc.fixture()
    lib = _lib(ctx)
    K, X, uv = fx["K"], np.ascontiguousarray(fx["X"][:4]), np.ascontiguousarray(fx["uv"][:4])
    out = dict(valid=np.full((4, 4), 7, np.int32), R=np.full((4, 4, 9), 7.0), t=np.full((4, 4, 3), 7.0), pose=np.full((4, 4, 7), 7.0))

    def call(handle=ctx.handle, K=K, n=4, X=X, uv=uv, **kw):
        o = dict(out)
        o.update(kw)
        return lib.ssx_pnp_debug_p3p(handle, ptr(K, dbl_p), n, ptr(X, dbl_p), ptr(uv, dbl_p), ptr(o["valid"], i32_p), ptr(o["R"], dbl_p),
                                     ptr(o["t"], dbl_p), ptr(o["pose"], dbl_p))
    for kw in (dict(handle=None), dict(K=None), dict(n=-1), dict(X=None), dict(uv=None), dict(valid=None), dict(R=None), dict(t=None), dict(pose=None),
               dict(K=K * np.array([1, np.nan, 1, 1])), dict(K=K * np.array([np.inf, 1, 1, 1]))):
        assert call(**kw) == SSX_ERR_INVALID_ARG, kw
    assert all((v == 7).all() for v in out.values())                       # a refused call writes nothing
    assert call(n=0) == 0 and lib.ssx_pnp_debug_p3p(ctx.handle, ptr(K, dbl_p), 0, None, None, None, None, None, None) == 0
    assert all((v == 7).all() for v in out.values())                       # n = 0 does nothing
    assert call() == 0
    assert out["valid"].tobytes() == tap[0][:4].tobytes() and out["R"].tobytes() == tap[1][:4].tobytes()
