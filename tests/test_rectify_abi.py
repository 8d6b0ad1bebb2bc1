"""CPU: the ABI of lens models and stereo rectification -- the ctypes mirrors have the header's sizes and offsets, the symbols exist, and
ssx_stereo_rectify (host arithmetic: no device) returns the bits of tools/rectify_model.py's rectify and refuses what it refuses."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tools import rectify_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_L, K_R = (40.0, 40.0, 31.5, 23.5), (41.0, 39.5, 32.2, 22.9)
KB_L, RT_R = (-0.02, 0.005, -0.001, 0.0002), (-0.28, 0.07, 0.004, -0.003, 0.01)
ROTATED = dict(R=rm.rot(*np.deg2rad([1.5, -2.0, 1.0])), t=(-0.11, 0.004, -0.003))


def test_struct_sizes_and_offsets_match_the_header():
    from ssvio_amd import _lib
    names = {"ssx_lens_params": _lib.LensParams, "ssx_lens_job": _lib.LensJob, "ssx_stereo_raw_rig": _lib.StereoRawRig, "ssx_stereo_rectified": _lib.StereoRectified}
    fields = [(n, f[0]) for n, cls in names.items() for f in cls._fields_]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ssx.h"\nint main(){' + "".join(f'printf("{n} %zu\\n", sizeof({n}));' for n in names)
            + "".join(f'printf("{n}.{f} %zu\\n", offsetof({n}, {f}));' for n, f in fields) + "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert got[n] == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    for n, f in fields:
        assert got[n + "." + f] == getattr(names[n], f).offset, (n, f)
    assert C.sizeof(_lib.LensParams) == 8 + 18 * 8 and _lib.SSX_LENS_RADTAN == rm.RADTAN == 0 and _lib.SSX_LENS_KB4 == rm.KB4 == 1


def test_symbols_are_exported_and_the_version_stays():
    import ssvio_amd
    from ssvio_amd import _lib
    lib = ssvio_amd.load()
    for sym in ("ssx_undistort_lens", "ssx_undistort_plan_add_lens", "ssx_stereo_rectify", "ssx_lens_debug_atan", "ssx_undistort", "ssx_undistort_plan_add"):
        assert hasattr(lib, sym), sym
    assert lib.ssx_version() == _lib.SSX_VERSION


def _both(models, coeffs, **kw):
    """the library's and the model's rectification of one rig"""
    from ssvio_amd import undistort as ud
    rig = dict(ROTATED)
    rig.update({k: kw.pop(k) for k in ("R", "t") if k in kw})
    Ks = kw.pop("Ks", (K_L, K_R))
    got = ud.stereo_rectify([ud.make_lens_params(m, K, c) for m, K, c in zip(models, Ks, coeffs)], rig["R"], rig["t"], **kw)
    want = rm.rectify(dict(cam=[dict(model=m, K=K, coeffs=c) for m, K, c in zip(models, Ks, coeffs)], R=rig["R"], t=rig["t"], **kw))
    return got, want


def _assert_bits(got, want, models, Ks, coeffs):
    d = lambda a: np.array(a[:], dtype=np.float64).tobytes()
    assert d(got.R_l) == want["R_l"].tobytes() and d(got.R_r) == want["R_r"].tobytes()
    assert d(got.newK) == want["newK"].tobytes() and np.float64(got.baseline).tobytes() == np.float64(want["b"]).tobytes()
    assert d(got.cam[0].iR) == want["iR_l"].tobytes() and d(got.cam[1].iR) == want["iR_r"].tobytes()
    for s in range(2):
        assert got.cam[s].model == models[s] and got.cam[s].reserved == 0
        assert tuple(got.cam[s].K[:]) == tuple(Ks[s]) and tuple(got.cam[s].coeffs[:len(coeffs[s])]) == tuple(coeffs[s])


def test_the_rotated_rig_is_the_models_bits():
    models, coeffs = (rm.KB4, rm.RADTAN), (KB_L, RT_R)
    got, want = _both(models, coeffs)
    _assert_bits(got, want, models, (K_L, K_R), coeffs)
    assert abs(got.baseline - np.linalg.norm(ROTATED["t"])) < 1e-15 and got.R_l[0] > 0.99


def test_random_rigs_are_the_models_bits():
    rng = np.random.default_rng(8)
    models, coeffs = (rm.RADTAN, rm.KB4), (RT_R, KB_L)
    for _ in range(40):
        R = rm.rot(*np.deg2rad(rng.uniform(-8, 8, 3)))
        t = (-rng.uniform(0.05, 0.6), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02))
        Ks = (tuple(rng.uniform(20, 900, 4)), tuple(rng.uniform(20, 900, 4)))
        got, want = _both(models, coeffs, R=R, t=t, Ks=Ks)
        _assert_bits(got, want, models, Ks, coeffs)


def test_the_identity_rig_and_the_overrides():
    from tools import undistort_model as um
    models, coeffs = (rm.RADTAN, rm.RADTAN), (RT_R, RT_R)
    got, want = _both(models, coeffs, R=np.eye(3), t=(-0.537, 0.0, 0.0), Ks=(K_L, K_L))
    _assert_bits(got, want, models, (K_L, K_L), coeffs)
    assert np.array(got.cam[0].iR[:]).tobytes() == um.default_iR(K_L).tobytes() and np.array(got.R_r[:]).tobytes() == np.eye(3).tobytes()
    got, want = _both((rm.KB4, rm.KB4), (KB_L, KB_L), f=22.0, cx=30.0, cy=25.0)
    _assert_bits(got, want, (rm.KB4, rm.KB4), (K_L, K_R), (KB_L, KB_L))
    assert tuple(got.newK[:]) == (22.0, 22.0, 30.0, 25.0)


def test_each_refusal_is_invalid_arg_with_the_models_reason_and_an_untouched_out():
    import ssvio_amd
    from ssvio_amd import _lib
    from ssvio_amd import undistort as ud
    lib = ud._fns(ssvio_amd.load())
    Rbad = np.array(ROTATED["R"]); Rbad[0, 0] += 1e-5
    cases = {
        "model": dict(model=2),
        "finite": dict(t=(np.nan, 0.0, 0.0)),
        "baseline": dict(t=(0.0, 0.0, 0.0)),
        "rotation": dict(R=Rbad),
        "side": dict(t=(0.11, 0.0, 0.0)),
        "axes": dict(R=np.eye(3), t=(-1e-9, 0.0, -0.1)),
    }
    for name, ch in cases.items():
        rig = _lib.StereoRawRig()
        rig.cam[0] = ud.make_lens_params(ch.get("model", rm.KB4), K_L, KB_L)
        rig.cam[1] = ud.make_lens_params(rm.RADTAN, K_R, RT_R)
        rig.R[:] = list(np.asarray(ch.get("R", ROTATED["R"]), dtype=np.float64).reshape(9))
        rig.t[:] = list(ch.get("t", ROTATED["t"]))
        out = _lib.StereoRectified()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        why = C.create_string_buffer(160)
        assert lib.ssx_stereo_rectify(C.byref(rig), C.byref(out), why, len(why)) == _lib.SSX_ERR_INVALID_ARG, name
        assert why.value.decode() == rm.REASONS[name], (name, why.value)
        assert bytes(out) == b"\x5a" * C.sizeof(out), name
        # the wrapper raises the reason; a short or absent buffer is no fault
        short = C.create_string_buffer(b"\x7f" * 8, 8)
        assert lib.ssx_stereo_rectify(C.byref(rig), C.byref(out), short, 8) == _lib.SSX_ERR_INVALID_ARG and short.raw[7:8] == b"\0"
        assert lib.ssx_stereo_rectify(C.byref(rig), C.byref(out), None, 0) == _lib.SSX_ERR_INVALID_ARG
    with pytest.raises(ValueError, match="baseline"):
        ud.stereo_rectify([ud.make_lens_params(rm.KB4, K_L, KB_L)] * 2, np.eye(3), (0.0, 0.0, 0.0))
    assert lib.ssx_stereo_rectify(None, None, None, 0) == _lib.SSX_ERR_INVALID_ARG


def test_shim_rectification_compiles_links_and_runs_its_host_part():
    from ssvio_amd import build
    lib = build.build()
    src = r'''
#include "ssx_shim.hpp"
int main(int argc, char**) {
  ssx_stereo_raw_rig rig{};
  for (int s = 0; s < 2; ++s) { rig.cam[s].model = s == 0 ? SSX_LENS_KB4 : SSX_LENS_RADTAN; rig.cam[s].K[0] = rig.cam[s].K[1] = 40.0; rig.cam[s].K[2] = 31.5; rig.cam[s].K[3] = 23.5; }
  rig.R[0] = rig.R[4] = rig.R[8] = 1.0; rig.t[0] = -0.5;
  const ssx_stereo_rectified r = ssx::StereoRectify(rig);     // host code: runs without a device
  if (!(r.baseline == 0.5 && r.newK[0] == 40.0 && r.R_l[0] == 1.0 && r.cam[0].model == SSX_LENS_KB4 && r.cam[1].iR[0] == 1.0 / 40.0)) return 1;
  if (argc > 100) {   // never executed here (no GPU): only has to compile and link
    ssx::Context ctx(0);
    std::vector<uint8_t> a(48 * 64), b(a.size()), c(a.size()), d(a.size());
    ssx::Camera::RectifyPair(ctx, r.cam, a.data(), 64, b.data(), 64, c.data(), 64, d.data(), 64, 48, 64, false);
    ssx::UndistortPlan plan(ctx, 48, 64);
    return plan.AddLens(r.cam[0]);
  }
  rig.t[0] = 0.5;                                              // the right camera on the left: refused with the reason
  try { ssx::StereoRectify(rig); } catch (const std::invalid_argument& e) { return std::string(e.what()).find("not to the right") != std::string::npos ? 0 : 2; }
  return 3;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.cpp"), lib,
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        assert subprocess.call([exe]) == 0


def test_lens_params_carry_the_model_and_the_default_iR():
    from ssvio_amd import _lib
    from ssvio_amd import undistort as ud
    from tools import undistort_model as um
    p = ud.make_lens_params(_lib.SSX_LENS_KB4, K_L, KB_L)
    assert p.model == 1 and p.reserved == 0 and tuple(p.coeffs[:]) == KB_L + (0.0,)
    assert np.array(p.iR[:]).tobytes() == um.default_iR(K_L).tobytes()
    q = ud.make_lens_params(_lib.SSX_LENS_RADTAN, K_R, RT_R, iR=np.arange(9.0))
    assert q.model == 0 and tuple(q.coeffs[:]) == RT_R and list(q.iR[:]) == list(range(9))
