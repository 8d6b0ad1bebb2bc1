"""ORB front-end plan A/B without a GPU: the status, the error text and the three digests of ssx_orb_debug_plan (every scalar of the
device view; every buffer's offset and the arena's bytes; the cell and cv::resize tables byte for byte) must be the same on two builds
of the library.
    python tools/orb_plan_ab.py out.json      (once per library: SSX_LIB=...)      python tools/orb_plan_ab.py --compare a.json b.json
    python tools/orb_plan_ab.py --time [runs]  seconds per pure plan of 1241x376, I = 256 (median of `runs` runs of 200 plans each)
The other side is the parent commit with tools/patches/orb_plan_digest_parent.diff (the same digest over its own plan(), the HIP calls
skipped): in a checkout of the parent, `patch -p0 -i <the patch>`, `python -m ssvio_amd.build`, and SSX_LIB=<its libssx.so>.
Cases: the KITTI shape at I = 1, 2, 256; detect-only with mask at I = 1, 8, 128; every shape and parameter set of tests/test_orb_gpu.py;
the refusals of plan().  tests/test_orb_plan.py checks the structure of the same cases."""
import ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = dict(nfeatures=2000, scale=1.2, nlevels=8, ini=20, mn=7)


def case(rows, cols, I=1, mask=0, detect=0, unchecked=0, **prm):
    return dict(rows=rows, cols=cols, I=I, mask=mask, detect=detect, unchecked=unchecked, **{**DEFAULT, **prm})


K = dict(rows=376, cols=1241)
CASES = (
    [case(**K, I=i) for i in (1, 2, 256)] + [case(**K, I=i, mask=1, detect=1, nfeatures=100) for i in (1, 8, 128)] +
    # tests/test_orb_gpu.py: Detect / DetectAndCompute budgets, with and without mask
    [case(**K, detect=d, nfeatures=n) for n in (100, 300, 2000, 3600) for d in (0, 1)] + [case(**K, mask=1, detect=1, nfeatures=300)] +
    [case(160, 260, nfeatures=300, nlevels=4, mask=m) for m in (0, 1)] + [case(160, 260, nfeatures=2000), case(160, 260, nfeatures=300, nlevels=4, ini=60, mn=5)] +
    # the four other pyramids, on both images
    [case(r, c, nfeatures=n, scale=s, nlevels=l) for (s, l, n) in ((1.5, 4, 400), (2.0, 3, 300), (2.3, 3, 300), (1.1, 6, 500)) for (r, c) in ((160, 260), (376, 1241))] +
    # tiny budgets on a wide image
    [case(368, 1341, detect=d, nfeatures=n, nlevels=l, scale=s, ini=35, mn=3) for (n, l, s) in ((50, 8, 1.1), (8, 8, 1.2), (20, 3, 1.5)) for d in (0, 1)] +
    # more levels than pixels
    [case(h, w, nfeatures=n, nlevels=l, scale=s, ini=10, mn=3) for (h, w, n, l, s) in ((48, 79, 300, 8, 2.0), (63, 69, 2000, 8, 2.0), (40, 40, 100, 8, 1.5))] +
    # other sizes (octree keys in LDS / in global scratch)
    [case(h, w, detect=d, nfeatures=n) for (h, w) in ((479, 641), (720, 1280), (1080, 1920)) for (d, n) in ((0, 2000), (1, 300))] +
    # degenerate small images
    [case(h, w, nlevels=l, nfeatures=n) for (h, w, l, n) in ((100, 130, 8, 500), (60, 90, 8, 200), (41, 41, 8, 50), (45, 300, 6, 300), (300, 45, 6, 300))] +
    # streamed batches, the stereo frame and batch of the other GPU tests
    [case(200, 320, I=8, nfeatures=300, nlevels=4), case(120, 200, nfeatures=100, nlevels=3), case(120, 200, I=2, mask=1, detect=1, nfeatures=100, nlevels=3)])

INVALID, UNSUPPORTED = -1, -5
# name -> (case, status, start of the error text).  The argument checks come first; `unchecked` cases reach the refusals behind them.
FAILING = {
    "image":        (case(100000, 160, detect=1, nfeatures=100, nlevels=3), INVALID, "ssx_orb: image 160x100000 outside"),
    "image_small":  (case(38, 200), INVALID, "ssx_orb: image 200x38 outside"),
    "levels_0":     (case(100, 160, nfeatures=100, nlevels=0), INVALID, "ssx_orb: unsupported parameters (nlevels=0 "),
    "levels_40":    (case(100, 160, nfeatures=100, nlevels=40), INVALID, "ssx_orb: unsupported parameters (nlevels=40 "),
    "levels_40_u":  (case(100, 160, nfeatures=100, nlevels=40, unchecked=1), INVALID, "ssx_orb: unsupported parameters (nlevels=40 "),   # (always checked)
    "scale_0.9":    (case(100, 160, nfeatures=100, nlevels=3, scale=0.9), INVALID, "ssx_orb: unsupported parameters"),
    "budget_-5":    (case(100, 160, nfeatures=-5, nlevels=3), INVALID, "ssx_orb: unsupported parameters"),
    "budget_big":   (case(100, 160, nfeatures=4089, nlevels=3), INVALID, "ssx_orb: unsupported parameters"),
    "images_0":     (case(100, 160, I=0), INVALID, "ssx_orb: unsupported parameters"),
    "level_cap":    (case(**K, nfeatures=20000, unchecked=1), UNSUPPORTED, "ssx_orb: 4343 features on level 0 exceed"),
    "octree_roots": (case(62, 2000, detect=1, nfeatures=100), UNSUPPORTED, "ssx_orb: level 0 (2000x62) is 66 times as wide as high"),
    "octree_lds":   (case(8000, 8000, detect=1, nfeatures=100, unchecked=1), UNSUPPORTED, "ssx_orb: 66049 grid cells on one level exceed"),
    "resize_scale": (case(400, 4000, nlevels=2, scale=100.0), UNSUPPORTED, "ssx_orb: pyramid scale factor 100 is too large"),
    # two reasons at once: the earlier one in plan()'s order is reported
    "image+params":        (case(30, 160, nlevels=0), INVALID, "ssx_orb: image 160x30 outside"),
    "params+resize":       (case(400, 4000, nlevels=2, scale=100.0, nfeatures=0), INVALID, "ssx_orb: unsupported parameters"),
    "level_cap+octree":    (case(8000, 8000, nfeatures=20000, nlevels=2, unchecked=1), UNSUPPORTED, "ssx_orb: 10909 features on level 0 exceed"),
    "level_cap+roots":     (case(62, 2000, nfeatures=20000, nlevels=2, unchecked=1), UNSUPPORTED, "features on level 0 exceed"),
    "roots+resize":        (case(62, 2000, nlevels=2, scale=100.0), UNSUPPORTED, "times as wide as high"),
    "level_cap+resize":   (case(400, 4000, nfeatures=20000, nlevels=2, scale=100.0, unchecked=1), UNSUPPORTED, "features on level 0 exceed"),
    "octree+resize":       (case(8000, 8000, nlevels=2, scale=100.0, unchecked=1), UNSUPPORTED, "grid cells on one level exceed"),
}


class PlanInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_buffers", C.c_int32), ("digest", C.c_uint64 * 3), ("arena_bytes", C.c_uint64), ("buf_off", C.c_uint64 * 32),
                ("buf_bytes", C.c_uint64 * 32), ("nlevels", C.c_int32), ("out_cap", C.c_int32), ("lvl_rows", C.c_int32 * 8), ("lvl_cols", C.c_int32 * 8),
                ("feat", C.c_int32 * 8), ("lvl_cell0", C.c_int32 * 9), ("gauss_tile0", C.c_int32 * 9), ("error", C.c_char * 256)]


def plan_info(lib, c):
    from ssvio_amd import _lib
    prm = _lib.OrbParams(c["nfeatures"], c["scale"], c["nlevels"], c["ini"], c["mn"])
    info = PlanInfo()
    lib.ssx_orb_debug_plan.restype = C.c_int32
    lib.ssx_orb_debug_plan.argtypes = [C.c_int32] * 3 + [C.POINTER(_lib.OrbParams)] + [C.c_int32] * 3 + [C.POINTER(PlanInfo)]
    st = lib.ssx_orb_debug_plan(c["rows"], c["cols"], c["I"], C.byref(prm), c["mask"], c["detect"], c["unchecked"], C.byref(info))
    assert st == info.status
    return info


def name(c):
    return "%(rows)dx%(cols)d/I%(I)d/m%(mask)d/d%(detect)d/u%(unchecked)d/n%(nfeatures)d/s%(scale)g/l%(nlevels)d/t%(ini)d-%(mn)d" % c


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        zero = [k for k in sorted(a) if a[k]["status"] == 0 and "0" * 16 in a[k]["digest"]]
        print("cases", len(a), "digests", sum(len(v["digest"]) for v in a.values()), "zero", zero, "different", bad)
        sys.exit(1 if bad or zero or not a else 0)
    from ssvio_amd import _lib
    lib = _lib.load()
    if sys.argv[1] == "--time":
        c = case(**K, I=256)
        runs = []
        for _ in range(int(sys.argv[2]) if len(sys.argv) > 2 else 5):
            t0 = time.perf_counter()
            for _ in range(200):
                plan_info(lib, c)
            runs.append((time.perf_counter() - t0) / 200)
        print("seconds per plan: median %.3e min %.3e max %.3e  %s" % (statistics.median(runs), min(runs), max(runs), " ".join("%.3e" % r for r in runs)))
        sys.exit(0)
    res = {}
    for c in CASES + [f[0] for f in FAILING.values()]:
        info = plan_info(lib, c)
        res[name(c)] = dict(status=info.status, error=info.error.decode(), digest=["%016x" % d for d in info.digest] if info.status == 0 else [])
    json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
    print("cases", len(res), "ok", sum(v["status"] == 0 for v in res.values()), "refused", sum(v["status"] != 0 for v in res.values()))
