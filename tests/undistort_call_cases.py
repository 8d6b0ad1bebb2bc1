"""The calls of ssx_undistort and ssx_undistort_plan_apply whose plan (csrc/undistort.hip: UdCall) is held to its rules on the CPU
(tests/test_undistort_call_plan.py), and run through the real entry points on the GPU (tests/test_undistort_call_plan_gpu.py,
tools/undistort_host_ab.py).  All at 45 x 67, the size of tests/test_undistort_gpu.py and tests/test_undistort_plan_gpu.py.

A case states its jobs as the hook takes them -- (src_off, src_stride, dst_off, dst_stride, tag), offsets in bytes from job 0's src --
the facts the runtime would give about each side, the memory that realises it, and what its comments promise: the two intakes and the
copies that carry images.  The byte counts are stated by rule in the tests, not here."""
from ssvio_amd import undistort as ud

ROWS, COLS = 45, 67
IMG = ROWS * COLS                    # 3015
SLICE = 3072                         # an arena's slices: 57 bytes between two images
MAX_JOBS = 1024                      # SSX_UNDISTORT_MAX_JOBS
N_MAPS = 2                           # job k names map k % 2 (or parameter set k % 2)


def _behind(n, ss, ds):
    """n sources one behind the other at a stride of ss, the n destinations behind them at ds"""
    return [(k * ROWS * ss, ss, n * ROWS * ss + k * ROWS * ds, ds, k % N_MAPS) for k in range(n)]


def _arena(n, src_at=None):
    """sources in slices of SLICE bytes (or at src_at[k]), the destinations in the slices behind the last source"""
    src_at = [k * SLICE for k in range(n)] if src_at is None else src_at
    d0 = -(-(max(src_at) + IMG) // SLICE) * SLICE
    return [(src_at[k], COLS, d0 + k * SLICE, COLS, k % N_MAPS) for k in range(n)]


def _pinned(n):
    return (True, [ud.PINNED] * n)


CASES = {}


def _case(name, entry, jobs, memory, on_device, src_intake, dst_intake, copies_up, copies_down, src_facts=None, dst_facts=None, gpu=True):
    CASES[name] = dict(name=name, entry=entry, jobs=jobs, memory=memory, on_device=on_device, src_intake=src_intake, dst_intake=dst_intake,
                       copies_up=copies_up, copies_down=copies_down, src_facts=src_facts, dst_facts=dst_facts, gpu=gpu)


# memory: "host" pageable arrays; "arena" one ssx_host_alloc block the offsets point into; "separate" one ssx_host_alloc per image;
# "device" one device allocation per side; "device to pinned" a device source and an ssx_host_alloc destination
for n in (1, 2, 8):
    for stride in (67, 80):
        _case(f"apply staged n={n} stride={stride}", ud.ENTRY_PLAN_APPLY, _behind(n, stride, stride), "host", False, ud.STAGED, ud.STAGED, 1, 1)
for n in (2, 8):
    _case(f"apply arena n={n}", ud.ENTRY_PLAN_APPLY, _arena(n), "arena", True, ud.RANGE, ud.RANGE, 1, 1, _pinned(n), _pinned(n))
_pitched = [(0, 80, 4 * ROWS * 80, 73, 0), (ROWS * 80, 80, 4 * ROWS * 80 + ROWS * 73 + 64, 73, 1), (2 * ROWS * 80 + 128, 80, 4 * ROWS * 80 + 3 * ROWS * 73, 73, 0)]
_case("apply arena pitched and uneven results", ud.ENTRY_PLAN_APPLY, _pitched, "arena", True, ud.RANGE, ud.EACH, 1, 3, _pinned(3), _pinned(3))
_uneven = [(so, COLS, do + (64 if k == 2 else 0), COLS, m) for k, (so, _, do, _, m) in enumerate(_arena(3))]
_case("apply arena uneven results at a stride of cols", ud.ENTRY_PLAN_APPLY, _uneven, "arena", True, ud.RANGE, ud.EACH, 1, 3, _pinned(3), _pinned(3))
_case("apply several allocations", ud.ENTRY_PLAN_APPLY, _arena(4), "separate", True, ud.EACH, ud.EACH, 4, 4, (False, [ud.PINNED] * 4), (False, [ud.PINNED] * 4))
_case("apply one device allocation", ud.ENTRY_PLAN_APPLY, _arena(4), "device", True, ud.IN_PLACE, ud.IN_PLACE, 0, 0, (True, [ud.DEVICE] * 4),
      (True, [ud.DEVICE] * 4))
_case("apply device source to pinned result", ud.ENTRY_PLAN_APPLY, _arena(1), "device to pinned", True, ud.IN_PLACE, ud.EACH, 0, 1, (False, [ud.DEVICE]),
      (False, [ud.PINNED]))
# the edges of the range's arithmetic, on the sources of a pinned arena: each falls back to a copy per image
_case("apply arena descending sources", ud.ENTRY_PLAN_APPLY, _arena(3, [2 * SLICE, SLICE, 0]), "arena", True, ud.EACH, ud.RANGE, 3, 1, _pinned(3), _pinned(3))
_case("apply arena sources closer than an image", ud.ENTRY_PLAN_APPLY, _arena(3, [0, IMG - 15, 2 * SLICE]), "arena", True, ud.EACH, ud.RANGE, 3, 1, _pinned(3),
      _pinned(3))
_case("apply arena sources over more than 2 n images", ud.ENTRY_PLAN_APPLY, _arena(2, [0, 3 * SLICE]), "arena", True, ud.EACH, ud.RANGE, 2, 1, _pinned(2),
      _pinned(2))
_case("apply arena sources exactly an image apart", ud.ENTRY_PLAN_APPLY, _arena(3, [0, IMG, 2 * IMG]), "arena", True, ud.RANGE, ud.RANGE, 1, 1, _pinned(3),
      _pinned(3))
for n in (1, 2, MAX_JOBS):
    _case(f"undistort staged n={n}", ud.ENTRY_UNDISTORT, _behind(n, 80, 72), "host", False, ud.STAGED, ud.STAGED, 1, 1)
    _case(f"undistort in place n={n}", ud.ENTRY_UNDISTORT, _behind(n, 80, 72), "arena", True, ud.IN_PLACE, ud.IN_PLACE, 0, 0, gpu=n < MAX_JOBS)


def plan_of(case):
    """the hook's answer for a case as it is stated"""
    return ud.debug_plan(case["entry"], ROWS, COLS, case["jobs"], case["on_device"], N_MAPS, case["src_facts"], case["dst_facts"])


def as_text():
    """the cases as lines for tools/undistort_call_check.hip (the builders under the host sanitizers, in a program of their own): per case
    `entry on_device n src_one_allocation dst_one_allocation`, then per job `src_off src_stride dst_off dst_stride tag src_kind dst_kind`"""
    lines = []
    for case in CASES.values():
        n = len(case["jobs"])
        sf, df = (case[s] or (False, [ud.DEVICE] * n) for s in ("src_facts", "dst_facts"))
        lines.append(f"{case['entry']} {int(case['on_device'])} {n} {int(sf[0])} {int(df[0])}")
        lines += [f"{so} {ss} {do} {ds} {tag} {sf[1][k]} {df[1][k]}" for k, (so, ss, do, ds, tag) in enumerate(case["jobs"])]
    return "\n".join(lines) + "\n"


# ---- the real call (GPU) ---------------------------------------------------------------------------------------------------------
def run(ctx, plan, case, imgs, prms):
    """The case through its real entry point on memory of the kind it names: job k reads imgs[k % len(imgs)] under map / parameter set
    k % N_MAPS (plan: an UndistortPlan that holds N_MAPS maps; prms: the UndistortParams of the two sets).
    -> (the n results as arrays, the entry point's last_call(), the jobs as the hook takes them for the pointers the call was given)"""
    import ctypes as C
    import numpy as np
    lib = ctx.lib
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    jobs, n, memory = case["jobs"], len(case["jobs"]), case["memory"]
    pinned, keep = [], []

    def host_alloc(nbytes):
        p = lib.ssx_host_alloc(nbytes)
        assert p
        pinned.append(p)
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))
        a[:] = 0xAB
        return p, a

    def device_alloc(nbytes):
        import torch
        t = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda:0")
        keep.append(t)
        return t.data_ptr(), t

    need = lambda so, ss: so + (ROWS - 1) * ss + COLS                                       # noqa: E731
    src_end = max(need(so, ss) for so, ss, _, _, _ in jobs)
    dst_lo, dst_end = min(do for _, _, do, _, _ in jobs), max(need(do, ds) for _, _, do, ds, _ in jobs)
    try:
        # (address, bytes as an array or a device tensor, offset of the image in it) per image
        if memory in ("host", "arena"):
            p, a = (host_alloc(dst_end) if memory == "arena" else (None, np.full(dst_end, 0xAB, np.uint8)))
            p = a.ctypes.data if p is None else p
            keep.append(a)
            src = [(p + so, a, so) for so, _, _, _, _ in jobs]
            dst = [(p + do, a, do) for _, _, do, _, _ in jobs]
        elif memory == "separate":
            blocks = sorted((host_alloc(IMG) for _ in range(2 * n)), key=lambda b: b[0])        # ascending, as an arena's slices would stand
            src = [(b[0], b[1], 0) for b in blocks[:n]]
            dst = [(b[0], b[1], 0) for b in blocks[n:]]
        else:
            ps, ts = device_alloc(src_end)
            pd, td = device_alloc(dst_end - dst_lo) if memory == "device" else host_alloc(dst_end - dst_lo)
            src = [(ps + so, ts, so) for so, _, _, _, _ in jobs]
            dst = [(pd + do - dst_lo, td, do - dst_lo) for _, _, do, _, _ in jobs]
        for k, (so, ss, _, _, _) in enumerate(jobs):
            _, mem, at = src[k]
            rows = np.full((ROWS, ss), 0xAB, np.uint8)
            rows[:, :COLS] = imgs[k % len(imgs)]
            flat = rows.reshape(-1)[:(ROWS - 1) * ss + COLS]
            if isinstance(mem, np.ndarray):
                mem[at:at + flat.size] = flat
            else:
                import torch
                mem[at:at + flat.size] = torch.from_numpy(flat.copy()).to(mem.device)
        if keep and not isinstance(keep[0], np.ndarray):
            import torch
            torch.cuda.synchronize()
        table = [(src[k][0], ss, dst[k][0], ds, tag) for k, (_, ss, _, ds, tag) in enumerate(jobs)]
        if case["entry"] == ud.ENTRY_PLAN_APPLY:
            plan.apply_ptrs(table, images_on_device=case["on_device"])
            stats = plan.last_call()
        else:
            ud.undistort_ptrs(ctx, [(s, ss, d, ds, prms[tag]) for s, ss, d, ds, tag in table], ROWS, COLS, images_on_device=case["on_device"])
            stats = ud.last_call(ctx)
        outs = []
        for k, (_, _, _, ds, _) in enumerate(jobs):
            _, mem, at = dst[k]
            flat = mem[at:at + (ROWS - 1) * ds + COLS]
            flat = flat if isinstance(flat, np.ndarray) else flat.cpu().numpy()
            full = np.zeros(ROWS * ds, np.uint8)
            full[:flat.size] = flat
            outs.append(full.reshape(ROWS, ds)[:, :COLS].copy())
        facts = [(s - table[0][0], ss, d - table[0][0], ds, tag) for s, ss, d, ds, tag in table]
        return outs, stats, facts
    finally:
        for p in pinned:
            lib.ssx_host_free(p)
