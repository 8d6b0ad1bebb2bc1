"""The LK calls of tests/lk_call_cases.py through the real entry points, each image layout as its case names it.

    python tools/lk_call_trace.py                      replay every case on GPU 0 and print a digest of the results per case
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python tools/lk_call_trace.py
    python tools/lk_call_trace.py --compare DIR_A DIR_B   the two traces' sequences of (kernel, grid, workgroup) and of (copy direction,
                                                       bytes), side by side: equal or the first difference

SSX_LIB=<another libssx.so> replays the cases on another build of the library (the A/B of profiles/lk_host_plan/trace_ab.txt).
Replay (class Replay) is also what tests/test_lk_gpu.py::test_every_image_intake_gives_the_same_bits runs."""
import csv
import ctypes as C
import functools
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import numpy as np

import lk_call_cases as cc


@functools.lru_cache(maxsize=None)
def base_image(seed, h, w):
    from tools.synth import make_stereo_pair
    return make_stereo_pair(seed=seed, h=h, w=w, n_blobs=max(60, h * w // 150))[0]


class Replay:
    """One case on one context: .run(call) -> [(next_pts, status, err)] per job; .pairs holds the (prev, next) images of the last call."""

    def __init__(self, ctx, c):
        self.ctx, self.c = ctx, c
        lib = ctx.lib
        lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
        lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
        h, w = c["h"], c["w"]
        slots = sorted({s for k in c["calls"] for s in k["slots"]})
        base = {s: base_image(60 + s, h, w) for s in slots}
        self.frames = {s: [np.ascontiguousarray(np.roll(base[s], (t * (s % 2), t * (1 + s % 3)), (0, 1))) for t in range(len(c["calls"]) + 1)] for s in slots}
        self.cur = {s: 0 for s in slots}                               # the frame each slot's kept pyramid belongs to
        self.kw = dict(winSize=c["win"], maxLevel=c["max_level"])

    def points(self, n):
        i = np.arange(n)
        return np.stack([6 + (i * 37) % (self.c["w"] - 12), 6 + (i * 53) % (self.c["h"] - 12)], 1).astype(np.float32) + np.float32(0.25)

    def pinned(self, nbytes):
        p = self.ctx.lib.ssx_host_alloc(nbytes)
        if not p:
            raise MemoryError("ssx_host_alloc")
        self.pins.append(p)
        return p

    def place(self, k, images):
        """the call's `next` images (or, second use, its previous ones) where the layout wants them -> addresses, job by job"""
        layout, d = k["layout"], cc.slice_bytes(self.c)
        if layout in (cc.ARENA, cc.ARENA_SKIP):
            offs = cc.next_offsets(self.c, k)
            block = self.pinned(max(offs) + d)
            for o, img in zip(offs, images):
                if img is not None:
                    C.memmove(block + o, img.ctypes.data, img.size)
            return [block + o for o in offs]
        if layout == cc.SEPARATE_HOST:
            addr = sorted((self.pinned(self.c["h"] * self.c["w"]) for _ in images), reverse=True)
            for a, img in zip(addr, images):
                if img is not None:
                    C.memmove(a, img.ctypes.data, img.size)
            return addr
        import torch
        bufs = sorted((torch.empty(self.c["h"] * self.c["w"], dtype=torch.uint8, device="cuda") for _ in images), key=lambda t: -t.data_ptr())
        for t, img in zip(bufs, images):
            if img is not None:
                t.copy_(torch.from_numpy(img.reshape(-1)))
        torch.cuda.synchronize()
        self.bufs += bufs
        return [t.data_ptr() for t in bufs]

    def run(self, k):
        from ssvio_amd import lk
        self.pins, self.bufs = [], []
        self.pairs = [(self.frames[s][self.cur[s]] if f else None, self.frames[s][self.cur[s] + 1]) for s, f in zip(k["slots"], k["fresh"])]
        self.pts = [self.points(n) for n in k["n"]]
        jobs = [dict(slot=s, prev_pts=p, next_pts=p) for s, p in zip(k["slots"], self.pts)]
        try:
            if k["layout"] == cc.HOST:
                for j, (prev, nxt) in zip(jobs, self.pairs):
                    j.update(prev=prev, next=nxt)
                out = lk.track_batch(self.ctx, jobs, **self.kw)
            else:
                nxt, prev = self.place(k, [b for _, b in self.pairs]), self.place(k, [a for a, _ in self.pairs])
                for j, (a, _), pa, na in zip(jobs, self.pairs, prev, nxt):
                    j.update(prev=None if a is None else pa, next=na, stride=self.c["w"])
                out = lk.track_batch_ptrs(self.ctx, jobs, self.c["h"], self.c["w"], **self.kw)
        finally:
            for p in self.pins:
                self.ctx.lib.ssx_host_free(p)
            self.bufs = []
        for s in k["slots"]:
            self.cur[s] += 1
        return out


def compare(dir_a, dir_b):
    def rows(d, what):
        f = sorted(glob.glob(d + f"/**/*{what}.csv", recursive=True))
        return sorted(csv.DictReader(open(f[-1])), key=lambda r: int(r["Start_Timestamp"])) if f else []

    def kernels(d):
        return [(r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"))
                for r in rows(d, "kernel_trace")]

    def copies(d):
        rs = rows(d, "memory_copy_trace")
        size = next((k for k in (rs[0] if rs else {}) if k.lower() in ("bytes", "size", "copy_size", "transfer_size")), None)
        return [(r["Direction"], int(r[size]) if size else None) for r in rs], size

    ok = True
    for what, a, b in (("kernel launches (name, grid, workgroup)", kernels(dir_a), kernels(dir_b)),
                       ("memory copies (direction, %s)" % (copies(dir_a)[1] or "this profiler's copy rows carry no size; copies made by a blit kernel show theirs as its grid"), copies(dir_a)[0], copies(dir_b)[0])):
        diff = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        print(f"{what}: A {len(a)}, B {len(b)}: " + ("EQUAL sequences" if diff is None else f"FIRST DIFFERENCE at {diff}: A {a[diff:diff + 1]} B {b[diff:diff + 1]}"))
        ok = ok and diff is None and len(a) > 0
        lk_rows = [x for x in a if isinstance(x[0], str) and "k_lk_" in x[0]]
        if lk_rows:
            print("  of them LK kernels: " + ", ".join(f"{n} x {sum(1 for x in lk_rows if x[0] == n)}" for n in sorted({x[0] for x in lk_rows})))
    return 0 if ok else 1


def main():
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        return compare(sys.argv[i + 1], sys.argv[i + 2])
    import ssvio_amd
    ctx = ssvio_amd.Context(0)
    for c in cc.CASES:
        r = Replay(ctx, c)
        h = hashlib.sha256()
        for k in c["calls"]:
            for o in r.run(k):
                for a in o:
                    h.update(a.tobytes())
        print(f"{c['name']:44s} {h.hexdigest()[:16]}", flush=True)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
