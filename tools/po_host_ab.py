"""Pose-only / loop-pose host side A/B: two builds of the library must return the same bytes, and their device code must be the same.

    SSX_LIB=<library> python tools/po_host_ab.py out.json     digests of one library's outputs (GPU; a fresh process per library)
    python tools/po_host_ab.py --compare a.json b.json        exit 1 unless every digest is equal
    python tools/po_host_ab.py --asm a.s b.s                  gfx950 assembly of pose_only.hip or pnp.hip of two commits (no GPU):
        hipcc <the flags of ssvio_amd/build.py> --cuda-device-only -S; per kernel the instruction stream, the kernel descriptor and the
        metadata entry must be equal once symbol names, function numbers of labels and the .file / .ident lines are masked
    python tools/po_host_ab.py --times LABEL=FILE ...         (no GPU) the `ms/call` and `fused call` figures of tools/po_time.py and
        tools/loop_pose_time.py outputs, FILEs of the same label being runs of one library: min / median / max per size, and where
        the second label's median lies in the first's min-max (exit 1 if above it)

Digested (sha256 of the bytes of every output):
  tests/pose_only_cases.py RUNS: each through ssx_pose_only_opt, through ssx_pose_only_opt_batch alone, and all as ONE traced batch
      (ssx_pose_only_debug_trace) -- poses, masks, counts, the trace arrays;
  tests/loop_pose_cases.py: CASES through ssx_pnp_ransac and ssx_pnp_debug_counts, REFINE_PARAMS through ssx_loop_pose_opt from the
      RANSAC's pose, and ssx_loop_compute_pose on every case of at least 10 pairs and under every pose of POSES."""
import ctypes as C
import hashlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(r):
    h = hashlib.sha256()
    for k in sorted(r):
        import numpy as np
        h.update(k.encode()); h.update(np.ascontiguousarray(r[k]).tobytes())
    return h.hexdigest()


def outputs():
    import numpy as np
    import loop_pose_cases as lc
    import pose_only_cases as pc
    import ssvio_amd
    from ssvio_amd import ba, loop
    from ssvio_amd._lib import dbl_p, i32_p, ptr
    out = {}
    with ssvio_amd.Context(0) as ctx:
        for n, r, i in pc.RUNS:
            p = pc.problem(n)
            out[f"opt/{pc.run_key(n, r, i)}"] = digest(ba.pose_only_opt(ctx, p["pose"], p["K"], p["xyz"], p["uv"], rounds=r, iters=i))
            out[f"batch1/{pc.run_key(n, r, i)}"] = digest(ba.pose_only_opt_batch(ctx, [p], rounds=r, iters=i)[0])
        res = ba.pose_only_trace(ctx, [pc.problem(n) for n, _, _ in pc.RUNS], [(r, i) for _, r, i in pc.RUNS])
        for (n, r, i), g in zip(pc.RUNS, res):
            out[f"traced/{pc.run_key(n, r, i)}"] = digest(g)
        loop._bind_pose(ctx.lib)
        ctx.lib.ssx_pnp_debug_counts.argtypes = [C.c_void_p, dbl_p, C.c_int32, dbl_p, dbl_p, C.c_int32, C.c_double, C.c_uint32, i32_p]
        ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
        for name, case in lc.CASES.items():
            p, seed = lc.problem(name), case[4]
            out[f"ransac/{name}"] = digest(loop.pnp_ransac(ctx, p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=seed))
            counts = np.zeros(lc.H, np.int32)
            ctx.check(ctx.lib.ssx_pnp_debug_counts(ctx.handle, ptr(p["K"], dbl_p), p["M"], ptr(p["xyz"], dbl_p), ptr(p["uv"], dbl_p), lc.H, lc.THR, seed,
                                                   ptr(counts, i32_p)))
            out[f"counts/{name}"] = digest(dict(counts=counts))
            out[f"compute/{name}"] = digest(loop.compute_correct_pose(ctx, p["xyz"], np.ones(p["M"], np.uint8), p["uv"], p["gt_pose"], ident, p["K"], lc.H, seed=seed))
        for (M, pose), rid in zip(lc.REFINE_PARAMS, lc.REFINE_IDS):
            p = lc.refine_problem(M, pose)
            r = loop.pnp_ransac(ctx, p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=lc.REFINE_SEED)
            out[f"refine/{rid}"] = digest(loop.loop_pose_opt(ctx, r["pose"], p["K"], p["xyz"], p["uv"]))
            out[f"compute-refine/{rid}"] = digest(loop.compute_correct_pose(ctx, p["xyz"], np.ones(M, np.uint8), p["uv"], p["gt_pose"], ident, p["K"], lc.H,
                                                                           seed=lc.REFINE_SEED))
    return out


# ---- --asm -----------------------------------------------------------------------------------------------------------------------
def kernel_of(sym):
    m = re.search(r"k_pose_only_generic|k_pose_onlyILi\d|k_pnp_ransac|k_pnp_p3p_tap|k_pnp_samples", sym)
    return (m.group(0) + ("+trace" if "PoTrace" in sym else "")) if m else sym


def asm_chunks(path):
    """kernel -> its lines: the function with its kernel descriptor; kernel/meta -> its entry of the metadata"""
    out, name = {}, "head"
    for line in open(path):
        m = re.match(r"\t\.section\t\.text\.(\S+?),", line)
        if m:
            name = kernel_of(m.group(1))
        elif line.startswith(("\t.section\t.AMDGPU.gpr_maximums", "\t.type\t__hip_cuid", "\t.amdgpu_metadata")):
            name = "module"
        out.setdefault(name, []).append(line)
    entry = []
    for line in out.get("module", []) + ["amdhsa.target"]:
        if line.startswith(("  - .agpr_count", "amdhsa.target")) and entry:
            out[kernel_of(next(l for l in entry if l.startswith("    .name:"))) + "/meta"] = entry
            entry = []
        if line.startswith("  - .agpr_count") or entry:
            entry.append(line)
    return out


def asm_masked(lines):
    out = []
    for l in lines:
        if re.match(r"\t\.(file|ident)\b", l):
            continue
        l = re.sub(r"_Z[A-Za-z0-9_]+", "SYM", l)
        l = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1N", l)
        l = re.sub(r"\bBB\d+_", "BBN_", l)
        out.append(re.sub(r"__hip_cuid_[0-9a-f]+", "CUID", l))
    return out


def asm_compare(a, b):
    ca, cb = asm_chunks(a), asm_chunks(b)
    bad = 0
    for k in sorted(set(ca) | set(cb)):
        if k in ("head", "module"):
            continue
        la, lb = asm_masked(ca.get(k, [])), asm_masked(cb.get(k, []))
        print(f"{k:32s} {len(la):6d} | {len(lb):6d} lines  {'identical' if la == lb else 'DIFFERENT'}")
        bad += la != lb
    return bad


# ---- --times ---------------------------------------------------------------------------------------------------------------------
def time_figures(path):
    """{size label: milliseconds} of a tools/po_time.py output, {pairs label: microseconds} of a tools/loop_pose_time.py output"""
    out = {}
    for line in open(path):
        m = re.match(r"M\s+(\d+)\s+inliers\s+\d+\s+([\d.]+) ms/call", line)
        if m:
            out[f"ssx_pose_only_opt M {int(m.group(1)):5d} (ms)"] = float(m.group(2))
        m = re.match(r"\s*(\d+)\s+([\d.]+) \(", line)
        if m:
            out[f"ssx_loop_compute_pose {int(m.group(1)):5d} pairs (us)"] = float(m.group(2))
    return out


def times(args):
    runs = {}
    for a in args:
        label, path = a.split("=", 1)
        for k, v in time_figures(path).items():
            runs.setdefault(k, {}).setdefault(label, []).append(v)
    bad = 0
    for k, by in runs.items():
        (la, va), (lb, vb) = list(by.items())[:2]
        med = statistics.median(vb)
        where = "ABOVE" if med > max(va) else "below (faster than)" if med < min(va) else "inside"
        bad += med > max(va)
        f = lambda l, v: f"{l} min {min(v):.3f} median {statistics.median(v):.3f} max {max(v):.3f} ({len(v)} runs)"      # noqa: E731
        print(f"{k:42s} {f(la, va)} | {f(lb, vb)} | {lb} median {where} {la}'s min-max")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        groups = sorted({k.split("/")[0] for k in a})
        for g in groups:
            print(f"{g:16s} {sum(k.startswith(g + '/') for k in a):4d} digests, different: {[k for k in bad if k.startswith(g + '/')]}")
        print("digests", len(a), "|", len(b), "different", len(bad))
        sys.exit(1 if bad or not a else 0)
    if sys.argv[1] == "--asm":
        sys.exit(1 if asm_compare(sys.argv[2], sys.argv[3]) else 0)
    if sys.argv[1] == "--times":
        sys.exit(1 if times(sys.argv[2:]) else 0)
    res = outputs()
    json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
    print("digests", len(res), "library", os.environ.get("SSX_LIB") or "ssvio_amd/libssx.so")
