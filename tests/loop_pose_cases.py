"""The inputs of tests/test_loop_pose_gpu.py, chosen on the CPU: tests/test_pnp_model.py asserts for every one of them that the
decision of the P3P-RANSAC model is not marginal (each solution of each hypothesis either keeps every ground-truth inlier under
half the threshold or loses at least three of them), so that the GPU test compares decisions, never coin flips.  A case that
breaks the condition gets another seed here; it is not excused there."""
import functools

from tools import pnp_model
from tools.synth import make_loop_pose_problem

H = 100              # the reference's iterationsCount
THR = 5.991          # the reference's reprojectionError
SIZES = (10, 64, 65, 257, 1000)

# name -> (M, frac_gross, noise_px, problem seed, RANSAC seed)
CASES = {}
for _M in SIZES:
    CASES[f"clean-{_M}"] = (_M, 0.0, 0.0, 100 + _M, 1)
    CASES[f"out30-{_M}"] = (_M, 0.3, 0.0, 202 + _M, 2)
    CASES[f"out60-{_M}"] = (_M, 0.6, 0.0, 300 + _M, 3)
CASES["noisy-257"] = (257, 0.3, 0.5, 457, 4)

# The inputs of the refinement test: M -> problem seed (30 % wrong matches, 0.5 px of noise).  256 | 257: one | two edges of a thread;
# 512 | 513 and 1536 | 1537: the two register-resident kernels | the generic one.  tests/test_pnp_model.py asserts that the result of
# the refinement of each does not hang on the last bits of its arithmetic.
REFINE = {10: 918, 256: 1156, 257: 1157, 513: 1413, 1536: 2436, 1537: 2437}
REFINE_SEED = 5      # of the RANSAC that supplies the start


@functools.lru_cache(maxsize=None)
def refine_problem(M):
    return make_loop_pose_problem(M=M, seed=REFINE[M], frac_gross=0.3, noise_px=0.5)


@functools.lru_cache(maxsize=None)
def problem(name):
    M, frac, noise, seed, _ = CASES[name]
    return make_loop_pose_problem(M=M, seed=seed, frac_gross=frac, noise_px=noise)


@functools.lru_cache(maxsize=None)
def model(name):
    """the model's answer, computed once per session and shared (read-only)"""
    p = problem(name)
    return pnp_model.pnp_ransac(p["K"], p["xyz"], p["uv"], H, THR, seed=CASES[name][4], detail=True)
