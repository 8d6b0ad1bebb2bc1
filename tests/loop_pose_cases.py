"""The inputs of tests/test_loop_pose_gpu.py, chosen on the CPU: tests/test_pnp_model.py asserts for every one of them that the
decision of the P3P-RANSAC model is not marginal (each solution of each hypothesis either keeps every ground-truth inlier under
half the threshold or loses at least three of them), so that the GPU test compares decisions, never coin flips.  A case that
breaks the condition gets another seed here; it is not excused there."""
import functools

import numpy as np

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

# Scenes away from identity (a loop closes kilometres from the first camera, at any heading): name -> ground-truth pose T_cw.  yaw170
# takes the y branch of rot_to_quat, y180 has qw = 0 exactly, r120 (120 degrees about (1, 1, 1)) has trace 0 exactly and takes the z
# branch, far (2.6 rad about (-0.84, 0.16, 0.51), the x branch) puts the points 3 km from the world origin, where t = Y0 - R X0 cancels.
_Y170 = np.deg2rad(170.0) / 2
POSES = {"yaw170": np.array([0.0, np.sin(_Y170), 0.0, np.cos(_Y170), 1.5, -1.0, 2.0]),
         "y180": np.array([0.0, 1.0, 0.0, 0.0, -2.0, 1.0, 1.5]),
         "r120": np.array([0.5, 0.5, 0.5, 0.5, 1.0, 2.0, -1.5]),
         "far": np.array([-0.81, 0.15, 0.49, 0.2675, 2000.0, -2000.0, 1000.0])}
POSES["far"][:4] /= np.linalg.norm(POSES["far"][:4])
POSE_OF = {}         # case -> name in POSES (the cases above: the pose make_loop_pose_problem draws)
# problem seeds chosen so that tests/test_pnp_model.py::test_gpu_test_inputs_are_not_marginal holds
_AWAY_SEEDS = {(p, M): 500 + M for p in POSES for M in (64, 257)}
for (_p, _M), _s in _AWAY_SEEDS.items():
    CASES[f"{_p}-{_M}"] = (_M, 0.3, 0.0, _s, 6)
    POSE_OF[f"{_p}-{_M}"] = _p

# The inputs of the refinement test: M -> problem seed (30 % wrong matches, 0.5 px of noise).  256 | 257: one | two edges of a thread;
# 512 | 513 and 1536 | 1537: the two register-resident kernels | the generic one.  tests/test_pnp_model.py asserts that the result of
# the refinement of each does not hang on the last bits of its arithmetic.
REFINE = {10: 918, 256: 1156, 257: 1157, 513: 1413, 1536: 2436, 1537: 2437}
REFINE_SEED = 5      # of the RANSAC that supplies the start
# ... and under the poses away from identity, 257 pairs each: pose -> problem seed
REFINE_AWAY = {"yaw170": 1157, "y180": 1157, "r120": 1157, "far": 1159}
# The oracle's composition against the compiled reference's, max |pose difference|, where it is not at rounding level (measured on the
# CPU as tests/test_pnp_model.py::test_refine_composition_oracle_agrees_with_reference does; the three poses near the origin give 2e-16,
# 1e-12 and 1e-15): 3 km from the origin two LM runs that differ in the last bits end 7e-7 m apart in t.
REFINE_ORACLE_VS_REF = {"far": 6.94e-7}
# The model's RANSAC pose against ground truth on the CPU: (quaternion, up to sign; translation).  Float32 pixels are ~1e-5 px of noise;
# the translation error is the rotation error times |X|.
MODEL_GT_ERR = {"yaw170-64": (7.9e-9, 1.4e-6), "yaw170-257": (3.2e-9, 2.2e-7), "y180-64": (8.1e-9, 1.4e-6), "y180-257": (3.2e-9, 2.3e-7),
                "r120-64": (6.2e-9, 1.4e-6), "r120-257": (3.0e-9, 2.4e-7), "far-64": (7.1e-9, 3.6e-5), "far-257": (2.7e-9, 7.3e-6)}


def pose_err(pose, gt):
    """(largest quaternion difference up to sign -- at half a turn qw = 0 and either sign is the answer --, largest translation difference)"""
    pose, gt = np.asarray(pose), np.asarray(gt)
    return min(np.abs(pose[:4] - gt[:4]).max(), np.abs(pose[:4] + gt[:4]).max()), np.abs(pose[4:] - gt[4:]).max()


def gt_bar(name):
    """the RANSAC pose against ground truth: 4 x the model's measured error, floor 1e-3 (what the cases near identity are held to)"""
    return max(1e-3, 4.0 * max(MODEL_GT_ERR[name])) if name in MODEL_GT_ERR else 1e-3


def refine_bar(M, pose=None):
    """ssx_loop_pose_opt against the oracle's composition: the bars of test_ba_gpu.py's pose-only tests, and 4 x the oracle's own distance
    from the reference where that is larger"""
    return max(1e-8 if M < 8 else 2e-9, 4.0 * REFINE_ORACLE_VS_REF.get(pose, 0.0))


def x_scale(p):
    """how far the scene is from the world origin, in units of the scenes near identity (|X| < 100 m): a rotation error moves t by |X| times it"""
    return max(1.0, np.abs(p["xyz"]).max() / 100.0)


@functools.lru_cache(maxsize=None)
def refine_problem(M, pose=None):
    if pose is None:
        return make_loop_pose_problem(M=M, seed=REFINE[M], frac_gross=0.3, noise_px=0.5)
    assert M == 257
    return make_loop_pose_problem(M=M, seed=REFINE_AWAY[pose], frac_gross=0.3, noise_px=0.5, gt_pose=POSES[pose])


REFINE_PARAMS = [(M, None) for M in REFINE] + [(257, pose) for pose in REFINE_AWAY]
REFINE_IDS = [str(M) if pose is None else f"{pose}-{M}" for M, pose in REFINE_PARAMS]


@functools.lru_cache(maxsize=None)
def problem(name):
    M, frac, noise, seed, _ = CASES[name]
    return make_loop_pose_problem(M=M, seed=seed, frac_gross=frac, noise_px=noise, gt_pose=POSES[POSE_OF[name]] if name in POSE_OF else None)


@functools.lru_cache(maxsize=None)
def model(name):
    """the model's answer, computed once per session and shared (read-only)"""
    p = problem(name)
    return pnp_model.pnp_ransac(p["K"], p["xyz"], p["uv"], H, THR, seed=CASES[name][4], detail=True)
