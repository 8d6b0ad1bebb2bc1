"""A small there-and-back drive that revisits its start with real drift, for the loop-closing tests and profiles.

The rig of tools.synth.make_lateral_sequence moves sideways to `reach` baselines and comes back: the return leg shows the outbound
LEFT images in reverse order, but its RIGHT images are rendered `right_factor` baselines beside the left camera while the settings
keep stating one baseline.  Every map point triangulated on the way back is therefore too near by that factor, the return leg is
measured too short by it, and the trajectory arrives beside the start instead of on it -- until a loop is closed.

The offsets ease in and out (half a cosine), so the velocity is zero at both ends and reverses smoothly at the far end: the
constant-velocity guess of the tracker stays good through the turn.

view_width: the lateral distance after which a point at the scene's MEDIAN depth has crossed the whole image (w pixels / its
disparity, in baselines, times the baseline).  `reach` is chosen beyond it: of what the far end sees, only the farthest strips of
the scene are still in view at the start."""
from __future__ import annotations

import os

import numpy as np

from tools import synth


def make_loop_drive(root, n_leg=40, reach=14.0, right_factor=1.5, seed=0, h=200, w=320, n_blobs=1500, dt=0.1, fx=synth.KITTI_K[0]):
    """Writes <root>/seq in KITTI layout (2 * n_leg - 1 stereo pairs).  -> dict(dir, dt, centres [n,3] ground truth, n_frames, view_width,
    K = (fx, fy, cx, cy), bf)."""
    from PIL import Image
    K = (float(fx), float(fx), w / 2.0, h / 2.0)
    baseline = synth.KITTI_BF / float(fx)                                  # the rig the settings state: Camera.Base.Line / fx
    out_alphas = reach * (1.0 - np.cos(np.pi * np.arange(n_leg) / (n_leg - 1))) / 2.0
    kw = dict(seed=seed, h=h, w=w, n_blobs=n_blobs, alphas=out_alphas)
    outbound, gt, disp = synth.make_lateral_sequence(**kw)
    wide, _, _ = synth.make_lateral_sequence(right_alpha=right_factor, **kw)
    frames = list(outbound) + [(outbound[k][0], wide[k][1]) for k in range(n_leg - 2, -1, -1)]
    alphas = np.concatenate([out_alphas, out_alphas[-2::-1]])
    centres = np.stack([alphas * baseline, np.zeros(len(alphas)), np.zeros(len(alphas))], 1)
    d = os.path.join(root, "seq")
    for sub in ("image_0", "image_1"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    with open(os.path.join(d, "times.txt"), "w") as f:
        for i, (L, R) in enumerate(frames):
            f.write(f"{i * dt:e}\n")
            Image.fromarray(L).save(os.path.join(d, "image_0", f"{i:06d}.png"))
            Image.fromarray(R).save(os.path.join(d, "image_1", f"{i:06d}.png"))
    view_width = float(w / np.median(disp)) * baseline
    return dict(dir=d, dt=dt, centres=centres, n_frames=len(frames), view_width=view_width, K=K, bf=synth.KITTI_BF)


def drive_settings(drive, overrides=None):
    """the settings of the drive: the camera of its images, a keyframe on every frame, a window of 5"""
    fx, fy, cx, cy = drive["K"]
    cfg = {"Camera1.fx": fx, "Camera1.fy": fy, "Camera1.cx": cx, "Camera1.cy": cy, "Camera2.fx": fx, "Camera2.fy": fy, "Camera2.cx": cx, "Camera2.cy": cy,
           "Camera.width": 320, "Camera.height": 200, "Camera.Base.Line": drive["bf"], "Map.ActiveMap.Size": 5, "numFeatures.trackingGood": 100000,
           "Min.Init.Landmark.Num": 100}
    cfg.update(overrides or {})
    return cfg


def end_point_error(traj_path, drive):
    """|last keyframe centre - first keyframe centre - ground truth| of a TUM trajectory with a keyframe on every frame"""
    tum = np.loadtxt(traj_path, ndmin=2)
    frame = np.rint(tum[:, 0] / drive["dt"]).astype(int)
    est = tum[:, 1:4] - tum[0, 1:4]
    gt = drive["centres"][frame] - drive["centres"][frame[0]]
    return float(np.linalg.norm(est[-1] - gt[-1])), est, gt, frame
