"""The inputs of tests/test_lk_image_cases.py (CPU) and tests/test_lk_images_gpu.py (GPU): made images, motions and points for the
pyramidal Lucas-Kanade tracker (ssvio_amd/csrc/lk.hip), built deterministically with plain numpy (the two blob images come from
tools.synth, which is numpy too); every array is read-only.

tests/test_lk_gpu.py draws every image with tools.synth.make_stereo_pair and moves it by a pixel or two per level.  The families
here are what that never gives:

  A  geometry   image sizes at which the smaller side of the top level is exactly the least k_lk_pyramid accepts (border + 2), one
                less, exactly the border (win + 1: two reflections), images smaller than the window, and eight levels
  B  steps      a smooth image moved, inside ONE level, further than the margin of the 32 x 32 neighbourhood k_lk_track keeps in
                LDS: the neighbourhood is copied again (stage_region / region_holds)
  C  limits     maxCount 0 (no iteration: the error step copies the neighbourhood itself), 1, 2, the clamps of TermCriteria
  D  texture    flat, saturated, striped, checkered and ramp images under minEigThreshold 0 .. 100
  G  coordinates  NaN, infinities, values beyond the int range, a denormal, the last sub-pixel of the image

What each case claims -- the level lists, the number of points that moved further than the margin, the points kept -- is asserted
from the CPU oracle alone in tests/test_lk_image_cases.py, so that a GPU comparison cannot pass on inputs that reach nothing."""
import functools

import numpy as np

F = np.float32
RG = 32                                                                 # side of k_lk_track's LDS neighbourhood
DEFAULT = dict(win=11, max_level=3, max_iters=30, eps=0.01, min_eig_threshold=1e-4)


def margin(win):
    """how far (in whole pixels, per axis) a window may move inside one level before k_lk_track copies its neighbourhood again"""
    return (RG - (win + 1)) // 2


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def levels(rows, cols, win, max_level):
    """buildOpticalFlowPyramid's rule: halve, rounding up, until max_level or a side not larger than the window -> (rows, cols) lists"""
    r, c = [rows], [cols]
    while len(r) <= max_level and (r[-1] + 1) // 2 > win and (c[-1] + 1) // 2 > win:
        r.append((r[-1] + 1) // 2); c.append((c[-1] + 1) // 2)
    return r, c


# ------------------------------------------------------------------------------------------------------ A: pyramid geometry
# name -> (rows, cols, win, max_level, level rows, level cols, k_lk_pyramid builds a 1-job call)
GEOMETRY = {
    "fused_limit_w11": (105, 112, 11, 3, [105, 53, 27, 14], [112, 56, 28, 14], True),       # top side = border + 2
    "first_unfused_w11": (104, 112, 11, 3, [104, 52, 26, 13], [112, 56, 28, 14], False),
    "double_fold_w11": (96, 128, 11, 3, [96, 48, 24, 12], [128, 64, 32, 16], False),        # 12 = win + 1 = the border
    "fused_limit_w15": (144, 150, 15, 3, [144, 72, 36, 18], [150, 75, 38, 19], True),
    "double_fold_w15": (128, 150, 15, 3, [128, 64, 32, 16], [150, 75, 38, 19], False),
    "fused_limit_w3": (48, 41, 3, 3, [48, 24, 12, 6], [41, 21, 11, 6], True),
    "double_fold_w3": (32, 41, 3, 3, [32, 16, 8, 4], [41, 21, 11, 6], False),
    "below_window_2x2": (2, 2, 11, 3, [2], [2], False),
    "below_window_3x17": (3, 17, 15, 3, [3], [17], False),
    "below_window_12x13": (12, 13, 11, 3, [12], [13], False),
    # (5, 40) at window 3 was asked for as a below_window case, but its side of 5 is above the border of 4 and folds once: it stays as
    # single_level_5x40, and below_window_3x40 -- a side the size of the window, two folds -- takes the place the name stands for
    "below_window_3x40": (3, 40, 3, 3, [3], [40], False),
    "single_level_5x40": (5, 40, 3, 3, [5], [40], False),
    "eight_levels": (700, 800, 5, 7, [700, 350, 175, 88, 44, 22, 11, 6], [800, 400, 200, 100, 50, 25, 13, 7], False),
}
WIDE = 17                                                               # jobs of a call that k_lk_pyramid never builds


def _noisy_roll(rng, a):
    return np.clip(np.roll(a, (1, 2), (0, 1)).astype(np.int16) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    """random texture; `next` and `third` are the image before them rolled by (1, 2) plus noise of +-2; points on a grid that reaches
    into the corners, the four corner pixels and two points just outside.  `others`: the frames of the 16 further jobs of the wide
    call, rolled copies."""
    rows, cols, win, max_level, lrows, lcols, fused = GEOMETRY[name]
    rng = np.random.default_rng(rows * 1000 + cols + win)
    prev = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    nxt = _noisy_roll(rng, prev)
    third = _noisy_roll(rng, nxt)
    gx, gy = np.meshgrid(np.linspace(0.5, cols - 1.5, 12), np.linspace(0.5, rows - 1.5, 9))
    pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(F)
    pts = np.concatenate([pts, np.array([[0, 0], [cols - 1, rows - 1], [cols - 1, 0], [0, rows - 1], [-3.5, 4.0], [cols + 2.0, rows / 2]], F)])
    others = [tuple(frozen(np.roll(f, (k, 2 * k), (0, 1))) for f in (prev, nxt, third)) for k in range(1, WIDE)]
    return dict(rows=rows, cols=cols, win=win, max_level=max_level, level_rows=lrows, level_cols=lcols, fused=fused,
                frames=(frozen(prev), frozen(nxt), frozen(third)), pts=frozen(pts), others=others)


# ------------------------------------------------------------------------------------------------------ B: steps beyond the margin
SMOOTH_ROWS, SMOOTH_COLS = 120, 160


@functools.lru_cache(maxsize=None)
def smooth(sigma=12.0, seed=3, rows=SMOOTH_ROWS, cols=SMOOTH_COLS):
    """white noise under a separable Gaussian of `sigma` (periodic, so that a roll is a translation everywhere), stretched to 0..255"""
    a = np.random.default_rng(seed).standard_normal((rows, cols))
    r = int(3 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = np.stack([np.convolve(np.pad(row, r, mode="wrap"), k, mode="valid") for row in a])
    a = np.stack([np.convolve(np.pad(col, r, mode="wrap"), k, mode="valid") for col in a.T]).T
    a = (a - a.min()) / (a.max() - a.min())
    return frozen(np.rint(a * 255.0).astype(np.uint8))


def step_points():
    gx, gy = np.meshgrid(np.linspace(40, 120, 9), np.linspace(40, 80, 5))
    return frozen(np.stack([gx.ravel(), gy.ravel()], 1).astype(F))


# name -> (win, shift in rows, shift in columns): next = np.roll(prev, (dy, dx), (0, 1)), so a point moves by (dx, dy).
# The diagonal cases move by (s, -s) in (rows, columns); shifts per window are margin + 1, + 3 and + 6.
def _steps():
    c = {}
    for win in (3, 5, 11, 15):
        for extra in (1, 3, 6):
            s = margin(win) + extra
            c["step_w%d_s%d" % (win, s)] = (win, s, -s)
    c["step_w11_y_only"] = (11, margin(11) + 3, 0)
    c["step_w11_opposite"] = (11, -(margin(11) + 3), margin(11) + 3)
    return c


STEPS = _steps()
# Window 3 sees too little of a sigma-12 image to follow 15 .. 20 pixels (the oracle keeps 8 - 11 of 45 points): its image is filtered
# with sigma 8, where it keeps 18 - 20.  The seeds are those, of 1 .. 12, with the most points to spare over the 15 the CPU test asks for.
STEP_IMAGE = {3: dict(sigma=8.0, seed=11), 5: dict(sigma=12.0, seed=7), 11: dict(sigma=12.0, seed=7), 15: dict(sigma=12.0, seed=7)}


@functools.lru_cache(maxsize=None)
def step_case(name):
    win, dy, dx = STEPS[name]
    prev = smooth(**STEP_IMAGE[win])
    return dict(win=win, max_level=0, shift=(dx, dy), frames=(prev, frozen(np.roll(prev, (dy, dx), (0, 1)))), pts=step_points())


# ------------------------------------------------------------------------------------------------------ C: the iteration limits
MAX_COUNTS = (0, 1, 2, 100, 1000, -5)
EPSILONS = (-1.0, 0.0, 10.0, 1e9)
CLAMPED_COUNT = {1000: 100, -5: 0}                                      # TermCriteria: maxCount to [0, 100], epsilon to [0, 10]
CLAMPED_EPS = {-1.0: 0.0, 1e9: 10.0}


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """"step": family B's window 11 moved by margin + 3 in one level, no guess.  "blobs": the blob texture of tests/test_lk_gpu.py
    rolled by (2, -6) with noise of +-3, four levels, the previous positions as the guess."""
    if name == "step":
        c = step_case("step_w11_s13")
        return dict(win=c["win"], max_level=0, frames=c["frames"], pts=c["pts"], guess=None)
    from tools.synth import make_stereo_pair
    prev = make_stereo_pair(seed=5, h=120, w=160, n_blobs=120)[0]
    rng = np.random.default_rng(9)
    nxt = np.clip(np.roll(prev, (2, -6), (0, 1)).astype(np.int16) + rng.integers(-3, 4, prev.shape), 0, 255).astype(np.uint8)
    gx, gy = np.meshgrid(np.linspace(12, 148, 9), np.linspace(12, 108, 5))
    pts = frozen(np.stack([gx.ravel(), gy.ravel()], 1).astype(F) + F(0.25))
    return dict(win=11, max_level=3, frames=(frozen(prev), frozen(nxt)), pts=pts, guess=pts)


LIMITS = ("step", "blobs")


# ------------------------------------------------------------------------------------------------------ D: degenerate texture
TEX_ROWS, TEX_COLS = 96, 128                                            # (the 12-row top level of double_fold_w11)
MIN_EIGS = (0.0, 1e-4, 1.0, 100.0)


def _textures():
    y, x = np.mgrid[0:TEX_ROWS, 0:TEX_COLS]
    return {
        "flat_90": np.full((TEX_ROWS, TEX_COLS), 90),
        "saturated": np.full((TEX_ROWS, TEX_COLS), 255),
        "stripes_v16": ((x // 8) % 2) * 255,
        "stripes_h16": ((y // 8) % 2) * 255,
        "stripes_diag": (((x + y) // 6) % 2) * 255,
        "checker_1": ((x + y) % 2) * 255,
        "checker_8": ((x // 8 + y // 8) % 2) * 255,
        "ramp_h": np.minimum(2 * x, 255),
    }


TEXTURES = tuple(_textures())


def texture_points():
    """7 x 5 points, 10 pixels inside the image: the grid at which the oracle keeps 15 / 30 / 35 / 0 points of the 8-pixel checkerboard at
    the four thresholds (a grid 16 pixels inside keeps 20 / 35 / 35 / 0: the counts belong to the positions)"""
    gx, gy = np.meshgrid(np.linspace(10, TEX_COLS - 10, 7), np.linspace(10, TEX_ROWS - 10, 5))
    return frozen(np.stack([gx.ravel(), gy.ravel()], 1).astype(F))


@functools.lru_cache(maxsize=None)
def texture_case(name):
    prev = _textures()[name].astype(np.uint8)
    return dict(frames=(frozen(prev), frozen(np.roll(prev, (1, 2), (0, 1)))), pts=texture_points())


# ------------------------------------------------------------------------------------------------------ G: coordinates
def bad_values(rows, cols):
    """-> float32 [k, 2]: every bad value as x beside an ordinary y, as y beside an ordinary x, and as both; the last sub-pixel of the
    image as a pair"""
    v = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 2147483648.0, -2147483904.0, 1e-40]
    out = []
    for b in v:
        out += [(b, 40.0), (50.0, b), (b, b)]
    out.append((cols - 1 + 0.999, rows - 1 + 0.999))
    with np.errstate(over="ignore"):
        return np.array(out, np.float64).astype(F)


@functools.lru_cache(maxsize=None)
def coordinate_case():
    """blob texture rolled by (1, 2); 12 ordinary points, then the bad ones.  -> frames, `good` [12, 2], `bad` [31, 2]"""
    from tools.synth import make_stereo_pair
    prev = make_stereo_pair(seed=5, h=120, w=160, n_blobs=120)[0]
    gx, gy = np.meshgrid(np.linspace(20, 140, 4), np.linspace(20, 100, 3))
    good = np.stack([gx.ravel(), gy.ravel()], 1).astype(F) + F(0.5)
    return dict(frames=(frozen(prev), frozen(np.roll(prev, (1, 2), (0, 1)))), good=frozen(good), bad=frozen(bad_values(*prev.shape)))
