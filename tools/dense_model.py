"""The contract of dense stereo, in plain numpy and integers only (the style of tools/undistort_model.py): what ssx_stereo_dense
(csrc/dense.hip) writes for a rectified pair.  cv::StereoSGBM cannot be pinned here, so the contract is the project's own: a 9 x 7
census, Hamming cost, semi-global matching over 4 or 8 paths, a left disparity with uniqueness and left-right checks and an integer
sub-pixel step.  Every value is a small integer, so the device is held to it with array_equal.

Inputs: left, right uint8 [rows, cols].  Parameters (DenseParams): D = disparities (64 or 128 through the ABI; the model takes any
D >= 2 for hand-evaluated toys), 1 <= P1 <= P2 <= 192, uniqueness 0..99 (percent), lr_tolerance (whole disparities, -1 = off),
paths 4 or 8.  The minimum disparity is 0.

1. census(img): uint64 per pixel.  Window 9 wide, 7 high, neighbour coordinates clamped to the image (replicated border); the 62
   neighbours in raster order, top-left first, skipping the centre; each shifts the word left and ORs in (neighbour < centre).
2. C(y, x, d) = popcount(censusL(y, x) ^ censusR(y, x - d)), 0..62; the constant 63 where x - d < 0.
3. Directions (dx, dy) in the order DIRECTIONS; paths = 4 takes the first four.  A path starts at every pixel whose predecessor
   (x - dx, y - dy) lies outside the image: L(p, d) = C(p, d).  Otherwise, with m = min_k L(p - r, k),
       L(p, d) = C(p, d) + min(L(p-r, d), L(p-r, d-1) + P1, L(p-r, d+1) + P1, m + P2) - m
   (the d-1 term absent at d = 0, the d+1 term at d = D-1).  L <= 63 + P2 <= 255: a byte.  S = the sum of L over the paths, uint16.
4. d0 = the FIRST minimum of S(y, x, .), s0 its value.  The pixel is valid iff 1 <= d0 <= D-2, d0 <= x, no d' with |d' - d0| > 1 has
   S(d') * (100 - uniqueness) < s0 * 100, and step 5 passes.  den = max(S(d0-1) + S(d0+1) - 2 s0, 1),
   sub = floor(((S(d0-1) - S(d0+1)) * 16 + den) / (2 den)), disp = 16 d0 + sub: int16 in 1/16 pixel, -16 where invalid.
5. dR(y, xr) = the first minimum over d of S(y, xr + d, d), candidates with xr + d >= cols excluded.  A left pixel passes iff
   |dR(y, x - d0) - d0| <= lr_tolerance.

Deviations from cv::StereoSGBM: census cost in place of Birchfield-Tomasi on Sobel-filtered images; no pre-filter cap; no
disparity margin (the clamped census and the constant 63 give every pixel a cost); the right disparity from the same volume with
the first-minimum rule; no speckle filter; sub-pixel by floor division, not by rounding to nearest of a float.
"""
from dataclasses import dataclass

import numpy as np

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))
INVALID = -16
CENSUS_W, CENSUS_H = 9, 7
COST_OUTSIDE = 63


@dataclass
class DenseParams:
    disparities: int = 128
    p1: int = 7
    p2: int = 86
    uniqueness: int = 10
    lr_tolerance: int = 1
    paths: int = 8

    def check(self):
        assert self.disparities >= 2
        assert 1 <= self.p1 <= self.p2 <= 192, "1 <= P1 <= P2 <= 192: a path value 63 + P2 must fit a byte"
        assert 0 <= self.uniqueness <= 99
        assert self.lr_tolerance >= -1
        assert self.paths in (4, 8)


def census(img):
    """-> uint64 [rows, cols]"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    rows, cols = img.shape
    ry, rx = CENSUS_H // 2, CENSUS_W // 2
    pad = np.pad(img, ((ry, ry), (rx, rx)), mode="edge")
    word = np.zeros((rows, cols), dtype=np.uint64)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dx == 0 and dy == 0:
                continue
            nb = pad[ry + dy:ry + dy + rows, rx + dx:rx + dx + cols]
            word = (word << np.uint64(1)) | (nb < img).astype(np.uint64)
    return word


def _popcount64(v):
    v = v.copy()
    n = np.zeros(v.shape, dtype=np.uint8)
    for _ in range(8):
        n += _POP8[(v & np.uint64(0xFF)).astype(np.intp)]
        v >>= np.uint64(8)
    return n


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def cost_volume(cl, cr, D):
    """-> uint8 [rows, cols, D]"""
    rows, cols = cl.shape
    C = np.full((rows, cols, D), COST_OUTSIDE, dtype=np.uint8)
    for d in range(min(D, cols)):
        C[:, d:, d] = _popcount64(cl[:, d:] ^ cr[:, :cols - d])
    return C


def _step(C, prev, p1, p2):
    """one step of the recurrence over a batch of pixels: C, prev int32 [n, D] -> L [n, D]"""
    big = np.int32(1 << 20)
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, big)
    lo[:, 1:] = prev[:, :-1] + p1
    hi = np.full_like(prev, big)
    hi[:, :-1] = prev[:, 1:] + p1
    return C + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + p2)) - m


def path_volume_from_cost(C, direction, p1, p2):
    """L of one direction (index into DIRECTIONS, or a (dx, dy) pair) -> uint8 [rows, cols, D]"""
    dx, dy = DIRECTIONS[direction] if isinstance(direction, (int, np.integer)) else direction
    rows, cols, D = C.shape
    Ci = C.astype(np.int32)
    L = np.zeros((rows, cols, D), dtype=np.int32)
    if dy == 0:
        xs = range(cols) if dx > 0 else range(cols - 1, -1, -1)
        for k, x in enumerate(xs):
            L[:, x] = Ci[:, x] if k == 0 else _step(Ci[:, x], L[:, x - dx], p1, p2)
    else:
        ys = range(rows) if dy > 0 else range(rows - 1, -1, -1)
        for k, y in enumerate(ys):
            if k == 0:
                L[y] = Ci[y]
                continue
            x = np.arange(cols)
            inside = (x - dx >= 0) & (x - dx < cols)
            L[y, ~inside] = Ci[y, ~inside]
            xi = x[inside]
            L[y, xi] = _step(Ci[y, xi], L[y - dy, xi - dx], p1, p2)
    assert L.min() >= 0 and L.max() <= COST_OUTSIDE + p2 <= 255, "a path value must fit a byte: L <= 63 + P2 <= 255"
    return L.astype(np.uint8)


def path_volume(left, right, direction, prm=None):
    prm = prm or DenseParams()
    prm.check()
    C = cost_volume(census(left), census(right), prm.disparities)
    return path_volume_from_cost(C, direction, prm.p1, prm.p2)


def sum_volume_from_cost(C, prm):
    S = np.zeros(C.shape, dtype=np.uint16)
    for k in range(prm.paths):
        S += path_volume_from_cost(C, k, prm.p1, prm.p2)
    return S


def sum_volume(left, right, prm=None):
    prm = prm or DenseParams()
    prm.check()
    return sum_volume_from_cost(cost_volume(census(left), census(right), prm.disparities), prm)


def right_disparity_from_sum(S):
    """dR -> uint8 [rows, cols]"""
    rows, cols, D = S.shape
    SR = np.full((rows, cols, D), 0xFFFF, dtype=np.uint16)
    for d in range(min(D, cols)):
        SR[:, :cols - d, d] = S[:, d:, d]
    return SR.argmin(axis=2).astype(np.uint8)       # argmin: the first minimum


def right_disparity(left, right, prm=None):
    return right_disparity_from_sum(sum_volume(left, right, prm))


def floor_div(num, den):
    """floor(num / den) for den > 0: Python's //, not C's truncation"""
    return num // den


def disparity_from_sum(S, prm):
    """-> int16 [rows, cols], 1/16 pixel, INVALID where a check fails"""
    rows, cols, D = S.shape
    Si = S.astype(np.int64)
    d0 = Si.argmin(axis=2)
    s0 = np.take_along_axis(Si, d0[..., None], axis=2)[..., 0]
    x = np.arange(cols)[None, :]
    valid = (d0 >= 1) & (d0 <= D - 2) & (d0 <= x)
    dd = np.arange(D)[None, None, :]
    far = np.abs(dd - d0[..., None]) > 1
    rival = far & (Si * (100 - prm.uniqueness) < s0[..., None] * 100)
    valid &= ~rival.any(axis=2)
    if prm.lr_tolerance >= 0:
        dR = right_disparity_from_sum(S).astype(np.int64)
        xr = np.clip(x - d0, 0, cols - 1)
        y = np.arange(rows)[:, None]
        valid &= np.abs(dR[y, xr] - d0) <= prm.lr_tolerance
    dm = np.clip(d0 - 1, 0, D - 1)[..., None]
    dp = np.clip(d0 + 1, 0, D - 1)[..., None]
    sm = np.take_along_axis(Si, dm, axis=2)[..., 0]
    sp = np.take_along_axis(Si, dp, axis=2)[..., 0]
    den = np.maximum(sm + sp - 2 * s0, 1)
    sub = floor_div((sm - sp) * 16 + den, 2 * den)
    disp = 16 * d0 + sub
    return np.where(valid, disp, INVALID).astype(np.int16)


def disparity(left, right, prm=None):
    """the contract: left, right uint8 [rows, cols] -> int16 [rows, cols]"""
    prm = prm or DenseParams()
    prm.check()
    left = np.ascontiguousarray(left, dtype=np.uint8)
    right = np.ascontiguousarray(right, dtype=np.uint8)
    assert left.shape == right.shape and left.ndim == 2
    return disparity_from_sum(sum_volume(left, right, prm), prm)


def cloud_samples(disp, left, stride, bf, max_depth):
    """the samples a keyframe keeps: every stride-th pixel of every stride-th row that is valid and within max_depth (z = bf * 16 /
    disp16 <= max_depth, f64) -> int array [n, 4]: u, v, disp16, intensity"""
    out = []
    rows, cols = disp.shape
    for v in range(0, rows, stride):
        for u in range(0, cols, stride):
            d = int(disp[v, u])
            if d > 0 and np.float64(bf) * 16.0 / np.float64(d) <= np.float64(max_depth):
                out.append((u, v, d, int(left[v, u])))
    return np.array(out, dtype=np.int64).reshape(-1, 4)
