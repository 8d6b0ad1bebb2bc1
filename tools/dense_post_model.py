"""The contract of what follows a dense disparity map, in plain numpy / Python and integers only (the style of tools/dense_model.py,
which it leaves alone): the speckle filter and the samples a keyframe keeps, as ssx_dense_postprocess and ssx_stereo_dense_post
(csrc/dense_post.inc) write them.  The device is held to it with array_equal.

Input: disp int16 [rows, cols] in 1/16 pixel, as tools/dense_model.py's disparity() writes it.

Validity.  A pixel is valid iff its value is > 0 (the rule of the host's SampleDense).  -16, 0, -1 and -32768 are all "not valid": they
are never rewritten and never joined to anything.

components(disp, speckle_range) -> (size, root), int32 [rows, cols].  Two 4-neighbours are joined iff both are valid and
|a - b| <= speckle_range (1/16 pixel, int32 arithmetic; the difference between the two NEIGHBOURS, not against a seed, so a ramp whose
steps are within the range is one component).  Row ends do not wrap.  Components are the connected components of that graph; size is the
pixel count of the pixel's component and root the smallest raster index y * cols + x in it; 0 and -1 where the pixel is not valid.  The
partition is unique, so both arrays are independent of any order of evaluation: the device may use atomics and still be compared bit for
bit.

filter_speckles(disp, speckle_size, speckle_range) -> int16 map: every valid pixel whose component has size <= speckle_size becomes
INVALID (-16), everything else is unchanged; speckle_size = 0 returns the map unchanged.  This is the rule of cv::filterSpeckles with
newVal = -16 (maxSpeckleSize = speckle_size, maxDiff = speckle_range); OpenCV is not the oracle, this file is.

min_disp16(bf, max_depth): the smallest d in 1 .. 32767 with f64(bf) * 16.0 / f64(d) <= f64(max_depth), or 32768 if there is none.  A
correctly rounded division is monotone in d, so the depth bar of dense_model.cloud_samples is exactly disp16 >= min_disp16(bf, max_depth):
the device needs one integer and no floating point.

samples(disp, left, stride, min_d16): every stride-th pixel of every stride-th row with disp >= max(min_d16, 1), in raster order, as
[n, 4] = u, v, disp16, intensity -- dense_model.cloud_samples(disp, left, stride, bf, max_depth) whenever min_d16 = min_disp16(bf,
max_depth).

postprocess(disp, left, post): the filter, then the samples of the filtered map.
"""
from dataclasses import dataclass

import numpy as np

INVALID = -16


@dataclass
class DensePost:
    speckle_size: int = 0        # 0 = no filter
    speckle_range: int = 16      # 1/16 pixel
    cloud_stride: int = 0        # 0 = no samples
    cloud_min_disp16: int = 1

    def check(self, rows, cols):
        assert 0 <= self.speckle_size <= rows * cols
        assert 0 <= self.speckle_range <= 32767
        assert self.cloud_stride == 0 or 1 <= self.cloud_stride <= 4000
        assert 1 <= self.cloud_min_disp16 <= 32768


def _find(parent, i):
    r = i
    while parent[r] != r:
        r = parent[r]
    while parent[i] != r:                                         # path compression
        parent[i], i = r, parent[i]
    return r


def components(disp, speckle_range):
    """-> (size, root) int32 [rows, cols]"""
    disp = np.asarray(disp)
    assert disp.dtype == np.int16 and disp.ndim == 2
    rows, cols = disp.shape
    d = disp.astype(np.int32)
    valid = d > 0
    rng = int(speckle_range)
    right = valid[:, 1:] & valid[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= rng)      # (y, x) -- (y, x + 1)
    down = valid[1:] & valid[:-1] & (np.abs(d[1:] - d[:-1]) <= rng)                   # (y, x) -- (y + 1, x)
    parent = list(range(rows * cols))

    def union(a, b):
        a, b = _find(parent, a), _find(parent, b)
        if a != b:
            parent[max(a, b)] = min(a, b)                         # the root is the smallest raster index

    for y, x in zip(*np.nonzero(right)):
        union(int(y) * cols + int(x), int(y) * cols + int(x) + 1)
    for y, x in zip(*np.nonzero(down)):
        union(int(y) * cols + int(x), (int(y) + 1) * cols + int(x))
    root = np.array([_find(parent, i) for i in range(rows * cols)], dtype=np.int32).reshape(rows, cols)
    count = np.bincount(root.ravel()[valid.ravel()], minlength=rows * cols).astype(np.int32)
    size = np.where(valid, count[root], 0).astype(np.int32)
    root = np.where(valid, root, -1).astype(np.int32)
    return size, root


def filter_speckles(disp, speckle_size, speckle_range):
    """cv::filterSpeckles' rule with newVal = -16 -> int16 map"""
    disp = np.asarray(disp)
    if int(speckle_size) == 0:
        return disp.copy()
    size, _ = components(disp, speckle_range)
    return np.where((disp > 0) & (size <= int(speckle_size)), np.int16(INVALID), disp).astype(np.int16)


def min_disp16(bf, max_depth):
    lo, hi = 1, 32768                                             # the predicate is monotone in d: bisect for the first d that passes
    ok = lambda d: np.float64(bf) * 16.0 / np.float64(d) <= np.float64(max_depth)
    while lo < hi:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def samples(disp, left, stride, min_d16):
    """-> int64 [n, 4]: u, v, disp16, intensity, in raster order"""
    disp = np.asarray(disp)
    bar = max(int(min_d16), 1)
    sub = disp[::stride, ::stride].astype(np.int64)
    v, u = np.nonzero(sub >= bar)                                 # nonzero walks in raster order
    v, u = v * stride, u * stride
    return np.stack([u, v, disp[v, u].astype(np.int64), np.asarray(left)[v, u].astype(np.int64)], axis=1).astype(np.int64).reshape(-1, 4)


def postprocess(disp, left, post):
    """-> (filtered map, samples or None)"""
    disp = np.asarray(disp)
    post.check(*disp.shape)
    out = filter_speckles(disp, post.speckle_size, post.speckle_range)
    return out, (samples(out, left, post.cloud_stride, post.cloud_min_disp16) if post.cloud_stride > 0 else None)
