"""Made disparity maps for the speckle filter's tests: each is built to break one way a labelling can go wrong.  Shared by the model's
CPU test (against a flood fill) and the device's GPU test (against the model).

made_maps(rows, cols) -> {name: (map int16 [rows, cols], speckle_range, [speckle sizes to filter at])}"""
import numpy as np

INVALID = -16
RANGE = 16
BLOB = 50                                                          # the speckle size of the "blobs" case


def _box_blob(m, y0, x0, n, value):
    """n pixels in raster order inside a box 8 wide whose corner is (y0, x0)"""
    for k in range(n):
        m[y0 + k // 8, x0 + k % 8] = value


def made_maps(rows, cols):
    pix = rows * cols
    out = {}
    out["constant"] = (np.full((rows, cols), 160, dtype=np.int16), RANGE, [pix - 1, pix])
    yy, xx = np.mgrid[0:rows, 0:cols]
    out["checkerboard"] = (np.where((yy + xx) % 2 == 0, 160, INVALID).astype(np.int16), RANGE, [1])
    # a one-pixel-wide serpentine through the whole map: full even rows, joined at alternating ends by one pixel of the odd rows
    m = np.full((rows, cols), INVALID, dtype=np.int16)
    m[0::2] = 200
    for y in range(1, rows, 2):
        m[y, cols - 1 if (y // 2) % 2 == 0 else 0] = 200
    out["serpentine"] = (m, RANGE, [int((m > 0).sum()) - 1, int((m > 0).sum())])
    # a comb whose teeth join only in the last row
    m = np.full((rows, cols), INVALID, dtype=np.int16)
    m[:, 0::2] = 300
    m[rows - 1] = 300
    out["comb"] = (m, RANGE, [int((m > 0).sum()) - 1, rows])
    # ramps along a row: steps of exactly the range are one component, steps of range + 1 cut every column off
    out["ramp_at_range"] = ((100 + RANGE * xx).astype(np.int16), RANGE, [pix - 1, pix])
    out["ramp_past_range"] = ((100 + (RANGE + 1) * xx).astype(np.int16), RANGE, [rows - 1, rows])
    # the last pixel of a row and the first of the next are equal and all else is invalid: no wrap
    m = np.full((rows, cols), INVALID, dtype=np.int16)
    m[rows // 2, cols - 1] = 160
    m[rows // 2 + 1, 0] = 160
    out["no_wrap"] = (m, RANGE, [1])
    # blobs of s - 1, s and s + 1 pixels at speckle_size = s, across a tile border where the map is wide enough
    m = np.full((rows, cols), INVALID, dtype=np.int16)
    for n, x0 in zip((BLOB - 1, BLOB, BLOB + 1), (4, 20, 60 if cols >= 72 else cols - 12)):
        _box_blob(m, 12, x0, n, 160)
    out["blobs"] = (m, RANGE, [BLOB])
    # what is not valid next to the largest value, at the largest range: the differences need 32-bit arithmetic
    m = np.full((rows, cols), INVALID, dtype=np.int16)
    m[20, 10:18] = [32767, 0, 32767, -1, 32767, -32768, 32767, 32767]
    m[21, 11] = 32767                                              # below the 0: joined to nothing
    out["extremes"] = (m, 32767, [1, 2])
    rng = np.random.default_rng(rows * 1000 + cols)
    m = rng.choice(np.array([100, 110, 130, 160], dtype=np.int16), size=(rows, cols))
    m[rng.random((rows, cols)) >= 0.6] = INVALID
    out["random"] = (m, RANGE, [3, 20])
    for v in out.values():
        v[0].setflags(write=False)
    return out


def seam_maps(rows, cols):
    """three jobs whose facing rows are equal and valid, all else invalid: a labelling that runs over a seam joins them"""
    maps = [np.full((rows, cols), INVALID, dtype=np.int16) for _ in range(3)]
    maps[0][rows - 1] = 160
    maps[1][0] = 160
    maps[1][rows - 1] = 160
    maps[2][0] = 160
    return maps
