"""The inputs of tests/test_orb_image_cases.py (CPU) and tests/test_orb_images_gpu.py (GPU): named images for the ORB front-end
(ssvio_amd/csrc/orb.hip), built deterministically with plain numpy.

tools.synth.make_stereo_pair draws smooth blobs in mid-range grey into a C-contiguous array.  The images here are what it never
gives: pixels at 0 and 255 (the saturating u16 arithmetic of the quick test, the score ceiling 254 and the dropped score 0), equal
scores next to each other (the strict '>' of the NMS), cells whose only corner is masked (emptiness is judged before the mask),
symmetric and periodic patches (m10 == m01 == 0, t0 == t1), noise at widths around the blur tile's 128 columns, levels of a few
pixels, masks that hold 1 and 128, rows that lie pitched and unaligned in a buffer that ends with the image's last byte, and
keypoints given on the edge of ScreenAndComputeKPsParams' screen and on halves.

A case is a dict: `img` (2-D uint8), `mask` (None or 2-D uint8, possibly a strided view), `prm` (the ORB parameters, oracle names),
`kind` ("extract": the whole pipeline; "pitched" / "batch": views of a buffer against their contiguous copies; "describe": given
keypoints) and `claims`, the facts the case says it reaches -- names of the counts tests/test_orb_image_cases.py derives from the
oracle (`reach` there), each of which must then be above zero.  Nothing here exceeds a capacity of the kernels and nothing reads
outside an image; tests/test_orb_image_cases.py asserts both.

The grid of ORBextractor::Detect / ComputeKeyPointsOctTree (make_cells of orb.hip) is written down a second time in `cells`, with
the ROI of every cell; the CPU test holds its cell counts against ssx_orb_debug_plan."""
import functools

import numpy as np

F = np.float32
CELL_CAP, CAND_CAP, SEL_CAP, EDGE, BORDER = 256, 16384, 4096, 19, 16     # orb_ws.hpp; BORDER = EDGE_THRESHOLD - 3
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DEFAULT = dict(nfeatures=500, scale_factor=1.2, nlevels=4, ini_th=20, min_th=7)
H, W = 120, 160


def cells(rows, cols):
    """make_cells (orb.hip): -> int array [cells, 6], per cell the ROI x0, y0, w, h in the level and the offset ox, oy its local
    coordinates take in the candidate records (relative to the 16-px border)"""
    out = []
    max_x, max_y = cols - BORDER, rows - BORDER
    width, height = F(max_x - BORDER), F(max_y - BORDER)
    n_cols, n_rows = int(width / F(30)), int(height / F(30))
    if n_cols < 1 or n_rows < 1:
        return np.zeros((0, 6), np.int64)
    w_cell, h_cell = int(np.ceil(width / F(n_cols))), int(np.ceil(height / F(n_rows)))
    for i in range(n_rows):
        ini_y = BORDER + i * h_cell
        if ini_y >= max_y - 3:
            continue
        h = min(ini_y + h_cell + 6, max_y) - ini_y
        for j in range(n_cols):
            ini_x = BORDER + j * w_cell
            if ini_x >= max_x - 6:
                continue
            w = min(ini_x + w_cell + 6, max_x) - ini_x
            out.append((ini_x, ini_y, w, h, j * w_cell, i * h_cell))
    return np.array(out, np.int64).reshape(-1, 6)


# ---------------------------------------------------------------------------------------------------------------- images
def noise(rows=H, cols=W, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.uint8)


def binary_noise(rows=H, cols=W, seed=2):
    return (np.random.default_rng(seed).integers(0, 2, (rows, cols)) * 255).astype(np.uint8)


def dots(period, rows=H, cols=W, fg=255, bg=0):
    a = np.full((rows, cols), bg, np.uint8)
    a[period // 2::period, period // 2::period] = fg
    return a


def checker(period, rows=H, cols=W):
    y, x = np.mgrid[0:rows, 0:cols]
    return (((y // period + x // period) & 1) * 255).astype(np.uint8)


def ramp(rows=H, cols=W):
    return np.tile(np.linspace(0, 255, cols).astype(np.uint8), (rows, 1))


def saturated_blobs(rows=H, cols=W, seed=3):
    """Gaussian blobs of both signs around mid grey, scaled by 6 and clipped: wide areas at 0 and at 255; the transitions between
    them carry +-24 of noise, so that corners sit on pixels within a threshold of either end of the range"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    f = np.zeros((rows, cols))
    for _ in range(60):
        cx, cy, s, a = rng.uniform(0, cols), rng.uniform(0, rows), rng.uniform(2.0, 7.0), rng.choice([-1.0, 1.0]) * rng.uniform(20, 60)
        f += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    f = 127.5 + 6.0 * f + rng.integers(-24, 25, (rows, cols))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def one_corner_per_cell(rows=H, cols=W, masked=False, domino=False):
    """black, with one 255 pixel in the middle of every level-0 cell (an isolated pixel is a corner of score 254 and the only one
    around it) and, 8 px to its right, one pixel of 12: a corner at minThFAST 7 and none at iniThFAST 20.  The cell finds the first at
    iniThFAST, so the second never shows.  masked: the mask is 0 on every 255 pixel -- at the coordinates the reference looks the mask
    up at, which are relative to the 16-px border -- and 255 elsewhere.  The reference judges a cell empty BEFORE the mask, so the
    cell is not run again at minThFAST: it yields nothing, the pixel of 12 included.
    domino: the 255 pixel has a second one right of it.  Neither is on the other's ring, so both are corners of score 254, and under
    the strict '>' both die: NMS leaves the cell nothing, it IS run again at minThFAST, and there the pixel of 12 is its one
    candidate (score 11)."""
    img = np.zeros((rows, cols), np.uint8)
    mask = np.full((rows, cols), 255, np.uint8)
    for x0, y0, w, h, ox, oy in cells(rows, cols):
        lx, ly = w // 2 - 4, h // 2
        img[y0 + ly, x0 + lx] = 255
        if domino:
            img[y0 + ly, x0 + lx + 1] = 255
        img[y0 + ly, x0 + lx + 8] = 12
        mask[oy + ly, ox + lx] = 0
    return img, (mask if masked else None)


def stripe_mask(rows, cols, vertical, width=5):
    """stripes of 0, 1, 128, 255, `width` px wide: narrower than a cell"""
    v = np.array([0, 1, 128, 255], np.uint8)[(np.arange(cols if vertical else rows) // width) % 4]
    return np.ascontiguousarray(np.tile(v, (rows, 1)) if vertical else np.tile(v[:, None], (1, cols)))


def pitched(a, stride, offset):
    """the rows of `a` as a view with row stride `stride` bytes, `offset` bytes into a buffer that ends with the last pixel of the
    last row; the bytes between the rows are 0xA5"""
    rows, cols = a.shape
    buf = np.full(offset + (rows - 1) * stride + cols, 0xA5, np.uint8)
    v = np.ndarray((rows, cols), np.uint8, buffer=buf, offset=offset, strides=(stride, 1))
    v[:] = a
    return v


# ---------------------------------------------------------------------------------------------------------------- the table
def _case(kind, img, mask=None, claims=(), **prm):
    assert not set(prm) - set(DEFAULT)
    return dict(kind=kind, img=img, mask=mask, prm={**DEFAULT, **prm}, claims=tuple(claims))


def _extract_cases():
    c = {}
    c["noise/uniform"] = _case("extract", noise(), claims=("sat_corners", "ties", "zero_desc_bytes"))
    c["noise/binary"] = _case("extract", binary_noise(), claims=("sat_corners", "resp254", "all_level0_254", "ties"))
    c["dots/p4"] = _case("extract", dots(4), claims=("sat_corners", "resp254", "all_level0_254", "axis_angles"))
    for name, img in (("checker/p1", checker(1)), ("checker/p4", checker(4)), ("checker/p7", checker(7)), ("dots/p2", dots(2))):
        c[name] = _case("extract", img, claims=("level0_empty", "keypoints"))
    c["ramp/h"] = _case("extract", ramp(), claims=("no_keypoints",))
    c["flat/0"] = _case("extract", np.zeros((H, W), np.uint8), claims=("no_keypoints",))
    c["flat/255"] = _case("extract", np.full((H, W), 255, np.uint8), claims=("no_keypoints",))
    c["blobs/saturated"] = _case("extract", saturated_blobs(), claims=("sat_corners", "keypoints", "px_at_0", "px_at_255"))
    img, _ = one_corner_per_cell()
    c["cell/one_corner"] = _case("extract", img, nlevels=2, claims=("one_per_cell", "resp254"))
    img, mask = one_corner_per_cell(masked=True)
    c["cell/one_corner_masked"] = _case("extract", img, mask, nlevels=2, claims=("masked_out_cells", "level0_no_candidates"))
    img, _ = one_corner_per_cell(domino=True)
    c["cell/all_tie"] = _case("extract", img, nlevels=2, claims=("ties", "all_cells_second_pass", "one_per_cell", "all_level0_11"))
    for ini, mn, claims in ((255, 0, ("second_pass_cells", "all_cells_second_pass")), (1, 1, ("keypoints", "ties")), (20, 0, ("keypoints",)),
                            (0, 0, ("keypoints", "ties"))):
        c["noise/th%d_%d" % (ini, mn)] = _case("extract", noise(), ini_th=ini, min_th=mn, claims=claims)
    c["mask/stripes_v"] = _case("extract", noise(), stripe_mask(H, W, True), claims=("mask_values", "masked_candidates", "keypoints"))
    c["mask/stripes_h"] = _case("extract", noise(), stripe_mask(H, W, False), claims=("mask_values", "masked_candidates", "keypoints"))
    c["mask/strided"] = _case("extract", noise(), pitched(stripe_mask(H, W, True, 7), W + 13, 3), claims=("mask_strided", "masked_candidates"))
    # blur and resize geometry on noise: widths around the blur tile's 128 columns (GT_W) and the second tile.  41 rows
    # hold no grid cell (every pixel of every level and blurred level is compared all the same); 62 rows hold one row of cells
    for cols in (124, 127, 128, 129, 131, 132, 133, 252, 256, 260):
        c["geom/41x%d" % cols] = _case("extract", noise(41, cols, seed=cols), claims=())
    c["geom/62x131"] = _case("extract", noise(62, 131, seed=5), claims=("keypoints",))
    # levels below 8 px in a dimension: the blur's byte-by-byte reflection, resize tables of a few entries
    c["small/40x160_s2.3"] = _case("extract", noise(40, 160, seed=6), scale_factor=2.3, claims=("small_levels",))
    c["small/160x40_s2.3"] = _case("extract", noise(160, 40, seed=7), scale_factor=2.3, claims=("small_levels",))
    c["small/41x41_s2.0"] = _case("extract", noise(41, 41, seed=8), scale_factor=2.0, nlevels=5, claims=("small_levels",))
    c["small/70x100_l8"] = _case("extract", noise(70, 100, seed=9), scale_factor=1.5, nlevels=7, claims=("small_levels", "keypoints"))
    # scale 2.3: quads of four destination columns span more than 8 source bytes, the byte-load branch of k_resize
    c["noise/scale2.3"] = _case("extract", noise(), scale_factor=2.3, claims=("keypoints",))
    c["binary/scale2.3"] = _case("extract", binary_noise(), scale_factor=2.3, nlevels=3, claims=("keypoints", "resp254"))
    return c


PITCH_ROWS = 72
STRIDES = ("cols+1", "cols+3", "cols+8", "2*cols")
OFFSETS = (0, 1, 3, 5)


def _stride(kind, cols):
    return dict(zip(STRIDES, (cols + 1, cols + 3, cols + 8, 2 * cols)))[kind]


def _pitched_cases():
    """16 views: every stride kind with every base offset, every residue of cols % 8 twice.  One noise field, cut to the width."""
    c = {}
    field = noise(PITCH_ROWS, 168, seed=11)
    for i in range(16):
        cols, kind, off = 160 + (i + i // 8) % 8, STRIDES[i % 4], OFFSETS[i // 4]
        a = np.ascontiguousarray(field[:, :cols])
        c["pitched/c%d_%s_o%d" % (cols, kind, off)] = dict(_case("pitched", pitched(a, _stride(kind, cols), off), nlevels=3, claims=("pitched",)), contiguous=a,
                                                           stride_kind=kind, offset=off)
    # one call, one pointer per image: four images of one stride (the batch takes one stride per call), each at another alignment
    for cols, kind in ((163, "cols+3"), (160, "cols+1")):
        imgs = [np.ascontiguousarray(noise(PITCH_ROWS, cols, seed=20 + k)) for k in range(4)]
        views = [pitched(a, _stride(kind, cols), off) for a, off in zip(imgs, OFFSETS)]
        c["batch/c%d_%s" % (cols, kind)] = dict(_case("batch", views[0], nlevels=1, claims=("pitched", "alignments")), views=views, contiguous=imgs)
    return c


def preimage(p, sc):
    """a float32 x with x / sc == p in float32 arithmetic (the kernel and the reference divide the given coordinate by the level's
    scale), or None when none of the floats around p * sc divides back to p; p = 18.999 only has to stay below 19"""
    p, sc = F(p), F(sc)
    x = F(p * sc)
    if p == F(18.999):
        return x if F(x / sc) < F(EDGE) else None
    for _ in range(4):
        x = np.nextafter(x, F(-np.inf))
    for _ in range(9):
        if F(x / sc) == p:
            return x
        x = np.nextafter(x, F(np.inf))
    return None


def level_scales(prm):
    s = [F(1)]
    for _ in range(1, prm["nlevels"]):
        s.append(F(s[-1] * F(prm["scale_factor"])))
    return s


def level_sizes(rows, cols, prm):
    """ComputePyramid's sizes (plan_levels of orb.hip): cvRound(size * (1 / scale))"""
    inv = [F(1) / s for s in level_scales(prm)]
    return [int(np.rint(F(rows) * i)) for i in inv], [int(np.rint(F(cols) * i)) for i in inv]


def describe_keypoints(rows, cols, prm):
    """keypoints at octaves 0 .. nlevels - 1, given at level-0 scale so that their position on the level is
      * the whole frame of the screen: x in {19, cols_l - 20} with every y, y in {19, rows_l - 20} with every x (kept where the
        pixel passes the FAST test), the same frame one pixel further out (x = cols_l - 19, y = rows_l - 19: dropped) and 18.999
        (dropped);
      * a 12 x 12 block of positions on .5 in both axes, even and odd integer parts (cvRound is half-to-even);
    and two octaves out of range.  Where no float divides back to the wanted position the keypoint is left out.
    -> (keypoints, wanted level positions [n, 2] as float32)"""
    lr, lc = level_sizes(rows, cols, prm)
    kps, want = [], []
    for l, sc in enumerate(level_scales(prm)):
        r, c = lr[l], lc[l]
        pos = []
        if r > 2 * EDGE and c > 2 * EDGE:
            for y in range(EDGE, r - EDGE):
                pos += [(EDGE, y), (c - EDGE - 1, y), (c - EDGE, y), (18.999, y)]
            for x in range(EDGE, c - EDGE):
                pos += [(x, EDGE), (x, r - EDGE - 1), (x, r - EDGE), (x, 18.999)]
            pos += [(x + 0.5, y + 0.5) for y in range(22, 34) for x in range(22, 34) if x + 1 < c - EDGE and y + 1 < r - EDGE]
        else:
            pos += [(r // 2, c // 2)]                       # a level too small for any keypoint: dropped
        for px, py in pos:
            x, y = preimage(px, sc), preimage(py, sc)
            if x is None or y is None:
                continue
            kps.append((x, y, l))
            want.append((px, py))
    kps += [(F(40), F(40), -1), (F(40), F(40), prm["nlevels"])]
    want += [(40, 40), (40, 40)]
    k = np.zeros(len(kps), KP_DTYPE)
    k["x"], k["y"], k["octave"] = [np.array(v) for v in zip(*kps)]
    k["size"], k["angle"], k["response"], k["class_id"] = 31.0, -1.0, -1.0, np.arange(len(k))
    return k, np.array(want, F)


def _describe_cases():
    c = {}
    for mn in (7, 0, 255):
        prm = {**DEFAULT, "min_th": mn}
        kps, want = describe_keypoints(H, W, prm)
        claims = ("desc_dropped_all",) if mn == 255 else ("at_19", "at_far_edge", "past_far_edge", "below_19", "half_even", "half_odd", "not_corner", "every_octave")
        c["describe/min_th%d" % mn] = dict(_case("describe", noise(), min_th=mn, claims=claims), kps=kps, want=want)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    return {**_extract_cases(), **_pitched_cases(), **_describe_cases()}


def names(kind):
    return [n for n, c in cases().items() if c["kind"] == kind]


# ---------------------------------------------------------------------------------------------------------------- FAST in numpy
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))


def fast9_numpy(img, t):
    """cv::FAST(img, t, nonmaxSuppression=true) stated plainly: a pixel 3 or more from every side is a corner at threshold t when 9
    contiguous pixels of its 16-pixel ring are all darker than v - t or all brighter than v + t; its score is the largest threshold at
    which it still is one (at most 254, kept as a byte); a corner survives when its score is strictly above the scores of its eight
    neighbours (0 for a pixel that is no corner).  -> x, y, score in row-major order."""
    v = img.astype(np.int32)
    h, w = v.shape
    t = min(max(int(t), 0), 255)
    ctr = v[3:h - 3, 3:w - 3]
    d = np.stack([ctr - v[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])           # v - ring
    arcs = [np.stack([d[(k + q) % 16] for q in range(9)]) for k in range(16)]
    dark = np.max([a.min(0) for a in arcs], 0)              # the arc is darker than v - t'  <=>  t' < min over the arc of (v - ring)
    bright = np.max([(-a).min(0) for a in arcs], 0)
    m = np.maximum(dark, bright)                            # a corner at t'  <=>  t' < m
    score = np.zeros((h, w), np.int32)
    score[3:h - 3, 3:w - 3] = np.where(m > t, m - 1, 0)
    corner = np.zeros((h, w), bool)
    corner[3:h - 3, 3:w - 3] = m > t
    p = np.pad(score, 1)
    nb = np.max([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)], 0)
    ys, xs = np.nonzero(corner & (score > nb))
    return xs, ys, score[ys, xs], score, corner
