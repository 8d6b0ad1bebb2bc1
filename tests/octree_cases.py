"""The inputs of tests/test_octree_cases.py (CPU) and tests/test_octree_gpu.py (GPU): named candidate sets for k_octree
(ssvio_amd/csrc/octree.hip), built deterministically with plain numpy, and a numpy restatement of the plan's geometry.

Images give the octree a few thousand well-spread candidates with varied responses.  The sets here are what images never give:
thousands of equal responses (every winner decided by candidate index, phase 2 all size ties), responses that rise with the index,
candidate counts on the edges of the kernel's thread chunks (1024 k +- 1) and on its capacities, a cluster that never splits, empty
roots, one candidate per root, budgets N around 1, 4 * nIni and M, and batches in which every (image, level) workgroup has a problem
of its own.

A case is a plan key plus, per (image, level), a candidate set in reference order: cell-row-major, row-major inside a cell -- the
order k_fast_cells leaves and k_octree gathers.  Pixels are distinct, a cell holds at most 256 (CELL_CAP), every pixel lies in the
one grid cell whose FAST interior (the cell's ROI less a 3-px frame) holds it: `order` sorts a point set so and asserts all that.

The plan's arithmetic (level sizes, per-level budgets, the cell grid: plan_levels / make_cells of ssvio_amd/csrc/orb.hip) is written
down a second time in `geometry`; tests/test_octree_cases.py holds it against ssx_orb_debug_plan, which also shows, through the bytes
of the octree scratch buffer, which of the kernel's four builds a key selects (`scratch_bytes`).

  the four builds   keys in LDS: up to 0.6 Mpx, else in global scratch.  Node tables in LDS while 50 * LN + 4 * (cells + 8) + 6 * 16384
                    (keys in LDS; 0 otherwise) fits 158 KB, LN = max(N, 256) + 8 rounded up to 8.  With the keys in LDS that is N up to
                    ~1250, so 400 x 240 detect-only has them in LDS at nfeatures <= 1000 and in global scratch at 3000.  With the keys in
                    global scratch the tables fit up to N ~ 3180: nfeatures 1000 and 3000 both keep them in LDS, 4000 puts them in global
                    scratch.  A pyramid never gives its level 0 that much (nfeatures <= 4088), so the multi-level cases reach global
                    tables on the small image only, at nfeatures 4088 (level 0: 1316).
"""
import functools

import numpy as np

F = np.float32
CELL_CAP, CAND_CAP, CAND_CAP_BIG, SEL_CAP, BORDER = 256, 16384, 65535, 4096, 16     # orb_ws.hpp; BORDER = EDGE_THRESHOLD - 3
OCT_NODE_BYTES, OCT_LDS_BUDGET, OCT_THREADS = 50, 158 * 1024, 1024


def key(rows, cols, nfeatures, images=1, nlevels=1, detect_only=True, scale=1.2):
    return dict(rows=rows, cols=cols, nfeatures=nfeatures, images=images, nlevels=nlevels, detect_only=detect_only, scale=scale)


def make_cells(rows, cols):
    """make_cells (orb.hip): -> int array [cells, 4], per cell the half-open interior x0, x1, y0, y1 relative to the border"""
    out = []
    max_x, max_y = cols - BORDER, rows - BORDER
    width, height = F(max_x - BORDER), F(max_y - BORDER)
    n_cols, n_rows = int(width / F(30)), int(height / F(30))
    if n_cols < 1 or n_rows < 1:
        return np.zeros((0, 4), np.int64)
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
            out.append((j * w_cell + 3, j * w_cell + w - 3, i * h_cell + 3, i * h_cell + h - 3))
    return np.array(out, np.int64).reshape(-1, 4)


def geometry(k):
    """plan_levels + plan_cells + plan_octree in numpy: levels as planned, per level rows, cols, budget N, cells, nIni, and the build"""
    L = 1 if k["detect_only"] else k["nlevels"]
    sc = [F(1)]
    for _ in range(1, L):
        sc.append(F(sc[-1] * F(k["scale"])))
    inv = [F(1) / s for s in sc]
    if k["detect_only"]:
        feat = [k["nfeatures"]]
    else:
        factor = F(1) / F(k["scale"])
        n_des = F(F(k["nfeatures"]) * (F(1) - factor)) / (F(1) - F(float(factor) ** L))
        feat = []
        for _ in range(L - 1):
            feat.append(int(np.rint(n_des)))
            n_des = F(n_des * factor)
        feat.append(max(k["nfeatures"] - sum(feat), 0))
    lvl_cols = [int(np.rint(F(k["cols"]) * i)) for i in inv]
    lvl_rows = [int(np.rint(F(k["rows"]) * i)) for i in inv]
    cells = [make_cells(r, c) for r, c in zip(lvl_rows, lvl_cols)]
    n_ini = [int(np.floor(F(c - 2 * BORDER) / F(r - 2 * BORDER) + F(0.5))) if r > 2 * BORDER else 0 for r, c in zip(lvl_rows, lvl_cols)]
    ln = (max([256] + feat) + 8 + 7) & ~7
    global_keys = lvl_rows[0] * lvl_cols[0] > 600000
    key_lds = 0 if global_keys else 6 * CAND_CAP
    global_tab = OCT_NODE_BYTES * ln + 4 * (max([1] + [len(c) for c in cells]) + 8) + key_lds > OCT_LDS_BUDGET
    slots_big = (CAND_CAP_BIG + OCT_THREADS - 1) // OCT_THREADS * OCT_THREADS
    stride = ((6 * slots_big if global_keys else 0) + (OCT_NODE_BYTES * ln if global_tab else 0) + 255) & ~255 if global_keys or global_tab else 0
    return dict(L=L, rows=lvl_rows, cols=lvl_cols, feat=feat, cells=cells, n_ini=n_ini, global_keys=global_keys, global_tab=global_tab,
                cap=CAND_CAP_BIG if global_keys else CAND_CAP, scratch_bytes=max(stride * k["images"] * L, 256))


def order(cells, xy):
    """the points in reference order; asserts: distinct, each in a cell, at most CELL_CAP per cell"""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    cell = np.full(len(xy), -1, np.int64)
    for lo in range(0, len(xy), 8192):
        p = xy[lo:lo + 8192]
        inside = ((p[:, None, 0] >= cells[None, :, 0]) & (p[:, None, 0] < cells[None, :, 1]) &
                  (p[:, None, 1] >= cells[None, :, 2]) & (p[:, None, 1] < cells[None, :, 3]))
        assert inside.sum(axis=1).max(initial=1) == 1 and inside.any(axis=1).all(), "a point in no cell (or in two)"
        cell[lo:lo + 8192] = inside.argmax(axis=1)
    assert len(np.unique(xy[:, 1] * 4096 + xy[:, 0])) == len(xy), "duplicate pixels"
    assert np.bincount(cell, minlength=1).max(initial=0) <= CELL_CAP, "more than CELL_CAP points in a cell"
    return xy[np.lexsort((xy[:, 0], xy[:, 1], cell))]


def lattice(cells, M, x_from=0, step=2):
    """M points on a lattice of every `step`-th pixel, dealt evenly to the cells (x >= x_from only), spread over each cell"""
    per = []
    for x0, x1, y0, y1 in cells:
        xs, ys = np.arange(x0, x1, step), np.arange(y0, y1, step)
        xs = xs[xs >= x_from]
        per.append(np.stack([np.tile(xs, len(ys)), np.repeat(ys, len(xs))], axis=1))
    room = np.array([min(len(p), CELL_CAP) for p in per])
    assert room.sum() >= M, "the lattice holds %d points, %d wanted" % (room.sum(), M)
    t = 0
    while np.minimum(room, t).sum() < M:
        t += 1
    quota = np.minimum(room, t)
    excess = quota.sum() - M
    for c in range(len(quota) - 1, -1, -1):
        if excess and quota[c] == t:
            quota[c] -= 1
            excess -= 1
    pts = [p[(np.arange(q) * len(p)) // q] for p, q in zip(per, quota) if q]
    return order(cells, np.concatenate(pts) if pts else np.zeros((0, 2), np.int64))


def scatter(cells, M, rng, avoid=None):
    """M distinct random pixels of the cells' interiors (none of `avoid`)"""
    seen = set() if avoid is None else {(int(x), int(y)) for x, y in avoid}
    out = []
    while len(out) < M:
        x0, x1, y0, y1 = cells[int(rng.integers(len(cells)))]
        if x1 <= x0 or y1 <= y0:
            continue
        p = (int(rng.integers(x0, x1)), int(rng.integers(y0, y1)))
        if p not in seen:
            seen.add(p)
            out.append(p)
    return np.array(out, np.int64).reshape(-1, 2)


def block(cells, side=20):
    """side x side adjacent pixels around the inner corner of the first four cells (a cell holds 256: the block needs all four)"""
    cx, cy = cells[0][1], cells[0][3]          # where the interiors of cells (0,0), (0,1), (1,0), (1,1) meet
    xs, ys = np.arange(cx - side // 2, cx + side // 2), np.arange(cy - side // 2, cy + side // 2)
    return np.stack([np.tile(xs, side), np.repeat(ys, side)], axis=1)


def responses(kind, M, rng):
    if kind == "equal":
        return np.full(M, 40, np.int64)
    if kind == "rising":                       # never falls with the index: the LAST candidate of a node holds its largest response
        return 1 + (np.arange(M) * 255) // max(M, 1)
    if kind == "few":                          # four values: long runs of ties
        return rng.integers(20, 24, M)
    return rng.integers(1, 256, M)             # "varied"


def one_set(g, level, kind, M, seed, x_from=0, points=None):
    rng = np.random.default_rng(seed)
    cells = g["cells"][level]
    xy = lattice(cells, M, x_from) if points is None else order(cells, points(cells, rng))
    return xy, responses(kind, len(xy), rng)


# name -> (key, {(image, level): set spec}, self-checks).  Set spec: dict(kind, M, seed[, x_from, points]).
# Self-checks (tests/test_octree_cases.py): n_ini per level 0, and per case any of phase2 (oracle returns N..N+2 < M), block (oracle returns 1)
A = dict(rows=240, cols=400)          # keys in LDS, 2 roots
K = dict(rows=376, cols=1241)         # keys in LDS, 4 roots
C1 = dict(rows=601, cols=1000)        # keys in global scratch, 2 roots
C2 = dict(rows=776, cols=776)         # keys in global scratch, 1 root: the level that can hold 65535 candidates in one node


def _block_plus(cells, rng):
    b = block(cells)
    return np.concatenate([b, scatter(cells, 300, rng, avoid=b)])


def _per_root(n_roots, width):
    def pts(cells, rng):
        # one pixel per root, at the root's middle column on the first cell row
        return np.array([[int((r + 0.5) * width / n_roots), cells[0][2] + 5] for r in range(n_roots)], np.int64)
    return pts


def _cases():
    c = {}

    def add(name, k, sets, n_ini, builds, **checks):
        c[name] = dict(name=name, key=k, sets=sets, n_ini=n_ini, builds=builds, checks=checks)

    def single(name, dims, nfeatures, n_ini, builds, kind, M, seed, **kw):
        checks = {q: kw.pop(q) for q in ("phase2", "block") if q in kw}
        add(name, key(nfeatures=nfeatures, **dims), {(0, 0): dict(kind=kind, M=M, seed=seed, **kw)}, n_ini, builds, **checks)

    LL, LG, GL, GG = (False, False), (True, False), (False, True), (True, True)      # (global_tab, global_keys)
    # ---- keys in LDS, tables in LDS
    single("A/equal", A, 1000, 2, LL, "equal", 3000, 1, phase2=True)
    single("A/rising", A, 1000, 2, LL, "rising", 3000, 2, phase2=True)
    for M in (1, 2, 1023, 1024, 1025, 2047, 2049):
        single("A/M%d" % M, A, 500, 2, LL, "few", M, 10 + M)
    for M in (16383, 16384, 16385):
        single("A/M%d" % M, A, 1000, 2, LL, "few", M, 20 + M)
    for N in (1, 5, 500):
        single("A/block/N%d" % N, A, N, 2, LL, "varied", 400, 30, points=lambda cells, rng: block(cells), block=True)
    single("A/block+300", A, 200, 2, LL, "varied", 700, 31, points=_block_plus)
    single("A/per_root", A, 100, 2, LL, "equal", 2, 32, points=_per_root(2, 368))
    for N in (1, 3, 8, 1199, 1200, 1205):
        single("A/sweep/N%d" % N, A, N, 2, LL, "varied", 1200, 40)
    single("A/sweep/N600", A, 600, 2, LL, "varied", 1200, 40, phase2=True)
    # ---- keys in LDS, tables in global scratch
    single("B/equal", A, 3000, 2, LG, "equal", 6000, 3, phase2=True)
    single("B/rising", A, 3000, 2, LG, "rising", 6000, 4, phase2=True)
    single("B/M1025", A, 3000, 2, LG, "few", 1025, 50)
    single("B/M16385", A, 3000, 2, LG, "few", 16385, 51, phase2=True)
    for N in (2999, 3000, 3005):
        single("B/sweep/N%d" % N, A, N, 2, LG, "varied", 3000, 52)
    single("B/sweep/N2000", A, 2000, 2, LG, "varied", 3000, 52, phase2=True)
    # ---- four roots: everything in the rightmost one, and one candidate in each
    single("K/right_root", K, 500, 4, LL, "few", 2000, 60, x_from=920, phase2=True)
    single("K/per_root", K, 500, 4, LL, "equal", 4, 61, points=_per_root(4, 1209))
    # ---- keys in global scratch
    single("C1/few/N1000", C1, 1000, 2, GL, "few", 30000, 70, phase2=True)
    single("C1/M1025/N4000", C1, 4000, 2, GG, "few", 1025, 71)
    single("C1/per_root", C1, 3000, 2, GL, "equal", 2, 72, points=_per_root(2, 968))
    single("C2/equal/N3000", C2, 3000, 1, GL, "equal", 20000, 73, phase2=True)
    single("C2/rising/N4000", C2, 4000, 1, GG, "rising", 20000, 74, phase2=True)
    for N in (1, 1000):
        single("C2/block/N%d" % N, C2, N, 1, GL, "varied", 400, 75, points=lambda cells, rng: block(cells), block=True)
    for M in (65535, 65536, 65537):
        single("C2/M%d/N1000" % M, C2, 1000, 1, GL, "few", M, 80 + M % 10, phase2=True)
    single("C2/M65536/N4000", C2, 4000, 1, GG, "equal", 65536, 90, phase2=True)
    # ---- every (image, level) workgroup its own problem, some empty
    small = [[700, 0, 333, 1], [0, 1500, 2, 90], [1025, 64, 0, 517]]
    big = [[20000, 0, 3000], [1, 9000, 0], [0, 2049, 6001]]
    kinds = ("few", "varied", "equal", "rising")
    for name, dims, nf, nl, counts, builds, n_ini in (("D/small/n1000", A, 1000, 4, small, LL, 2), ("D/small/n4088", A, 4088, 4, small, LG, 2),
                                                      ("D/big/n3000", C1, 3000, 3, big, GL, 2)):
        sets = {(i, l): dict(kind=kinds[(i + l) % 4], M=counts[i][l], seed=100 + 10 * i + l) for i in range(3) for l in range(nl) if counts[i][l]}
        add(name, key(nfeatures=nf, images=3, nlevels=nl, detect_only=False, **dims), sets, n_ini, builds)
    return c


CASES = _cases()
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (case, geometry, {(image, level): (xy int [M, 2], response int [M])}); made once per session, shared, read-only"""
    case = CASES[name]
    g = geometry(case["key"])
    sets = {}
    for (i, l), s in sorted(case["sets"].items()):
        xy, r = one_set(g, l, s["kind"], s["M"], s["seed"], s.get("x_from", 0), s.get("points"))
        assert len(xy) == s["M"], (name, i, l, len(xy))
        xy.setflags(write=False); r.setflags(write=False)
        sets[(i, l)] = (xy, r)
    return case, g, sets


def candidates(sets):
    """the sets of a case as the tap takes them: int32 [n, 5] rows (image, level, x, y, response)"""
    rows = [np.column_stack([np.full(len(xy), i), np.full(len(xy), l), xy, r]) for (i, l), (xy, r) in sorted(sets.items())]
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 5), np.int32)


def keypoints(po, xy, r):
    """a set as the oracle takes it"""
    kp = np.zeros(len(xy), po.KP_DTYPE)
    kp["x"] = xy[:, 0]; kp["y"] = xy[:, 1]; kp["response"] = r
    kp["size"] = 7; kp["angle"] = -1; kp["class_id"] = -1
    return kp


def oracle_select(po, g, level, xy, r):
    """po.octree on the first `cap` candidates of a level -> int [n, 3] (x, y, response) in list order"""
    kp = keypoints(po, xy[:g["cap"]], r[:g["cap"]])
    out = po.octree(kp, BORDER, g["cols"][level] - BORDER, BORDER, g["rows"][level] - BORDER, g["feat"][level])
    return np.stack([out["x"], out["y"], out["response"]], axis=1).astype(np.int32)
