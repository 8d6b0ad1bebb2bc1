"""GPU parity of the pyramidal LK tracker (N1) against the CPU oracle: BIT-EXACT pyramids, Scharr images, tracked
positions (f32 bit patterns), status flags and errors -- the normal matrix / mismatch sums are exact integers on
both sides, every float operation is the same IEEE operation in the same order.  (The oracle itself is "parity
unpinned vs OpenCV": tests/test_oracle_lk.py.)"""
import numpy as np
import pytest

from ssvio_amd import lk
from tools.synth import make_stereo_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kitti():
    return make_stereo_pair(seed=0)


def _points(po, img, n=400):
    k, _ = po.orb_extract(img, prm=po.orb_params(nfeatures=n, nlevels=1))
    return np.stack([k["x"], k["y"]], 1).astype(np.float32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_pyramid_and_scharr_bit_exact(ctx, po, kitti):
    L, R, _ = kitti
    pts = _points(po, L, 50)
    lk.calcOpticalFlowPyrLK(ctx, L, R, pts, pts)
    prev, nxt = L, R
    for level in range(4):
        if level > 0:
            prev, nxt = po.lk_pyr_down(prev), po.lk_pyr_down(nxt)
        assert np.array_equal(lk.stage_level(ctx, 0, level), prev), f"prev pyramid level {level}"
        assert np.array_equal(lk.stage_level(ctx, 1, level), nxt), f"next pyramid level {level}"
        assert np.array_equal(lk.stage_deriv(ctx, level), po.lk_scharr(prev)), f"Scharr level {level}"


def test_stereo_tracking_with_initial_flow_bit_exact(ctx, po, kitti):
    """FindFeaturesInRight (frontend.cpp:374-384): left -> right, initial guess = the left position"""
    L, R, disp = kitti
    pts = _points(po, L, 1500)
    g = lk.calcOpticalFlowPyrLK(ctx, L, R, pts, pts)
    o = po.lk_track(L, R, pts, pts)
    assert g[3] == o[3] == 3
    assert _same(g[1], o[1]) and _same(g[0], o[0]) and _same(g[2], o[2])
    ok = g[1] > 0
    d = (pts[:, 0] - g[0][:, 0])[ok]
    true = disp[np.clip(np.round(pts[ok, 1]).astype(int), 0, 375), np.clip(np.round(pts[ok, 0]).astype(int), 0, 1240)]
    assert ok.mean() > 0.9 and np.median(np.abs(d - true)) < 0.1          # sanity against the synthetic ground truth


def test_temporal_tracking_bit_exact(ctx, po, kitti):
    """TrackLastFrame (frontend.cpp:156-166): last left -> current left; here a shifted + noisy copy, with and
    without initial guesses, other windows and iteration limits"""
    L = kitti[0]
    rng = np.random.default_rng(1)
    cur = np.roll(np.roll(L, 2, axis=0), -6, axis=1)
    cur = np.clip(cur.astype(np.int16) + rng.integers(-3, 4, cur.shape), 0, 255).astype(np.uint8)
    pts = _points(po, L, 800)
    guess = pts + np.array([-5.0, 1.5], np.float32)
    for kw, init in ((dict(), guess), (dict(), None), (dict(winSize=7, maxLevel=2), guess), (dict(winSize=15, maxLevel=1, maxCount=5), None),
                     (dict(maxLevel=0, epsilon=0.1), guess)):
        g = lk.calcOpticalFlowPyrLK(ctx, L, cur, pts, init, **kw)
        prm = po.lk_params(win=kw.get("winSize", 11), max_level=kw.get("maxLevel", 3), max_iters=kw.get("maxCount", 30),
                           eps=kw.get("epsilon", 0.01), use_initial_flow=int(init is not None))
        o = po.lk_track(L, cur, pts, init, prm=prm)
        assert g[3] == o[3]
        assert _same(g[1], o[1]) and _same(g[0], o[0]) and _same(g[2], o[2]), kw
    g = lk.calcOpticalFlowPyrLK(ctx, L, cur, pts, guess)
    ok = g[1] > 0
    assert ok.mean() > 0.9 and np.abs(np.median((g[0] - pts)[ok], 0) - np.array([-6.0, 2.0])).max() < 0.05


def test_edge_cases_bit_exact(ctx, po):
    """points outside / at the border / on flat areas, a pyramid cut short, no points, bad arguments"""
    L, R, _ = make_stereo_pair(seed=5, h=120, w=160, n_blobs=120)
    pts = np.array([[-40.0, 30.0], [30.0, 400.0], [500.0, 30.0], [0.0, 0.0], [159.0, 119.0], [5.2, 3.7], [155.5, 60.0],
                    [80.0, 60.0], [-5.5, -5.5], [164.9, 124.9]], np.float32)
    for a, b in ((L, R), (L, L), (np.full_like(L, 90), np.full_like(L, 90))):
        g = lk.calcOpticalFlowPyrLK(ctx, a, b, pts, pts)
        o = po.lk_track(a, b, pts, pts)
        assert g[3] == o[3] and _same(g[1], o[1]) and _same(g[0], o[0]) and _same(g[2], o[2])
    tiny = make_stereo_pair(seed=6, h=40, w=60, n_blobs=30)[0]
    g = lk.calcOpticalFlowPyrLK(ctx, tiny, tiny, np.array([[30.0, 20.0]], np.float32))
    o = po.lk_track(tiny, tiny, np.array([[30.0, 20.0]], np.float32), prm=po.lk_params(use_initial_flow=0))
    assert g[3] == o[3] == 1 and _same(g[0], o[0]) and _same(g[1], o[1])
    g = lk.calcOpticalFlowPyrLK(ctx, L, R, np.zeros((0, 2), np.float32))
    assert g[0].shape == (0, 2) and g[1].shape == (0,)
    with pytest.raises(Exception):
        lk.calcOpticalFlowPyrLK(ctx, L, R, pts, pts, winSize=10)          # even window
    with pytest.raises(ValueError):
        lk.calcOpticalFlowPyrLK(ctx, L, R[:50], pts)


def test_chained_tracking_reuses_the_previous_pyramid(ctx, po):
    """ssx_lk_track_next: frame t -> t+1 with the pyramid of frame t kept from the previous call; same bits as the
    two-image call and as the oracle, over a 4-frame sequence; refused without a matching previous call"""
    from ssvio_amd import Context
    from ssvio_amd._lib import SsxError
    from tools.synth import make_lateral_sequence
    frames = [f[0] for f in make_lateral_sequence(n_frames=4, seed=2)[0]]
    pts = _points(po, frames[0], 600)
    fresh = Context(0)
    with pytest.raises(SsxError):
        lk.calcOpticalFlowPyrLK(fresh, None, frames[1], pts)              # nothing to chain to
    g = lk.calcOpticalFlowPyrLK(fresh, frames[0], frames[1], pts)
    o = po.lk_track(frames[0], frames[1], pts, prm=po.lk_params(use_initial_flow=0))
    assert _same(g[0], o[0]) and _same(g[1], o[1])
    for t in (1, 2):
        keep = g[1] > 0
        pts = g[0][keep]
        g = lk.calcOpticalFlowPyrLK(fresh, None, frames[t + 1], pts)
        o = po.lk_track(frames[t], frames[t + 1], pts, prm=po.lk_params(use_initial_flow=0))
        assert _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]), t
        assert np.array_equal(lk.stage_level(fresh, 0, 2), po.lk_pyr_down(po.lk_pyr_down(frames[t])))
        assert (g[1] > 0).mean() > 0.8
    with pytest.raises(SsxError):
        lk.calcOpticalFlowPyrLK(fresh, None, frames[3], pts, winSize=7)   # other window: the kept pyramid does not fit
    with pytest.raises(SsxError):
        lk.calcOpticalFlowPyrLK(fresh, None, frames[3][:100], pts)        # other size
    fresh.close()


def test_track_batch_equals_single_calls(ctx, po):
    """ssx_lk_track_batch -- one frame of each of n streams in one call, every stream on its own slot of the context -- returns,
    per job, the bits of ssx_lk_track / ssx_lk_track_next on a context of the job's own: fresh and chained jobs mixed in one
    call, different point counts (one job without points), three chained steps, the jobs listed in another order than their slots."""
    import ssvio_amd
    S, steps = 6, 3
    rng = np.random.default_rng(7)
    seqs = []
    for s_ in range(S):
        base = make_stereo_pair(seed=20 + s_, h=240, w=400, n_blobs=500)[0]
        seqs.append([np.ascontiguousarray(np.roll(np.roll(base, k * (1 + s_ % 3), axis=1), k * (s_ % 2), axis=0)) for k in range(steps + 1)])
    pts = [_points(po, seqs[s_][0], 40 + 37 * s_) if s_ != 4 else np.zeros((0, 2), np.float32) for s_ in range(S)]
    # reference: every stream alone on a context of its own
    ref = []
    for s_ in range(S):
        c = ssvio_amd.Context(0)
        p = pts[s_]
        out = []
        for k in range(steps):
            prev = seqs[s_][k] if (k == 0 or (s_ == 2 and k == 2)) else None          # stream 2 restarts its chain at step 2
            g = lk.calcOpticalFlowPyrLK(c, prev, seqs[s_][k + 1], p, p)
            out.append(g)
            p = g[0]
        ref.append(out)
        c.close()
    p_cur = [p.copy() for p in pts]
    order = [3, 0, 5, 1, 4, 2]
    for k in range(steps):
        jobs = [dict(slot=s_, prev=(seqs[s_][k] if (k == 0 or (s_ == 2 and k == 2)) else None), next=seqs[s_][k + 1], prev_pts=p_cur[s_], next_pts=p_cur[s_])
                for s_ in order]
        got = lk.track_batch(ctx, jobs)
        for s_, g in zip(order, got):
            r = ref[s_][k]
            assert _same(g[0], r[0]) and _same(g[1], r[1]) and _same(g[2], r[2]), (k, s_)
            p_cur[s_] = g[0]
    import pytest as _pt
    with _pt.raises(ssvio_amd.SsxError):                     # a slot twice in one call
        lk.track_batch(ctx, [dict(slot=1, prev=seqs[0][0], next=seqs[0][1], prev_pts=pts[0]), dict(slot=1, prev=seqs[1][0], next=seqs[1][1], prev_pts=pts[1])])
    with _pt.raises(ssvio_amd.SsxError):                     # a chained job on a slot that holds nothing
        lk.track_batch(ctx, [dict(slot=77, prev=None, next=seqs[0][1], prev_pts=pts[0])])


@pytest.mark.parametrize("h,w,win,max_level", [(120, 160, 11, 3), (121, 163, 11, 3), (97, 250, 7, 3), (113, 113, 15, 2), (200, 333, 5, 3), (64, 90, 11, 3),
                                               (111, 112, 11, 1), (130, 97, 13, 3), (376, 1241, 11, 2)])
def test_pyramids_borders_and_chains_over_sizes_and_windows(ctx, po, h, w, win, max_level):
    """Odd and even sizes at every level, windows 5 .. 15 (border 6 .. 16), 1 - 3 pyramid levels above the image, small top levels: the
    pyramid / derivative images of both frames level by level, points on a grid that reaches into the image corners (their windows
    read the reflected border of every level), and a chained third frame (the derivative images of a chained job's previous image were
    written one call earlier) -- all bit for bit the oracle's.  Covers k_lk_pyramid (one launch per image) and, where a level is too
    small for it, the per-level kernels."""
    from ssvio_amd import Context
    rng = np.random.default_rng(h * 1000 + w)
    L, R, _ = make_stereo_pair(seed=40 + h % 7, h=h, w=w, n_blobs=max(60, h * w // 150))
    T = np.clip(np.roll(L, (1, 2), (0, 1)).astype(np.int16) + rng.integers(-2, 3, L.shape), 0, 255).astype(np.uint8)
    gx, gy = np.meshgrid(np.linspace(0.5, w - 1.5, 12), np.linspace(0.5, h - 1.5, 9))
    pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    pts = np.concatenate([pts, np.array([[0, 0], [w - 1, h - 1], [w - 1, 0], [0, h - 1], [-3.5, 4.0], [w + 2.0, h / 2]], np.float32)])
    c = Context(0)
    prm = po.lk_params(win=win, max_level=max_level)
    g = lk.calcOpticalFlowPyrLK(c, L, R, pts, pts, winSize=win, maxLevel=max_level)
    o = po.lk_track(L, R, pts, pts, prm=prm)
    assert g[3] == o[3]
    assert _same(g[1], o[1]) and _same(g[0], o[0]) and _same(g[2], o[2])
    prev, nxt = L, R
    for level in range(g[3] + 1):
        if level > 0:
            prev, nxt = po.lk_pyr_down(prev), po.lk_pyr_down(nxt)
        assert np.array_equal(lk.stage_level(c, 0, level), prev) and np.array_equal(lk.stage_level(c, 1, level), nxt), level
        assert np.array_equal(lk.stage_deriv(c, level), po.lk_scharr(prev)), level
    # chained: R is now the previous image
    g2 = lk.calcOpticalFlowPyrLK(c, None, T, pts, pts, winSize=win, maxLevel=max_level)
    o2 = po.lk_track(R, T, pts, pts, prm=prm)
    assert _same(g2[1], o2[1]) and _same(g2[0], o2[0]) and _same(g2[2], o2[2])
    prev = R
    for level in range(g2[3] + 1):
        if level > 0:
            prev = po.lk_pyr_down(prev)
        assert np.array_equal(lk.stage_deriv(c, level), po.lk_scharr(prev)), ("chained", level)
    c.close()


def test_wide_and_narrow_calls_interleave(ctx, po):
    """Calls of up to 16 jobs build their pyramids and derivative images with k_lk_pyramid (one launch per image, the derivative
    images of the new frame kept for the chained job that follows); wider calls use the per-level kernels and keep none.  A slot that
    goes wide -> narrow -> narrow -> wide gets the oracle's bits at every step (the narrow call after a wide one computes the missing
    derivative images itself), and so do the slots that only see the wide calls."""
    from ssvio_amd import Context
    c = Context(0)
    S, few = 20, 4
    base = [make_stereo_pair(seed=60 + s_, h=120, w=168, n_blobs=200)[0] for s_ in range(S)]
    frames = [[np.ascontiguousarray(np.roll(base[s_], (k * (s_ % 2), k * (1 + s_ % 3)), (0, 1))) for k in range(5)] for s_ in range(S)]
    gx, gy = np.meshgrid(np.linspace(6, 160, 8), np.linspace(6, 112, 6))
    pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    cur = [0] * S                                                       # the frame each slot's kept pyramid belongs to

    def call(slots, fresh):
        jobs = [dict(slot=s_, prev=frames[s_][cur[s_]] if fresh else None, next=frames[s_][cur[s_] + 1], prev_pts=pts, next_pts=pts) for s_ in slots]
        got = lk.track_batch(c, jobs)
        for s_, g in zip(slots, got):
            o = po.lk_track(frames[s_][cur[s_]], frames[s_][cur[s_] + 1], pts, pts)
            assert _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]), (s_, cur[s_], fresh, len(slots))
            cur[s_] += 1

    call(range(S), True)                   # wide, fresh
    call(range(few), False)                # narrow, chained to a wide call
    call(range(few), False)                # narrow, chained to a narrow call
    call(range(S), False)                  # wide, chained: slots 0 .. 3 come from a narrow call, the others from the first wide one
    call(range(few, 2 * few), False)       # narrow after wide for other slots
    c.close()


@pytest.mark.parametrize("h,w,max_level,nj", [(120, 168, 3, 3), (120, 168, 3, 17), (240, 400, 4, 3), (240, 400, 4, 17)])
def test_every_image_intake_gives_the_same_bits(po, h, w, max_level, nj):
    """The four ways an image reaches the device (csrc/lk.hip: choose_intake) give, per job, the bytes of the staged path in points,
    status and error: one pinned block sliced at a constant distance (one DMA copy), the same with a slice left out, a pinned block per
    image and a device buffer per image (both listed in descending address order, so that no arena is seen) -- for k_lk_pyramid (3 jobs
    at four levels) and the per-level kernels (17 jobs, or five levels), a fresh call and then a chained one through the same intake, one
    job without points.  Which intake and which pyramid kernel a call took is asserted through ssx_lk_debug_last_call."""
    import lk_call_cases as cc
    from ssvio_amd import Context
    from tools.lk_call_trace import Replay
    cases = {c["name"]: c for c in cc.CASES}
    c = Context(0)
    ref = []
    host = Replay(c, cases[f"intake-{h}x{w}-{nj}jobs-{cc.HOST}"])
    for k in host.c["calls"]:
        ref.append(host.run(k))
        info = lk.last_call(c)
        assert (info.intake, bool(info.use_fused)) == (cc.STAGED, host.c["use_fused"])
        if nj == 3:
            prm = po.lk_params(max_level=max_level)
            for s_, (prev, nxt), p, g in zip(k["slots"], host.pairs, host.pts, ref[-1]):
                o = po.lk_track(host.frames[s_][host.cur[s_] - 1] if prev is None else prev, nxt, p, p, prm=prm)
                assert _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]), (s_, k["fresh"])
    for layout in (cc.ARENA, cc.ARENA_SKIP, cc.SEPARATE_HOST, cc.DEVICE):
        r = Replay(c, cases[f"intake-{h}x{w}-{nj}jobs-{layout}"])
        for k, want in zip(r.c["calls"], ref):
            got = r.run(k)
            info = lk.last_call(c)
            assert (info.intake, bool(info.use_fused)) == (r.c["intake"], r.c["use_fused"]), layout
            for j, (g, o) in enumerate(zip(got, want)):
                assert _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]), (layout, k["fresh"], j)
    c.close()


def _raw_batch_call(c, slot, prev, nxt, pts):
    """one job through ssx_lk_track_batch (host images) with the caller's arrays in view -> (status, next_pts, status bytes, err):
    a refused call returns no result, so what it left in the arrays is looked at here"""
    import ctypes as C
    arr = (lk.LkJob * 1)()
    job = dict(slot=slot, prev_pts=pts, next_pts=pts)
    _, guess, (npts, st, er) = lk._fill_job(arr[0], job, nxt.ctypes.data_as(lk.u8_p), nxt.strides[0], None if prev is None else prev.ctypes.data_as(lk.u8_p),
                                            0 if prev is None else prev.strides[0])
    st[:] = 7; er[:] = -1.0                                            # (neither is a value the tracker writes into all of them)
    prm = lk.LkParams(11, 3, 30, 0.01, 1e-4, 1)
    rc = lk._batch_fn(c.lib)(c.handle, 1, arr, nxt.shape[0], nxt.shape[1], C.byref(prm), 0)
    return rc, guess, npts, st, er


def test_a_call_of_another_size_drops_every_chain(po):
    """include/ssx.h, ssx_lk_track_next / ssx_lk_track_batch: a context holds chains for ONE (rows, cols, win, max_level); a call with
    another key drops them all, on every slot.  Size A on slot 0, size B on slot 1, then a chained A on slot 0: refused (SsxError's
    status, no result, next_pts as passed) -- and the refusal changes nothing: slot 1's B chain goes on with the oracle's bytes.  A
    fresh A call starts a new chain, and the chained call behind it gives the oracle's bytes from the kept pyramid of the right
    frame."""
    from ssvio_amd import Context, _lib
    sizes = {"A": (120, 160), "B": (97, 130)}
    frames, pts = {}, {}
    for n_, (h, w) in sizes.items():
        base = make_stereo_pair(seed=70 + h % 5, h=h, w=w, n_blobs=160)[0]
        frames[n_] = [np.ascontiguousarray(np.roll(base, (t, 2 * t), (0, 1))) for t in range(4)]
        gx, gy = np.meshgrid(np.linspace(4.5, w - 5.5, 10), np.linspace(4.5, h - 5.5, 6))
        pts[n_] = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
        assert len(pts[n_]) == 60
    A, B = frames["A"], frames["B"]
    c = Context(0)

    def oracle_bytes(got, prev, nxt, p):
        o = po.lk_track(prev, nxt, p, p)
        return _same(got[0], o[0]) and _same(got[1], o[1]) and _same(got[2], o[2])

    g = lk.track_batch(c, [dict(slot=0, prev=A[0], next=A[1], prev_pts=pts["A"], next_pts=pts["A"])])[0]                  # 1: fresh, size A, slot 0
    assert oracle_bytes(g, A[0], A[1], pts["A"])
    g = lk.track_batch(c, [dict(slot=1, prev=B[0], next=B[1], prev_pts=pts["B"], next_pts=pts["B"])])[0]                  # 2: fresh, size B, slot 1
    assert oracle_bytes(g, B[0], B[1], pts["B"])
    rc, guess, npts, st, er = _raw_batch_call(c, 0, None, A[2], pts["A"])                                                # 3: chained, size A, slot 0
    assert rc == _lib.SSX_ERR_INVALID_ARG and "no previous ssx_lk_track call" in c.lib.ssx_last_error(c.handle).decode()
    assert _same(npts, guess) and (st == 7).all() and (er == -1.0).all()
    with pytest.raises(_lib.SsxError):
        lk.track_batch(c, [dict(slot=0, prev=None, next=A[2], prev_pts=pts["A"], next_pts=pts["A"])])
    # (the refused call has not re-planned the context: size B's chain is still there)
    g = lk.track_batch(c, [dict(slot=1, prev=None, next=B[2], prev_pts=pts["B"], next_pts=pts["B"])])[0]
    assert oracle_bytes(g, B[1], B[2], pts["B"])
    g = lk.track_batch(c, [dict(slot=0, prev=A[1], next=A[2], prev_pts=pts["A"], next_pts=pts["A"])])[0]                  # 4: fresh, size A, slot 0
    assert oracle_bytes(g, A[1], A[2], pts["A"])
    with pytest.raises(_lib.SsxError):                                 # (and now size B's chain is gone in its turn)
        lk.track_batch(c, [dict(slot=1, prev=None, next=B[3], prev_pts=pts["B"], next_pts=pts["B"])])
    g = lk.track_batch(c, [dict(slot=0, prev=None, next=A[3], prev_pts=pts["A"], next_pts=pts["A"])])[0]                  # 5: chained, size A, slot 0
    assert oracle_bytes(g, A[2], A[3], pts["A"])
    kept, new = A[2], A[3]
    for level in range(4):
        if level > 0:
            kept, new = po.lk_pyr_down(kept), po.lk_pyr_down(new)
        assert np.array_equal(lk.stage_level(c, 0, level), kept) and np.array_equal(lk.stage_level(c, 1, level), new), level
    assert lk.stage_level(c, 0, 3).shape == (15, 20)
    c.close()


@pytest.mark.parametrize("nj", [5, 17])
def test_images_allocated_one_by_one_are_never_one_copy(po, record_property, nj):
    """A pinned allocation per image, the jobs listed in ASCENDING address order: what a cohort of two image sizes hands the library
    (host/stream_batcher.cpp: the streams of the larger size keep buffers of their own).  If the allocator happens to place them at
    equal distances and close together, pointer arithmetic sees an arena, and one copy over the range would cross whatever lies
    between the allocations.  So the library is ASKED first (ssx_lk_debug_intake: pointer queries only) and must not answer LK_ARENA;
    only then is the call made -- a fresh one, then a chained one -- and compared with the staged path's bytes.  Whether the allocator
    produced the adjacent layout is not in the test's hands: it is recorded (the deterministic check of the decision is
    tests/test_lk_plan.py::test_an_arena_is_one_allocation).  A real arena -- one pinned block, constant distance -- is still LK_ARENA,
    by the hook and by the call."""
    import ctypes as C
    import lk_call_cases as cc
    from ssvio_amd import Context
    h, w = 120, 168
    c, c_ref = Context(0), Context(0)
    lib = c.lib
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    base = [make_stereo_pair(seed=60 + s_, h=h, w=w, n_blobs=200)[0] for s_ in range(nj)]
    frames = [[np.ascontiguousarray(np.roll(base[s_], (t * (s_ % 2), t * (1 + s_ % 3)), (0, 1))) for t in range(3)] for s_ in range(nj)]
    gx, gy = np.meshgrid(np.linspace(6, 160, 8), np.linspace(6, 112, 6))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    pts = [grid[:0] if s_ == 1 else grid[:40 + s_ % 9] for s_ in range(nj)]                  # (one job without points)
    want_split = cc.EACH if nj <= 16 else cc.IN_PLACE                  # k_lk_pyramid up to 16 jobs: a copy per pinned image in front of it
    pins = []

    def pinned(nbytes):
        p = lib.ssx_host_alloc(nbytes)
        assert p
        pins.append(p)
        return p

    def one_by_one(images):
        """-> ascending addresses of separately pinned copies of the images, image j at address j"""
        addr = sorted(pinned(h * w) for _ in images)
        for a, img in zip(addr, images):
            C.memmove(a, img.ctypes.data, img.size)
        return addr

    def check(got, ref, what):
        for j, (g, o) in enumerate(zip(got, ref)):
            assert _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]), (what, j)

    try:
        ref = [lk.track_batch(c_ref, [dict(slot=s_, prev=frames[s_][0], next=frames[s_][1], prev_pts=pts[s_], next_pts=pts[s_]) for s_ in range(nj)]),
               lk.track_batch(c_ref, [dict(slot=s_, prev=None, next=frames[s_][2], prev_pts=pts[s_], next_pts=pts[s_]) for s_ in range(nj)])]
        assert lk.last_call(c_ref).intake == cc.STAGED
        for t, fresh in ((1, True), (2, False)):
            nxt = one_by_one([frames[s_][t] for s_ in range(nj)])
            prev = one_by_one([frames[s_][t - 1] for s_ in range(nj)]) if fresh else [None] * nj
            intake, adjacent = lk.debug_intake(c, nxt, h, w)           # ask ...
            record_property(f"{'fresh' if fresh else 'chained'}_call_pointers_pass_the_arena_arithmetic", adjacent)
            print(f"{nj} jobs, {'fresh' if fresh else 'chained'} call: separate allocations pass the arena's arithmetic: {adjacent}; distances "
                  f"{sorted({b - a for a, b in zip(nxt, nxt[1:])})}")
            assert intake == want_split, (intake, adjacent)
            got = lk.track_batch_ptrs(c, [dict(slot=s_, prev=prev[s_], next=nxt[s_], stride=w, prev_pts=pts[s_], next_pts=pts[s_]) for s_ in range(nj)], h, w)   # ... then run
            info = lk.last_call(c)
            assert (info.intake, info.arena_bytes, bool(info.use_fused)) == (want_split, 0, nj <= 16)
            check(got, ref[t - 1], ("one by one", t))
        # one pinned block sliced at a constant distance, on a context of its own: the arena of before
        a = Context(0)
        d = (h * w + 255) & ~255
        for t, fresh in ((1, True), (2, False)):
            block = [pinned(nj * d) for _ in range(2 if fresh else 1)]
            for s_ in range(nj):
                C.memmove(block[0] + s_ * d, frames[s_][t].ctypes.data, h * w)
                if fresh:
                    C.memmove(block[1] + s_ * d, frames[s_][t - 1].ctypes.data, h * w)
            nxt = [block[0] + s_ * d for s_ in range(nj)]
            assert lk.debug_intake(a, nxt, h, w) == (cc.IN_ARENA, True)
            got = lk.track_batch_ptrs(a, [dict(slot=s_, prev=block[1] + s_ * d if fresh else None, next=nxt[s_], stride=w, prev_pts=pts[s_], next_pts=pts[s_])
                                          for s_ in range(nj)], h, w)
            info = lk.last_call(a)
            assert (info.intake, info.arena_bytes) == (cc.IN_ARENA, (nj - 1) * d + h * w)
            check(got, ref[t - 1], ("arena", t))
            # the allocation must COVER the range: the same distances from further up the block, the last image reaching past its end
            assert lk.debug_intake(a, [p_ + d - 256 for p_ in nxt], h, w) == (want_split, True)
        a.close()
    finally:
        for p_ in pins:
            lib.ssx_host_free(p_)
        c.close(); c_ref.close()


def test_a_prepared_batch_is_one_arena(po):
    """lk.PreparedTrackBatch (what tools/bench_next.py times as the batched LK call) holds its images as the stream batcher does: one
    pinned arena, a slice per job, taken in one copy; per job the oracle's bytes."""
    import lk_call_cases as cc
    from ssvio_amd import Context
    c = Context(0)
    S, h, w = 3, 120, 168
    base = [make_stereo_pair(seed=60 + s_, h=h, w=w, n_blobs=200)[0] for s_ in range(S)]
    nxt = [np.ascontiguousarray(np.roll(b, (1, 2), (0, 1))) for b in base]
    gx, gy = np.meshgrid(np.linspace(6, 160, 8), np.linspace(6, 112, 6))
    pts = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
    lk.track_batch(c, [dict(slot=s_, prev=nxt[s_], next=base[s_], prev_pts=pts, next_pts=pts) for s_ in range(S)])          # fills the slots
    prep = lk.PreparedTrackBatch(c, [dict(slot=s_, prev=None, next=nxt[s_], prev_pts=pts, next_pts=pts) for s_ in range(S)])
    try:
        got = prep.run()
        info = lk.last_call(c)
        assert (info.intake, info.arena_bytes) == (cc.IN_ARENA, 2 * ((h * w + 255) & ~255) + h * w)
        for s_, g in enumerate(got):
            o = po.lk_track(base[s_], nxt[s_], pts, pts)
            assert _same(g[0], o[0]) and _same(g[1], o[1]) and _same(g[2], o[2]), s_
    finally:
        prep.close()
        c.close()
