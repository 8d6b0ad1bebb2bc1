"""The plan of the ORB front-end without a GPU (ssx_orb_debug_plan, include/ssx_test_hooks.h): the arena layout, the per-level
tables and the output capacity over the cases of tools/orb_plan_ab.py (every shape and parameter set of tests/test_orb_gpu.py, the
batch sizes of the headline and of the keyframe detection), and the refusals of plan() with their order.

plan() has six refusals.  Two check the arguments (image side, parameters) and are what tests/test_misuse_gpu.py provokes on a GPU.
Of the four behind them only the resize scale can be reached through an entry point: a budget of at most SEL_CAP - 8 features never
gives a level more than that, at most (4000 / 30)^2 cells of 4 bytes fit the octree's LDS, and a cell's ROI is at most
ceil(w / floor(w / 30)) + 6 <= 66 < 72 pixels wide.  The level cap and the octree's LDS are therefore reached with the hook's
`unchecked` flag (the argument checks skipped), the cell ROI by no input at all: it has no case."""
import pytest

from ssvio_amd import _lib
from tools.orb_plan_ab import CASES, FAILING, INVALID, case, name, plan_info

MAX_LEVELS, EDGE_THRESHOLD = 8, 19


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("c", CASES, ids=name)
def test_plan_layout_and_tables(lib, c):
    p = plan_info(lib, c)
    assert p.status == _lib.SSX_OK, p.error
    assert p.n_buffers == 17 and all(d != 0 for d in p.digest)
    spans = [(p.buf_off[b], p.buf_bytes[b]) for b in range(p.n_buffers)]
    for off, nbytes in spans:
        assert off % 256 == 0 and nbytes > 0 and off + nbytes <= p.arena_bytes
    for (a, na), (b, _) in zip(spans, spans[1:]):             # (memory order: disjoint when each ends before the next begins)
        assert a + na <= b
    nl = p.nlevels
    assert nl == (1 if c["detect"] else c["nlevels"])
    for tab in (p.lvl_cell0, p.gauss_tile0):
        assert tab[0] == 0 and all(tab[l] <= tab[l + 1] for l in range(MAX_LEVELS))
        assert all(tab[l] == tab[nl] for l in range(nl, MAX_LEVELS + 1))
    need = 0
    for l in range(nl):
        bw, bh = p.lvl_cols[l] - 2 * (EDGE_THRESHOLD - 3), p.lvl_rows[l] - 2 * (EDGE_THRESHOLD - 3)
        n_ini = (2 * bw + bh) // (2 * bh) if bh > 0 and bw > 0 else 0   # lround(bw / bh), never below 0
        need += max(p.feat[l] + 4, 4 * n_ini + 4)
    assert p.out_cap >= need
    assert sum(p.feat[l] for l in range(nl)) >= c["nfeatures"] if not c["detect"] else p.feat[0] == c["nfeatures"]


@pytest.mark.parametrize("which", sorted(FAILING))
def test_plan_refusals_and_their_order(lib, which):
    c, status, text = FAILING[which]
    p = plan_info(lib, c)
    assert p.status == status and text in p.error.decode(), (p.status, p.error)
    assert all(d == 0 for d in p.digest) and p.arena_bytes == 0


def test_plan_refuses_more_octree_roots_than_the_kernel_places(lib):
    """k_octree places at most 64 root nodes (nIni = a level's (cols - 32) / (rows - 32), rounded); a level with grid cells and more
    roots came back empty and silent, so the plan refuses the key, naming the level and its aspect.  62 rows leave 30: nIni 64 up to
    1966 columns (1934 / 30 = 64.47), 65 from 1967 (64.5 rounds up), 66 at 2000.  A level WITHOUT cells (the pyramid's upper levels
    here, 52 rows and less) refuses nothing, and a tall level (nIni 0: 300 x 45 of tests/test_orb_gpu.py::test_degenerate_small_images)
    still plans and selects nothing, as in the reference."""
    for cols, n_ini in ((1952, 64), (1966, 64), (1967, 65), (2000, 66)):
        for kw in (dict(detect=1, nfeatures=100), dict(nfeatures=500, nlevels=8)):
            p = plan_info(lib, case(62, cols, **kw))
            if n_ini <= 64:
                assert p.status == _lib.SSX_OK, p.error
                assert 1 <= p.lvl_cell0[1] <= (cols - 32) // 30 and p.out_cap >= 4 * n_ini + 4
                assert all(p.lvl_cell0[l] == p.lvl_cell0[1] for l in range(1, MAX_LEVELS + 1))        # cells on level 0 only
            else:
                assert p.status == _lib.SSX_ERR_UNSUPPORTED
                assert p.error.decode() == "ssx_orb: level 0 (%dx62) is %d times as wide as high: the octree takes at most 64 root nodes" % (cols, n_ini)
                assert all(d == 0 for d in p.digest) and p.arena_bytes == 0
    assert plan_info(lib, case(300, 45, nlevels=6, nfeatures=300)).status == _lib.SSX_OK
    assert plan_info(lib, case(45, 300, nlevels=6, nfeatures=300)).status == _lib.SSX_OK


def test_plan_rejections_of_the_misuse_test(lib):
    """tests/test_misuse_gpu.py::test_orb_entry_points_reject_bad_arguments: 0 levels, scale < 1, a negative budget, too many levels
    (ssx_orb_extract on 100 x 160) and an absurd height (ssx_orb_detect)"""
    for kw in (dict(nlevels=0), dict(scale=0.9), dict(nfeatures=-5), dict(nlevels=40)):
        p = plan_info(lib, case(100, 160, **{**dict(nfeatures=100, nlevels=3), **kw}))
        assert p.status == INVALID and p.error.startswith(b"ssx_orb: unsupported parameters"), kw
    p = plan_info(lib, case(100000, 160, detect=1, nfeatures=100, nlevels=3))
    assert p.status == INVALID and p.error.startswith(b"ssx_orb: image 160x100000 outside the supported range")
    assert plan_info(lib, case(100, 160, nfeatures=100, nlevels=3)).status == _lib.SSX_OK      # the good call beside them
