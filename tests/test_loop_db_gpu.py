"""GPU parity of the device-resident keyframe database (ssx_kfdb_*: AddToKeyframeDatabase, DetectLoop, MatchFeatures of
src/ssvio/loopclosing.cpp:646, :72-103, :105-145) against a few lines of numpy over the CPU oracle's two primitives,
po.bow_score_l1 and po.bf_match.  DetectLoop and MatchFeatures are integer and ordered-double arithmetic, so every
comparison is exact: the scores are the oracle's doubles bit for bit, the winner, the pairs and the minimum distance
are equal."""
import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import loop as sloop
from ssvio_amd import voc as svoc
from ssvio_amd._lib import SsxError
from tools.synth import make_stereo_pair, make_vocabulary

pytestmark = pytest.mark.gpu

MAX_WORD = 6000            # word ids of the scan tests: a 1500-word query and a 1200-word row share about 300 words
ROW_LENGTHS = (0, 1, 64, 65, 1200, 255, 256, 257)      # around a wavefront's chunk of 64 and its four chunks in flight
EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.float64))


def make_bow(rng, n, max_word=MAX_WORD):
    """a synthetic BowVector: sorted unique ids, positive values normalised to sum 1"""
    ids = np.sort(rng.choice(max_word, n, replace=False)).astype(np.int32)
    vals = rng.random(n) + 0.05
    return ids, vals / vals.sum() if n else vals


def ref_detect(po, entries, query_id, query, threshold, min_id_gap=20):
    """DetectLoop (loopclosing.cpp:72-103) over [(kf_id, bow)] in id order -> (found, best id, best float, scores)"""
    scores, best, best_id = [], np.float32(0.0), None
    for kf_id, bow in entries:
        if query_id - kf_id < min_id_gap:
            break
        s = 0.0
        if len(query[0]) and len(bow[0]):
            s = po.bow_score_l1(query, bow)
            if np.float32(s) > best:
                best, best_id = np.float32(s), kf_id
        scores.append(s)
    found = best_id is not None and not best < np.float32(threshold)
    return found, best_id, best, np.array(scores, np.float64)


def ref_match(po, loop_desc, loop_cls, cur_desc, cur_cls):
    """MatchFeatures (loopclosing.cpp:105-135): match(loop, current), the distance screen, the std::set of pairs"""
    idx, dist = po.bf_match(loop_desc, cur_desc)
    md = int(dist.min())
    thr = max(2 * md, 30)
    pairs = sorted({(int(cur_cls[idx[i]]), int(loop_cls[i])) for i in range(len(idx)) if dist[i] <= thr})
    return np.array(pairs, np.int32).reshape(-1, 2), md


def fill(ctx, entries, hint=4):
    db = sloop.KeyframeDatabase(ctx, keyframes_hint=hint)
    for kf_id, bow in entries:
        db.add(kf_id, bow)
    return db


def check_detect(po, db, entries, query_id, query, threshold=0.0, min_id_gap=20):
    found, best_id, best, n_scored, scores = db.detect_loop(query_id, query, threshold, min_id_gap=min_id_gap, with_scores=True)
    r_found, r_id, r_best, r_scores = ref_detect(po, entries, query_id, query, threshold, min_id_gap)
    assert n_scored == len(r_scores)
    assert scores.tobytes() == r_scores.tobytes(), np.nonzero(scores != r_scores)[0][:8]
    assert found == r_found
    if found:
        assert best_id == r_id and best == r_best
    return found, best_id, best


@pytest.fixture(scope="module")
def scan(po):
    """300 rows (lengths 0, 1, 64, 65, 1200, 255, 256, 257 and random ones between) and the queries: 1500 words, 20 000 (global memory), the two
    sizes around the LDS limit, one word, none"""
    rng = np.random.default_rng(2024)
    rows = []
    for i in range(300):
        n = ROW_LENGTHS[i % 10] if i % 10 < len(ROW_LENGTHS) else int(rng.integers(200, 1200))
        rows.append((i, make_bow(rng, n)))
    queries = {"1500": make_bow(rng, 1500),
               "20000": make_bow(rng, 20000, max_word=60000),       # 240 KB of (id, value) pairs: searched in global memory
               "4097": make_bow(rng, 4097, max_word=12000),         # one word past what is staged in LDS
               "4096": make_bow(rng, 4096, max_word=12000),
               "1": make_bow(rng, 1, max_word=50),
               "empty": EMPTY}
    return rows, queries


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 300])
def test_scores_are_the_oracles_bits(ctx, po, scan, n):
    rows, queries = scan
    db = fill(ctx, rows[:n])                                  # 300 rows from a hint of 4: several growth steps of table and arena
    assert db.size() == (n, sum(len(b[0]) for _, b in rows[:n]), 0)
    for name, q in queries.items():
        found, _, _ = check_detect(po, db, rows[:n], 10 ** 6, q)
        assert not found or (n > 0 and name != "empty")
    db.close()


def test_gap_rule(ctx, po):
    rng = np.random.default_rng(5)
    ids = [3, 7, 10, 25, 40, 41, 60, 100, 4000000000]
    entries = [(i, make_bow(rng, 300)) for i in ids]
    db = fill(ctx, entries)
    q = make_bow(rng, 400)
    out = db.detect_loop(60, q, 0.0, with_scores=True)        # 40 has gap exactly 20: the last eligible; 41 has 19
    assert out[3] == 5 and len(out[4]) == 5
    check_detect(po, db, entries, 60, q)
    check_detect(po, db, entries, 61, q)                      # now 41 is eligible too
    assert db.detect_loop(61, q, 0.0)[3] == 6
    check_detect(po, db, entries, 4000000020, q)              # ids beyond 32 bits; everything eligible
    assert db.detect_loop(4000000020, q, 0.0)[3] == len(ids)
    for query_id in (10, 19, 22):                             # below min_id_gap (and 22 - 3 = 19): nothing is eligible
        found, best_id, best, n_scored, scores = db.detect_loop(query_id, q, 0.0, with_scores=True)
        assert not found and best_id is None and n_scored == 0 and len(scores) == 0
    assert db.detect_loop(23, q, 0.0)[3] == 1                 # 23 - 3 = 20
    check_detect(po, db, entries, 30, q, min_id_gap=5)        # another gap: 3 .. 25
    assert db.detect_loop(30, q, 0.0, min_id_gap=5)[3] == 4
    db.close()


def near_copy(rng, query, n=1200):
    """a row showing the query's place: n of its words with values within a factor of the query's"""
    pick = np.sort(rng.choice(len(query[0]), n, replace=False))
    vals = query[1][pick] * rng.uniform(0.7, 1.3, n)
    return query[0][pick].copy(), vals / vals.sum()


def float_tie(po, query, a):
    """entry B = A with ONE common word's value stepped down by nextafter 64 .. 1024 times so that score(B) != score(A) while
    np.float32 of both are equal; words and step counts are searched in a fixed order until one holds"""
    s_a = po.bow_score_l1(query, a)
    common = np.nonzero(np.isin(a[0], query[0]))[0]
    for w in common[:200]:
        for steps in (64, 128, 256, 512, 1024):
            vals = a[1].copy()
            vals[w:w + 1].view(np.int64)[0] -= steps          # np.nextafter(v, 0) `steps` times, for a positive double
            s_b = po.bow_score_l1(query, (a[0], vals))
            if s_b != s_a and np.float32(s_b) == np.float32(s_a):
                return (a[0].copy(), vals), s_a, s_b
    raise AssertionError("no float tie with differing doubles among the first 200 common words")


def test_float_tie_lowest_id_wins_even_when_doubles_differ(ctx, po):
    rng = np.random.default_rng(77)
    q = make_bow(rng, 1500)
    a = near_copy(rng, q)
    b, s_a, s_b = float_tie(po, q, a)
    assert s_b != s_a and np.float32(s_b) == np.float32(s_a)
    others = [make_bow(rng, 1200) for _ in range(70)]
    assert max(np.float32(po.bow_score_l1(q, o)) for o in others) < np.float32(s_a)     # A and B are the best
    bows = others[:10] + [b] + others[10:66] + [a] + others[66:]   # B (id 10) before A (id 67, another wavefront and workgroup)
    entries = list(enumerate(bows))
    db = fill(ctx, entries)
    found, best_id, best = check_detect(po, db, entries, 1000, q)
    assert found and best_id == 10 and best == np.float32(s_b)
    db.close()
    # the other way round the winner is A: the order decides, not the larger double
    bows = others[:10] + [a] + others[10:66] + [b] + others[66:]
    entries = list(enumerate(bows))
    db = fill(ctx, entries)
    found, best_id, best = check_detect(po, db, entries, 1000, q)
    assert found and best_id == 10
    db.close()
    # an exact duplicate: the first wins
    entries = [(5 * i + 2, bow) for i, bow in enumerate(others[:3] + [a] + others[3:40] + [a] + others[40:])]
    db = fill(ctx, entries)
    found, best_id, best = check_detect(po, db, entries, 1000, q)
    assert found and best_id == 5 * 3 + 2 and best == np.float32(s_a)
    db.close()


def test_threshold_is_strict_less_than_on_the_float_score(ctx, po):
    rng = np.random.default_rng(9)
    q = make_bow(rng, 800)
    entries = list(enumerate([make_bow(rng, 700) for _ in range(9)] + [near_copy(rng, q, 600)]))
    db = fill(ctx, entries)
    _, _, best, _ = ref_detect(po, entries, 100, q, 0.0)
    assert best > 0
    up, down = np.nextafter(best, np.float32(2.0)), np.nextafter(best, np.float32(0.0))
    assert db.detect_loop(100, q, best)[:3] == (True, 9, best)          # max_score < threshold is false at equality
    assert db.detect_loop(100, q, down)[:3] == (True, 9, best)
    assert db.detect_loop(100, q, up)[:3] == (False, None, None)
    for thr in (best, up, down):
        check_detect(po, db, entries, 100, q, threshold=thr)
    # no common word with anything: every score is 0, nothing is found even at threshold 0
    far = (q[0][:50] + MAX_WORD, q[1][:50] / q[1][:50].sum())
    assert not db.detect_loop(100, far, 0.0)[0]
    check_detect(po, db, entries, 100, far)
    db.close()


def flip_bits(rng, desc, lo, hi):
    out = desc.copy()
    for row in out:
        for bit in rng.choice(256, int(rng.integers(lo, hi + 1)), replace=False):
            row[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def match_case(rng, n_loop, n_cur, min_flips, n_classes=12):
    """current descriptors = loop descriptors with min_flips .. 40 flipped bits plus random ones; few distinct class ids"""
    loop_desc = rng.integers(0, 256, (n_loop, 32), dtype=np.uint8)
    n_copy = max(1, min(n_cur, n_loop) * 2 // 3)
    src = rng.integers(0, n_loop, n_copy)
    copies = flip_bits(rng, loop_desc[src], min_flips, 40)
    if min_flips == 0:
        copies[0] = loop_desc[src[0]]                         # an exact copy: min_distance == 0, the threshold is 30
    cur_desc = np.concatenate([copies, rng.integers(0, 256, (n_cur - n_copy, 32), dtype=np.uint8)])[rng.permutation(n_cur)]
    loop_cls = rng.integers(-1, n_classes, n_loop).astype(np.int32)
    cur_cls = rng.integers(-1, n_classes, n_cur).astype(np.int32)
    return loop_desc, loop_cls, cur_desc, cur_cls


def check_match(ctx, po, case, expect_min):
    loop_desc, loop_cls, cur_desc, cur_cls = case
    db = sloop.KeyframeDatabase(ctx, keyframes_hint=1)
    db.add(3, EMPTY, np.zeros((5, 32), np.uint8), np.arange(5))
    db.add(8, make_bow(np.random.default_rng(1), 77), loop_desc, loop_cls)
    db.add(9, EMPTY, np.zeros((2, 32), np.uint8), np.arange(2))
    assert db.size() == (3, 77, len(loop_desc) + 7)
    r_pairs, r_md = ref_match(po, loop_desc, loop_cls, cur_desc, cur_cls)
    assert expect_min(r_md), r_md
    pairs, md = db.match_features(8, cur_desc, cur_cls)
    assert md == r_md
    assert np.array_equal(pairs, r_pairs)
    pairs, md = db.match_features(8, cur_desc, cur_cls, cap=len(r_pairs))        # exactly enough
    assert np.array_equal(pairs, r_pairs)
    with pytest.raises(SsxError) as e:                                          # one short
        db.match_features(8, cur_desc, cur_cls, cap=len(r_pairs) - 1)
    assert e.value.status == _lib.SSX_ERR_CAPACITY and e.value.n_pairs == len(r_pairs)
    db.close()
    return len(r_pairs)


@pytest.mark.parametrize("min_flips", [0, 16])
@pytest.mark.parametrize("n_cur", [1, 64, 900])
@pytest.mark.parametrize("n_loop", [1, 63, 257, 1000])
def test_match_screen(ctx, po, n_loop, n_cur, min_flips):
    rng = np.random.default_rng(1000 * n_loop + 10 * n_cur + min_flips)
    case = match_case(rng, n_loop, n_cur, min_flips)
    # min_flips 0: min_distance == 0 and the threshold is 30; min_flips 16: min_distance >= 16 and the threshold is 2 * min_distance
    check_match(ctx, po, case, (lambda md: md == 0) if min_flips == 0 else (lambda md: md >= 16))


def test_match_more_kept_pairs_than_sort_in_lds(ctx, po):
    """5000 loop descriptors all within the screen and class ids wide enough that more than 4096 distinct pairs survive"""
    rng = np.random.default_rng(31)
    cur_desc = rng.integers(0, 256, (900, 32), dtype=np.uint8)
    loop_desc = flip_bits(rng, cur_desc[rng.integers(0, 900, 5000)], 0, 10)
    loop_desc[17] = cur_desc[4]
    loop_cls = rng.integers(-3, 700, 5000).astype(np.int32)
    cur_cls = rng.integers(-3, 300, 900).astype(np.int32)
    n = check_match(ctx, po, (loop_desc, loop_cls, cur_desc, cur_cls), lambda md: md == 0)
    assert 4096 < n < 5000                                    # past the LDS sort, and de-duplication had work


def test_end_to_end_revisit(ctx, po):
    """30 places, a noisy revisit of place 5: DetectLoop finds it, MatchFeatures equals the restatement"""
    voc = make_vocabulary(k=10, L=4, seed=9)
    V = svoc.Vocabulary.from_arrays(ctx, 10, 4, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    prm = po.orb_params(nfeatures=1000, nlevels=4)
    db = sloop.KeyframeDatabase(ctx, keyframes_hint=8)
    entries, stored = [], {}
    for i in range(30):
        img = make_stereo_pair(seed=11 + i, h=200, w=320, n_blobs=400)[0]
        _, desc = po.orb_extract(img, prm=prm)
        cls = (np.arange(len(desc)) % 150).astype(np.int32)   # several pyramid keypoints per feature id
        bow = V.transform(desc)
        db.add(i, bow, desc, cls)
        entries.append((i, bow)); stored[i] = (desc, cls, img)
    rng = np.random.default_rng(0)
    img5 = stored[5][2]
    again = np.clip(img5.astype(np.int16) + rng.integers(-2, 3, img5.shape), 0, 255).astype(np.uint8)
    _, cur_desc = po.orb_extract(again, prm=prm)
    cur_cls = (np.arange(len(cur_desc)) % 150).astype(np.int32)
    query = V.transform(cur_desc)
    found, best_id, best = check_detect(po, db, entries, 60, query, threshold=0.05)
    scores = ref_detect(po, entries, 60, query, 0.05)[3]
    assert found and best_id == 5 and int(np.argmax(scores)) == 5, scores
    pairs, md = db.match_features(best_id, cur_desc, cur_cls)
    r_pairs, r_md = ref_match(po, stored[5][0], stored[5][1], cur_desc, cur_cls)
    assert md == r_md and np.array_equal(pairs, r_pairs) and len(pairs) >= 10
    db.close()
    V.close()


def test_misuse_leaves_the_database_usable(ctx, po):
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    cls = np.arange(40, dtype=np.int32)
    db = sloop.KeyframeDatabase(ctx, keyframes_hint=2)
    entries = [(10, make_bow(rng, 200)), (20, make_bow(rng, 200))]
    db.add(10, entries[0][1], desc, cls)
    db.add(20, entries[1][1])                                 # without descriptors
    for bad_id in (20, 15, -1):                               # ids that do not ascend
        with pytest.raises(SsxError) as e:
            db.add(bad_id, make_bow(rng, 10))
        assert e.value.status == _lib.SSX_ERR_INVALID_ARG
    with pytest.raises(SsxError) as e:                        # word ids that do not ascend
        db.add(30, (np.array([5, 5], np.int32), np.array([0.5, 0.5])))
    assert e.value.status == _lib.SSX_ERR_INVALID_ARG
    with pytest.raises(SsxError) as e:                        # an unknown loop id
        db.match_features(11, desc, cls)
    assert e.value.status == _lib.SSX_ERR_INVALID_ARG
    with pytest.raises(SsxError) as e:                        # a keyframe without descriptors
        db.match_features(20, desc, cls)
    assert e.value.status == _lib.SSX_ERR_INVALID_ARG
    with pytest.raises(SsxError) as e:                        # ssx_bf_match's limit on the train side
        db.match_features(10, np.zeros((65536, 32), np.uint8), np.zeros(65536, np.int32))
    assert e.value.status == _lib.SSX_ERR_UNSUPPORTED
    assert db.size() == (2, 400, 40)                          # nothing of the refused calls was stored
    # no descriptors on one side: zero pairs
    pairs, md = db.match_features(10, np.zeros((0, 32), np.uint8), np.zeros(0, np.int32))
    assert len(pairs) == 0
    db.add(30, make_bow(rng, 5), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32))
    entries.append((30, None))
    pairs, md = db.match_features(30, desc, cls)
    assert len(pairs) == 0
    # and the database still answers
    q = make_bow(rng, 300)
    check_detect(po, db, entries[:2], 40, q)
    pairs, md = db.match_features(10, desc, cls)
    r_pairs, r_md = ref_match(po, desc, cls, desc, cls)
    assert md == r_md == 0 and np.array_equal(pairs, r_pairs) and len(pairs) == 40
    db.close()
