"""Deleting nodes from an exact-score builder graph on the MI355X (include/jvector_exact_delete.h through ExactGraphBuilder.mark_deleted /
remove_deleted / live_bits / deleted_counts / entry).  The yardstick is bq_delete_yardstick's merged_lists / remove_deleted restated with
the two score sources swapped: candidates are scored by oracle.compare_many (never the engine), the prune is exact_build_ref's
retain_diverse over oracle pair scores.  Every comparison is np.array_equal on ids, score BITS, diverseBefore, entry, counts and live
bits: there is no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from bq_delete_yardstick import NodeArray, fallback_draws, merge
from exact_build_ref import Pairs, clustered, retain_diverse
from oracle import oracle as O


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def rows_with_copies(seed, N, D, centres=20):
    """unit rows around a few centres, a third of them copies of other rows: equal scores, and the merge's pair rule, are exercised"""
    v = clustered(seed, N, D, centres)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rng = np.random.default_rng(seed)
    dst = rng.choice(N, N // 3, replace=False)
    v[dst] = v[rng.choice(np.setdiff1d(np.arange(N), dst), len(dst))]
    return v


def build(ctx, v, vsf, max_degree, overflow, beam=20, alpha=1.2, batch=64, upto=None):
    upto = len(v) if upto is None else upto
    vs = J.VectorSet(ctx, v)
    gb = J.ExactGraphBuilder(ctx, vs, vsf, max_degree, beam, alpha, overflow)
    gb.seed(0)
    lo = 1
    while lo < upto:
        hi = min(upto, lo + min(batch, lo))
        gb.insert_batch(np.arange(lo, hi, dtype=np.int32))
        lo = hi
    present = np.zeros(len(v), bool)
    present[:upto] = True
    return gb, vs, present


def mask(N, ids):
    m = np.zeros(N, bool)
    m[np.asarray(ids, np.int64)] = True
    return m


def bits_of(m):
    return np.packbits(np.pad(m, (0, (-len(m)) % 64)), bitorder="little").view(np.uint64)


def merged_lists(vsf, v, ids, sc, present, marked, max_degree, seed=0, only=None):
    """rules 1 - 4 and 7 per affected node, ascending: dict(node, ids, scores, candidates, raw two-hop entries, fallback)"""
    out = []
    for i in (range(len(ids)) if only is None else only):
        row = [(int(k), s) for k, s in zip(ids[i], sc[i]) if k >= 0]
        if not present[i] or marked[i] or not any(marked[k] for k, _ in row):
            continue
        raw = [int(k) for j, _ in row if marked[j] for k in ids[j] if k >= 0 and k != i and not marked[k]]
        order = sorted(set(raw))
        fallback = len(order) == 0
        if fallback:
            order = sorted(fallback_draws(i, len(ids), max_degree, present, marked, seed))
        cand, live = NodeArray(), NodeArray()
        if order:
            for k, x in zip(order, O.compare_many(int(vsf), v[i], v[order])):
                cand.insert_sorted(k, x)
        for k, s in row:
            if not marked[k]:
                live.add_in_order(k, s)
        m = merge(live, cand)
        out.append(dict(node=i, ids=np.asarray(m.nodes, np.int32), scores=np.asarray(m.scores, np.float32), candidates=cand.size(), raw=len(raw),
                        fallback=fallback))
    return out


def prune_into(vsf, v, lst_ids, lst_sc, before, max_degree, alpha):
    """retainDiverse(list, before): the selected (ids, scores)"""
    n = len(lst_ids)
    (sel, _, _), _ = retain_diverse([Pairs(vsf, v, lst_ids)], lst_ids[None, :], lst_sc[None, :], max_degree, alpha, np.array([n], np.int32),
                                    np.array([before], np.int32))
    pos = sel[0][sel[0] >= 0]
    return lst_ids[pos], lst_sc[pos]


def remove_deleted(vsf, v, ids, sc, db, present, marked, max_degree, alpha, seed, entry):
    ids, sc, db, present = ids.copy(), sc.copy(), db.copy(), present.copy()
    lists = merged_lists(vsf, v, ids, sc, present, marked, max_degree, seed)
    for m in lists:
        i = m["node"]
        ki, ks = prune_into(vsf, v, m["ids"], m["scores"], 0, max_degree, alpha)
        ids[i], sc[i], db[i] = -1, 0.0, len(ki)
        ids[i, :len(ki)], sc[i, :len(ki)] = ki, ks
    ids[marked], sc[marked], db[marked] = -1, 0.0, 0
    present[marked] = False
    if entry >= 0 and marked[entry]:
        entry = int(np.flatnonzero(present)[0]) if present.any() else -1
    counts = dict(removed=int(marked.sum()), rewritten=len(lists), candidates=sum(m["candidates"] for m in lists),
                  fallback=sum(m["fallback"] for m in lists))
    return (ids, sc, db), present, entry, counts, lists


def same_lists(got, want):
    assert np.array_equal(got[0], want[0]), np.flatnonzero((got[0] != want[0]).any(axis=1))[:5]
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)) and np.array_equal(got[2], want[2])


def round_against_the_yardstick(gb, vsf, v, present, marked, max_degree, alpha, seed=0):
    """mark + remove, compared with the yardstick applied to the lists read before the call; returns (present afterwards, lists)"""
    before, entry = gb.working_rows(), gb.entry
    want, want_present, want_entry, counts, lists = remove_deleted(vsf, v, *before, present, marked, max_degree, alpha, seed, entry)
    gb.mark_deleted(np.flatnonzero(marked).astype(np.int32))
    assert gb.deleted_counts()[0] == int(marked.sum())
    assert gb.remove_deleted(seed) == counts
    got = gb.working_rows()
    same_lists(got, want)
    assert gb.entry == want_entry and gb.deleted_counts()[0] == 0 and gb.stats()["inserted"] == int(want_present.sum())
    assert np.array_equal(gb.live_bits(), bits_of(want_present))
    untouched = np.setdiff1d(np.flatnonzero(present & ~marked), [m["node"] for m in lists])
    same_lists([a[untouched] for a in got], [a[untouched] for a in before])
    assert want_present[got[0][got[0] >= 0]].all()                          # no row names a removed id
    return want_present, lists


@pytest.mark.parametrize("D,max_degree,overflow", [(24, 8, 1.2), (65, 8, 1.2), (128, 16, 1.25), (260, 8, 1.0)])
@pytest.mark.parametrize("vsf", [VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE])
def test_remove_deleted_equals_the_yardstick_over_chained_rounds(ctx, vsf, D, max_degree, overflow):
    """the tile path with one chunk (24) and with two (128), the lane path at an odd D (65, 260 = 4 x 65), working rows of 20; four rounds
    on one builder: one node, 10 % of the repaired graph, a set with the entry, 50 %; then finish against enforceDegree"""
    N, alpha = 300, 1.2
    v = rows_with_copies(D + max_degree, N, D)
    gb, vs, present = build(ctx, v, vsf, max_degree, overflow)
    cap = J.ExactBuildScorer(ctx, None, vs, vsf).max_candidates(max_degree)
    rng = np.random.default_rng(D)
    live = lambda: np.flatnonzero(present)[1:]                              # (node 0, the entry, has a round of its own)
    sets = [lambda: [N // 2], lambda: rng.choice(live(), N // 10, replace=False),
            lambda: np.append(rng.choice(live(), 20, replace=False), 0), lambda: rng.choice(np.flatnonzero(present), int(present.sum()) // 2, replace=False)]
    dup_seen = False
    for pick in sets:
        present, lists = round_against_the_yardstick(gb, vsf, v, present, mask(N, pick()), max_degree, alpha)
        assert lists and not any(m["fallback"] for m in lists) and max(len(m["ids"]) for m in lists) <= cap
        dup_seen |= any(m["raw"] > m["candidates"] for m in lists)
    assert dup_seen                                                         # duplicates were there to drop before the scoring
    assert gb.entry == int(np.flatnonzero(present)[0]) > 0
    ids, sc, db = gb.working_rows()
    want = np.full((N, max_degree), -1, np.int32)
    for i in range(N):
        n = int((ids[i] >= 0).sum())
        keep = ids[i, :n] if n <= max_degree else prune_into(vsf, v, ids[i, :n], sc[i, :n], db[i], max_degree, alpha)[0]
        want[i, :len(keep)] = keep
    assert np.array_equal(gb.finish(np.empty((N, max_degree), np.int32)), want)
    gb.close()
    vs.close()


@pytest.mark.parametrize("keep", [1, 3])
def test_fallback_draws_follow_the_seed(ctx, keep):
    """all but one node marked: no candidate, no draw, an empty row; all but three: the draws decide.  The same seed twice is byte-identical."""
    N, D, max_degree, vsf = 200, 24, 8, VSF.DOT_PRODUCT
    v = rows_with_copies(9, N, D)
    marked = mask(N, np.random.default_rng(keep).permutation(N)[keep:])
    rows = []
    for _ in range(2):
        gb, vs, present = build(ctx, v, vsf, max_degree, 1.2)
        _, lists = round_against_the_yardstick(gb, vsf, v, present, marked, max_degree, 1.2, seed=5)
        assert any(m["fallback"] for m in lists) and len(lists) <= keep
        rows.append(gb.working_rows())
        gb.close()
        vs.close()
    same_lists(rows[0], rows[1])


def test_a_list_beyond_the_prune_capacity_is_refused_and_nothing_changes(ctx):
    N, D, max_degree, vsf = 1000, 8, 64, VSF.EUCLIDEAN                     # (768 rows: the longest list is 374, under the 512 the prune holds)
    v = rows_with_copies(17, N, D)
    gb, vs, present = build(ctx, v, vsf, max_degree, 1.0, beam=100, batch=256)
    cap = J.ExactBuildScorer(ctx, None, vs, vsf).max_candidates(max_degree)
    ids, sc, db = gb.working_rows()
    two_hop = [len(np.unique(ids[ids[i][ids[i] >= 0]])) for i in range(N)]
    node = int(np.argmax(two_hop))
    one = ids[node][ids[node] >= 0]
    marked = mask(N, one)
    longest = len(merged_lists(vsf, v, ids, sc, present, marked, max_degree, only=[node])[0]["ids"])
    assert longest > cap, (node, longest, cap)                              # the precondition
    gb.mark_deleted(one.astype(np.int32))
    entry = gb.entry
    with pytest.raises(UnsupportedError, match=rf"would merge \d+ .* above the {cap} "):
        gb.remove_deleted()
    same_lists(gb.working_rows(), (ids, sc, db))
    assert gb.deleted_counts() == (len(one), 0) and gb.entry == entry and gb.stats()["inserted"] == N
    assert np.array_equal(gb.live_bits(), bits_of(present & ~marked))
    gb.close()
    vs.close()


def test_errors_live_bits_and_the_life_of_an_id(ctx):
    N, D, max_degree, upto, vsf = 300, 24, 8, 200, VSF.DOT_PRODUCT
    v = rows_with_copies(23, N, D)
    gb, vs, present = build(ctx, v, vsf, max_degree, 1.2, upto=upto)
    before = gb.working_rows()
    assert gb.remove_deleted() == dict(removed=0, rewritten=0, candidates=0, fallback=0)
    for bad in ([upto], [N], [-1], [5, upto + 3]):                          # never inserted, outside the rows
        with pytest.raises(ValueError):
            gb.mark_deleted(np.array(bad, np.int32))
    same_lists(gb.working_rows(), before)
    assert gb.deleted_counts() == (0, 0) and np.array_equal(gb.live_bits(), bits_of(present))
    rng = np.random.default_rng(2)
    gone = rng.choice(np.arange(1, upto), 40, replace=False).astype(np.int32)
    marked = mask(N, gone)
    gb.mark_deleted(gone)
    gb.mark_deleted(gone[:10])                                              # marking twice is fine
    assert gb.deleted_counts() == (40, 0)
    bits = gb.live_bits()
    assert np.array_equal(bits, bits_of(present & ~marked))
    # ExactGraphSearcher packs a bool filter into these very words: the marked nodes are hidden before the removal ...
    accept = np.unpackbits(bits.view(np.uint8), bitorder="little")[:N].astype(bool)
    q = v[gone[:16]]
    g = J.GraphIndex(ctx, N, [(None, np.ascontiguousarray(before[0]))], gb.entry, 0)
    searcher = J.ExactGraphSearcher(ctx, g, vs)
    assert marked[searcher.search(q, vsf, 5, 30)[0]].any()
    hidden = searcher.search(q, vsf, 5, 30, accept=accept)[0]
    assert (hidden >= 0).all() and not marked[hidden].any()
    g.close()
    gb.remove_deleted()
    # ... and gone from an unfiltered search after it
    g = J.GraphIndex(ctx, N, [(None, np.ascontiguousarray(gb.working_rows()[0]))], gb.entry, 0)
    after = J.ExactGraphSearcher(ctx, g, vs).search(q, vsf, 5, 30)[0]
    assert (after >= 0).all() and not marked[after].any()
    g.close()
    for call in (gb.mark_deleted, gb.insert_batch, gb.improve_batch):      # a removed id is never reused
        with pytest.raises(ValueError, match="removed"):
            call(gone[:1])
    gb.insert_batch(np.arange(upto, N, dtype=np.int32))                     # an insert after a removal works
    present[upto:] = True
    assert gb.stats()["inserted"] == N - 40 and np.array_equal(gb.live_bits(), bits_of(present & ~marked))
    ids = gb.working_rows()[0]
    assert (ids[upto:] >= 0).any(axis=1).all() and not marked[ids[ids >= 0]].any()
    # an emptied graph has entry -1 and can be seeded again, not with a removed id
    gb.mark_deleted(np.flatnonzero(present & ~marked).astype(np.int32))
    assert gb.remove_deleted()["removed"] == N - 40
    assert gb.entry == -1 and gb.stats()["inserted"] == 0 and not gb.live_bits().any() and (gb.working_rows()[0] == -1).all()
    gb.close()
    vs.close()
    gb, vs, _ = build(ctx, v, vsf, max_degree, 1.2, upto=40)
    gb.mark_deleted(np.arange(40, dtype=np.int32))
    gb.remove_deleted()
    with pytest.raises(ValueError, match="removed"):
        gb.seed(3)
    gb.seed(40)
    gb.insert_batch(np.arange(41, 60, dtype=np.int32))
    assert gb.entry == 40 and gb.stats()["inserted"] == 20
    gb.close()
    vs.close()
