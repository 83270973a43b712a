"""BQ compaction on the MI355X (include/jvector_bq_compact.h through BQGraphBuilder.renumbering / compact) against the yardstick of
tests/bq_compact_yardstick.py.  The renumbering is monotone and every order of this engine breaks ties to the smaller id, so a
compacted builder is the same graph under another naming and everything here is exact: the maps, the rows, the BQ rows; a search over
the new rows returns the old results id for mapped id, score bit for score bit; and inserts and improves on the compacted builder give,
under the extended map, the lists and the adjacency they give on the source.  No tolerance anywhere.  The CPU twin (ABI, the kernel
bodies on the lane emulator) is tests/test_bq_compact_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from bq_builder_yardstick import cluster_data
from bq_compact_yardstick import compact_lists, renumbering
from bq_graph_yardstick import np_encode

MAX_DEGREE, OVERFLOW, BEAM, ALPHA = 8, 1.2, 40, 1.2
N, UPTO, GONE, SPARE = 2000, 1500, 150, 500


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def build(ctx, v, D, max_degree=MAX_DEGREE, overflow=OVERFLOW, beam=BEAM, alpha=ALPHA, batch=128, upto=None):
    """(builder, BQVectors, words, present): nodes 0..upto-1 inserted in order, in batches"""
    n = len(v)
    upto = n if upto is None else upto
    words = np_encode(v, D)
    bq = J.BQVectors(ctx, D, words=words)
    gb = J.BQGraphBuilder(ctx, bq, max_degree, beam, alpha, overflow)
    gb.seed(0)
    lo = 1
    while lo < upto:
        hi = min(upto, lo + min(batch, lo))
        gb.insert_batch(np.arange(lo, hi, dtype=np.int32))
        lo = hi
    present = np.zeros(n, bool)
    present[:upto] = True
    return gb, bq, words, present


def removed(ctx, D, seed=0, gone=None):
    """the build of every case: N rows, UPTO inserted, GONE random nodes (or `gone`) marked and removed.
    (builder, BQVectors, words, v, present afterwards)"""
    v = cluster_data(N, D, 41 + D, dup=60)
    gb, bq, words, present = build(ctx, v, D, upto=UPTO)
    if gone is None:
        gone = np.random.default_rng(seed + D).choice(UPTO, GONE, replace=False)
    gone = np.asarray(gone, np.int32)
    if len(gone):
        gb.mark_deleted(gone)
        assert gb.remove_deleted()["removed"] == len(gone)
        present[gone] = False
    return gb, bq, words, v, present


def sentinel(capacity, W, seed=99):
    return np.random.default_rng(seed).integers(0, 2 ** 63, (capacity, W), dtype=np.int64).astype(np.uint64) | np.uint64(1 << 63)


def destination(ctx, D, capacity):
    pattern = sentinel(capacity, (D + 63) // 64)
    return J.BQVectors(ctx, D, words=pattern), pattern


def rows_of(gb):
    ids, sc, db = gb.working_rows()
    return ids, sc.view(np.int32), db


def same_rows(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert len(bad) == 0, (bad[:5], g[bad[:1]], w[bad[:1]])


def bits_of(mask):
    return np.packbits(np.pad(np.asarray(mask, bool), (0, (-len(mask)) % 64)), bitorder="little").view(np.uint64)


def check_fresh_state(new, live, capacity, entry):
    """rules 7 and 8"""
    assert new.n == capacity and new.entry == entry
    st = new.stats()
    assert (st["search_s"], st["prune_s"], st["backlink_s"]) == (0.0, 0.0, 0.0)
    assert (st["batches"], st["reprunes"], st["inserted"], st["visited"], st["expanded"]) == (0, 0, live, 0, 0)
    assert new.deleted_counts() == (0, 0)
    assert np.array_equal(new.live_bits(), bits_of(np.arange(capacity) < live))


# ------------------------------------------------------------- 1. maps and rows -------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 192])
def test_maps_rows_and_bq_rows_equal_the_yardstick(ctx, D):
    gb, bq, words, v, present = removed(ctx, D)
    live = int(present.sum())
    assert live == UPTO - GONE
    before, entry, inserted = rows_of(gb), gb.entry, gb.stats()["inserted"]
    want_o2n, want_n2o = renumbering(present)
    o2n, n2o = gb.renumbering()
    assert o2n.dtype == n2o.dtype == np.int32 and np.array_equal(o2n, want_o2n) and np.array_equal(n2o, want_n2o)
    capacity = live + SPARE
    dst, pattern = destination(ctx, D, capacity)
    new, o2n, n2o = gb.compact(dst)
    assert np.array_equal(o2n, want_o2n) and np.array_equal(n2o, want_n2o)
    assert new.row_width() == gb.row_width() and new.max_degree == gb.max_degree
    same_rows(rows_of(new), compact_lists(*before, present, capacity))
    got = dst.get()
    assert np.array_equal(got[:live], words[want_n2o])
    assert np.array_equal(got[live:], pattern[live:])                     # rule 3: the rows of future nodes are not written
    check_fresh_state(new, live, capacity, int(want_o2n[entry]))
    # the source is as it was
    same_rows(rows_of(gb), before)
    assert gb.entry == entry and gb.stats()["inserted"] == inserted == live and np.array_equal(bq.get(), words)
    # an id of the new builder does not count as removed: marking one works
    new.mark_deleted(np.array([0, live - 1], np.int32))
    assert new.deleted_counts() == (2, 0)
    for x in (new, gb, dst, bq):
        x.close()


# ---------------------------------------------------------- 2. search isomorphism ----------------------------------------------------------

@pytest.mark.parametrize("D", [64, 192])
def test_a_search_of_the_compacted_rows_is_the_old_search_renamed(ctx, D):
    gb, bq, words, v, present = removed(ctx, D)
    live = int(present.sum())
    dst, _ = destination(ctx, D, live + SPARE)
    new, o2n, n2o = gb.compact(dst)
    rng = np.random.default_rng(7 + D)
    q = (v[rng.choice(N, 32, replace=False)] + 0.05 * rng.standard_normal((32, D))).astype(np.float32)
    old_ids = np.ascontiguousarray(gb.working_rows()[0])
    new_ids = np.ascontiguousarray(new.working_rows()[0][:live])
    g_old = J.GraphIndex(ctx, N, [(None, old_ids)], gb.entry, 0)
    g_new = J.GraphIndex(ctx, live, [(None, new_ids)], new.entry, 0)
    vs_old, vs_new = J.VectorSet(ctx, v), J.VectorSet(ctx, np.ascontiguousarray(v[n2o]))
    for exact in (False, True):
        a = J.BQGraphSearcher(ctx, g_old, bq, vs_old if exact else None).search(q, VSF.DOT_PRODUCT, 10, 40, return_stats=True)
        b = J.BQGraphSearcher(ctx, g_new, dst, vs_new if exact else None).search(q, VSF.DOT_PRODUCT, 10, 40, return_stats=True)
        assert (a[0] >= 0).all() and (b[0] >= 0).all() and (b[0] < live).all()
        assert np.array_equal(n2o[b[0]], a[0])
        assert np.array_equal(b[1].view(np.int32), a[1].view(np.int32))
        assert np.array_equal(b[2], a[2])                                  # visitedCount / expandedCount
    for x in (g_old, g_new, new, gb, dst, bq):
        x.close()


# ------------------------------------------------------- 3. construction isomorphism -------------------------------------------------------

@pytest.mark.parametrize("D", [64, 192])
def test_inserts_and_improves_on_the_compacted_builder_equal_the_sources(ctx, D):
    """a compacted builder is a builder: nothing in the insert path may depend on an id other than through its order"""
    gb, bq, words, v, present = removed(ctx, D)
    live = int(present.sum())
    capacity = live + SPARE
    dst, _ = destination(ctx, D, capacity)
    new, o2n, n2o = gb.compact(dst)
    improve = np.flatnonzero(present)[::4][:300].astype(np.int32)
    assert len(improve) == 300
    # path A: the source goes on
    gb.insert_batch(np.arange(UPTO, UPTO + 200, dtype=np.int32))
    gb.insert_batch(np.arange(UPTO + 200, N, dtype=np.int32))
    gb.improve_batch(improve)
    a_rows = rows_of(gb)
    a_out = gb.finish(np.empty((N, MAX_DEGREE), np.int32))
    # path B: the compacted builder, the new nodes' rows uploaded behind the live ones
    dst.upload(live, words[UPTO:N])
    new.insert_batch(np.arange(live, live + 200, dtype=np.int32))
    new.insert_batch(np.arange(live + 200, live + SPARE, dtype=np.int32))
    new.improve_batch(o2n[improve])
    b_rows = rows_of(new)
    b_out = new.finish(np.empty((capacity, MAX_DEGREE), np.int32))
    # the extended map 1500 + i -> live + i is the sequential renumbering of A's present set
    present_a = present.copy()
    present_a[UPTO:] = True
    ext, ext_inv = renumbering(present_a)
    assert np.array_equal(ext[:UPTO], o2n[:UPTO]) and np.array_equal(ext[UPTO:], live + np.arange(SPARE))
    same_rows(b_rows, compact_lists(*a_rows, present_a, capacity))
    rows = a_out[ext_inv]
    assert np.array_equal(b_out, np.where(rows >= 0, ext[np.maximum(rows, 0)], rows))
    assert new.stats()["inserted"] == gb.stats()["inserted"] == capacity
    for x in (new, gb, dst, bq):
        x.close()


# ------------------------------------------------------------------ 4. edges ------------------------------------------------------------------

def test_nothing_removed_is_the_identity_and_the_builder_grows(ctx):
    D = 64
    gb, bq, words, v, present = removed(ctx, D, gone=[])
    before = rows_of(gb)
    dst, pattern = destination(ctx, D, N + 64)
    new, o2n, n2o = gb.compact(dst)
    assert np.array_equal(o2n[:UPTO], np.arange(UPTO)) and (o2n[UPTO:] == -1).all() and np.array_equal(n2o, np.arange(UPTO))
    got = rows_of(new)
    same_rows(tuple(g[:N] for g in got), before)
    same_rows(got, compact_lists(*before, present, N + 64))
    assert np.array_equal(dst.get(0, UPTO), words[:UPTO]) and np.array_equal(dst.get(UPTO), pattern[UPTO:])
    check_fresh_state(new, UPTO, N + 64, gb.entry)
    # with every row inserted the whole builder moves, and the capacity beyond n is new room
    gb.insert_batch(np.arange(UPTO, N, dtype=np.int32))
    full = rows_of(gb)
    dst2, _ = destination(ctx, D, N + 64)
    new2, o2n, n2o = gb.compact(dst2)
    assert np.array_equal(o2n, np.arange(N)) and np.array_equal(n2o, np.arange(N))
    same_rows(rows_of(new2), compact_lists(*full, np.ones(N, bool), N + 64))
    dst2.upload(N, words[:64])
    new2.insert_batch(np.arange(N, N + 64, dtype=np.int32))
    assert new2.stats()["inserted"] == N + 64
    for x in (new2, new, gb, dst2, dst, bq):
        x.close()


def test_the_entry_node_removed_first_gives_entry_zero(ctx):
    D = 64
    gb, bq, words, v, present = removed(ctx, D, gone=[0, 5, 700])
    assert gb.entry == 1                                   # deletion rule 8: the smallest live id
    dst, _ = destination(ctx, D, UPTO)
    new, o2n, n2o = gb.compact(dst)
    assert new.entry == 0 and o2n[1] == 0 and o2n[0] == -1 and n2o[0] == 1
    same_rows(rows_of(new), compact_lists(*rows_of(gb), present, UPTO))
    for x in (new, gb, dst, bq):
        x.close()


def test_an_empty_graph_compacts_to_a_fresh_builder(ctx):
    n, D = 65, 64
    v = cluster_data(n, D, 3)
    gb, bq, words, present = build(ctx, v, D, 4, 1.5, beam=20, upto=40)
    gb.mark_deleted(np.arange(40, dtype=np.int32))
    gb.remove_deleted()
    dst, pattern = destination(ctx, D, n)
    new, o2n, n2o = gb.compact(dst)
    assert (o2n == -1).all() and len(o2n) == n and len(n2o) == 0
    ids, sc, db = rows_of(new)
    assert ids.shape == (n, gb.row_width()) and (ids == -1).all() and (sc == 0).all() and (db == 0).all()
    assert np.array_equal(dst.get(), pattern)
    check_fresh_state(new, 0, n, -1)
    dst.upload(0, words)
    new.seed(0)                                             # id 0 was removed from the source; here it is a fresh id
    new.insert_batch(np.arange(1, n, dtype=np.int32))
    assert new.entry == 0 and new.stats()["inserted"] == n
    assert (new.working_rows()[0][:, 0] >= 0).all()
    for x in (new, gb, dst, bq):
        x.close()


def test_forty_thousand_nodes_rank_over_three_scan_blocks(ctx):
    n, D = 40_000, 64
    v = cluster_data(n, D, 12, clusters=12)
    gb, bq, words, present = build(ctx, v, D, beam=20, batch=4096)
    gone = np.random.default_rng(4).choice(n, 4000, replace=False).astype(np.int32)
    gb.mark_deleted(gone)
    assert gb.remove_deleted()["removed"] == 4000
    present[gone] = False
    want_o2n, want_n2o = renumbering(present)
    o2n, n2o = gb.renumbering()
    assert np.array_equal(o2n, want_o2n) and np.array_equal(n2o, want_n2o)
    before = rows_of(gb)
    dst, pattern = destination(ctx, D, n - 4000 + 100)
    new, o2n, n2o = gb.compact(dst)
    assert np.array_equal(o2n, want_o2n) and np.array_equal(n2o, want_n2o)
    same_rows(rows_of(new), compact_lists(*before, present, n - 4000 + 100))
    got = dst.get()
    assert np.array_equal(got[:n - 4000], words[want_n2o]) and np.array_equal(got[n - 4000:], pattern[n - 4000:])
    for x in (new, gb, dst, bq):
        x.close()


# ------------------------------------------------------------------ 5. errors ------------------------------------------------------------------

def test_refused_calls_create_nothing_and_change_nothing(ctx):
    D = 64
    gb, bq, words, v, present = removed(ctx, D)
    live = int(present.sum())
    before, entry, stats, counts = rows_of(gb), gb.entry, gb.stats(), gb.deleted_counts()
    good, good_pat = destination(ctx, D, live + 10)
    other_d, other_pat = destination(ctx, 128, live + 10)
    small, small_pat = destination(ctx, D, live - 1)

    def unchanged():
        same_rows(rows_of(gb), before)
        assert gb.entry == entry and gb.stats() == stats and np.array_equal(bq.get(), words)
        for d, pat in ((good, good_pat), (other_d, other_pat), (small, small_pat)):
            assert np.array_equal(d.get(), pat)

    with pytest.raises(ValueError, match="dimension"):
        gb.compact(other_d)
    unchanged()
    with pytest.raises(ValueError, match="own"):
        gb.compact(bq)
    unchanged()
    with pytest.raises(ValueError, match="%d destination rows for %d nodes" % (live - 1, live)):
        gb.compact(small)
    unchanged()
    assert gb.deleted_counts() == counts
    # pending marks: refused until remove_deleted has run
    some = np.flatnonzero(present)[10:13].astype(np.int32)
    gb.mark_deleted(some)
    with pytest.raises(ValueError, match="marked"):
        gb.compact(good)
    unchanged()
    assert gb.deleted_counts() == (3, counts[1])
    o2n, n2o = gb.renumbering()                              # a marked node is still a node of the graph
    assert np.array_equal(o2n, renumbering(present)[0])
    gb.remove_deleted()
    present[some] = False
    new, o2n, n2o = gb.compact(good)
    assert np.array_equal(o2n, renumbering(present)[0]) and new.stats()["inserted"] == live - 3
    for x in (new, gb, good, other_d, small, bq):
        x.close()


# --------------------------------------------------------------- 6. determinism ---------------------------------------------------------------

def test_two_compactions_are_byte_identical(ctx):
    D = 192
    gb, bq, words, v, present = removed(ctx, D)
    live = int(present.sum())
    runs = []
    for _ in range(2):
        dst, _ = destination(ctx, D, live + SPARE)
        new, o2n, n2o = gb.compact(dst)
        runs.append((o2n, n2o, *rows_of(new), dst.get()))
        new.close()
        dst.close()
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    gb.close()
    bq.close()
