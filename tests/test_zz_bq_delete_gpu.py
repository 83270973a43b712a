"""BQ deletions on the MI355X (include/jvector_bq_delete.h through BQGraphBuilder.mark_deleted / remove_deleted / live_bits) against the
yardstick of tests/bq_delete_yardstick.py, the literal restatement of removeDeletedNodes: after remove_deleted the working lists — ids,
order, score bits, diverseBefore marks — the entry, the counts and the adjacency after finish equal the yardstick's byte for byte.  The
rest is structural (untouched rows, no dangling reference, blank removed rows), the fallback, the refusal, the errors, live_bits as a
search filter, inserts after a removal, and the recall of a repaired graph against a rebuilt one.  The CPU twin (ABI, the kernel bodies
on the lane emulator) is tests/test_bq_delete_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from bq_build_yardstick import retain_diverse
from bq_builder_yardstick import cluster_data
from bq_delete_yardstick import merged_lists, remove_deleted
from bq_graph_yardstick import np_encode


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def build(ctx, v, D, max_degree, overflow, beam=40, alpha=1.2, batch=128, upto=None):
    """(builder, BQVectors, words, present): nodes 0..upto-1 inserted in order, in batches"""
    N = len(v)
    upto = N if upto is None else upto
    words = np_encode(v, D)
    bq = J.BQVectors(ctx, D, words=words)
    gb = J.BQGraphBuilder(ctx, bq, max_degree, beam, alpha, overflow)
    gb.seed(0)
    lo = 1
    while lo < upto:
        hi = min(upto, lo + min(batch, lo))
        gb.insert_batch(np.arange(lo, hi, dtype=np.int32))
        lo = hi
    present = np.zeros(N, bool)
    present[:upto] = True
    return gb, bq, words, present


def mask(N, ids):
    m = np.zeros(N, bool)
    m[np.asarray(ids, np.int64)] = True
    return m


def same_lists(got, want):
    (gi, gs, gd), (wi, ws, wd) = got, want
    bad = np.flatnonzero((gi != wi).any(axis=1))
    assert len(bad) == 0, (bad[:5], gi[bad[:1]], wi[bad[:1]])
    assert np.array_equal(gs.view(np.int32), ws.view(np.int32))
    assert np.array_equal(gd, wd)


def check_structure(ids, sc, db, present, removed):
    """no row names a removed node, itself, -1 in the middle or an id twice; removed rows are blank"""
    N = len(ids)
    deg = (ids >= 0).sum(axis=1)
    assert all((ids[i, :deg[i]] >= 0).all() and (ids[i, deg[i]:] == -1).all() for i in range(N))
    assert not (ids == np.arange(N)[:, None]).any()
    srt = np.sort(ids, axis=1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()
    named = ids[ids >= 0]
    assert not removed[named].any() and present[named].all()
    assert (ids[removed] == -1).all() and (sc[removed] == 0).all() and (db[removed] == 0).all()


def remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, marked, cap, seed=0, allow_fallback=False):
    """one mark + remove round against the yardstick; returns (present afterwards, yardstick info)"""
    before = gb.working_rows()
    entry = gb.entry
    # `marked` may be a list of sets: the case is the first one that meets the preconditions on the graph as the device built it
    for marked in (marked if isinstance(marked, list) else [marked]):
        want_ids, want_sc, want_db, want_present, want_entry, info = remove_deleted(words, D, *before, present, marked, max_degree, alpha, seed, entry)
        if info["max_len"] <= cap and (allow_fallback or info["counts4"][3] == 0):
            break
    # the preconditions of the case: within capacity, and (unless the case is about it) no fallback
    assert info["max_len"] <= cap, info["max_len"]
    assert allow_fallback or info["counts4"][3] == 0
    gb.mark_deleted(np.flatnonzero(marked).astype(np.int32))
    assert gb.deleted_counts()[0] == int(marked.sum())
    counts = gb.remove_deleted(seed)
    got = gb.working_rows()
    same_lists(got, (want_ids, want_sc, want_db))
    assert (counts["removed"], counts["rewritten"], counts["candidates"], counts["fallback"]) == info["counts4"]
    assert gb.entry == want_entry and gb.deleted_counts()[0] == 0
    assert gb.stats()["inserted"] == int(want_present.sum())
    # untouched rows: a live node without a marked neighbour keeps its ids, score bits and mark
    untouched = np.setdiff1d(np.flatnonzero(present & ~marked), info["affected"])
    assert np.array_equal(got[0][untouched], before[0][untouched]) and np.array_equal(got[2][untouched], before[2][untouched])
    assert np.array_equal(got[1][untouched].view(np.int32), before[1][untouched].view(np.int32))
    check_structure(*got, want_present, ~want_present)   # (not in the graph: removed now or earlier, or never inserted)
    return want_present, info


def finish_yardstick(words, D, ids, sc, db, max_degree, alpha):
    """enforceDegree on every row: retainDiverse(row, diverseBefore) where the row is longer than maxDegree"""
    out = np.full((len(ids), max_degree), -1, np.int32)
    for i in range(len(ids)):
        n = int((ids[i] >= 0).sum())
        if n <= max_degree:
            out[i, :n] = ids[i, :n]
            continue
        sel, _, _ = retain_diverse(words, D, ids[i:i + 1], sc[i:i + 1], max_degree, alpha, cand_count=np.array([n], np.int32), diverse_before=db[i:i + 1])
        pos = sel[0][sel[0] >= 0]
        out[i, :len(pos)] = ids[i, pos]
    return out


# ------------------------------------------------------ byte parity with the yardstick ------------------------------------------------------

@pytest.mark.parametrize("max_degree,overflow", [(8, 1.2), (16, 1.25)])
@pytest.mark.parametrize("D", [64, 192, 768])
def test_remove_deleted_equals_the_yardstick(ctx, D, max_degree, overflow):
    """one build, four rounds on it: a single node; 10 % (a second round on an already repaired graph); a set with the entry node, whose
    successor must be the yardstick's; 50 %.  Then the adjacency after finish."""
    N, alpha = 2000, 1.2
    v = cluster_data(N, D, 31 + D + max_degree, dup=60)
    gb, bq, words, present = build(ctx, v, D, max_degree, overflow)
    cap = J.BQBuildScorer(ctx, None, bq).max_candidates(max_degree)
    rng = np.random.default_rng(D + max_degree)
    present, info = remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, mask(N, [N // 2]), cap)
    assert info["counts4"][1] >= 1
    tenths = [mask(N, rng.choice(np.flatnonzero(present)[1:], N // 10, replace=False)) for _ in range(6)]   # (node 0, the entry, stays: it has a round of its own)
    present, info = remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, tenths, cap)
    assert info["counts4"][1] > N // 10
    assert gb.entry == 0
    with_entry = np.concatenate([[0], rng.choice(np.flatnonzero(present)[1:], 20, replace=False)])
    present, info = remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, mask(N, with_entry), cap)
    assert gb.entry == int(np.flatnonzero(present)[0]) > 0
    halves = [mask(N, rng.choice(np.flatnonzero(present), int(present.sum()) // 2, replace=False)) for _ in range(6)]
    present, info = remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, halves, cap)
    assert info["counts4"][1] > N // 4 and info["max_len"] > gb.row_width()
    ids, sc, db = gb.working_rows()
    out = gb.finish(np.empty((N, max_degree), np.int32))
    assert np.array_equal(out, finish_yardstick(words, D, ids, sc, db, max_degree, alpha))
    assert gb.deleted_counts() == (0, N - int(present.sum()))
    gb.close()
    bq.close()


# ------------------------------------------------------------------ fallback ------------------------------------------------------------------

def test_fallback_when_the_whole_two_hop_neighbourhood_is_marked(ctx):
    N, D, max_degree, alpha = 2000, 64, 8, 1.2
    v = cluster_data(N, D, 5, dup=40)
    rows = {}
    for run, seed in enumerate((3, 3, 4)):
        gb, bq, words, present = build(ctx, v, D, max_degree, 1.2)
        ids, sc, db = gb.working_rows()
        node = 777
        one = ids[node][ids[node] >= 0]
        two = np.unique(ids[one][ids[one] >= 0])
        marked = mask(N, np.setdiff1d(np.concatenate([one, two]), [node]))
        lists = {m["node"]: m for m in merged_lists(words, D, ids, sc, present, marked, max_degree, seed)}
        assert lists[node]["fallback"] and lists[node]["candidates"] >= 1      # the yardstick: no candidate, so the draws decide
        cap = J.BQBuildScorer(ctx, None, bq).max_candidates(max_degree)
        present, info = remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, marked, cap, seed=seed, allow_fallback=True)
        assert node in info["fallback_nodes"]
        got = gb.working_rows()
        row = got[0][node][got[0][node] >= 0]
        assert len(row) >= 1 and present[row].all() and node not in row and len(set(row.tolist())) == len(row)
        rows[run] = (got[0].copy(), got[1].copy(), got[2].copy())
        gb.close()
        bq.close()
    same_lists(rows[0], rows[1])                                               # the same seed: byte-identical
    # another seed: each run above equals the yardstick under its own seed, so the rows differ exactly where the yardstick's do
    print("fallback row, seed 3:", rows[0][0][777], "seed 4:", rows[2][0][777])


# ------------------------------------------------------------------- refusal -------------------------------------------------------------------

def test_a_list_beyond_the_prune_capacity_is_refused_and_nothing_changes(ctx):
    N, D, max_degree, alpha = 2000, 768, 64, 1.2
    v = cluster_data(N, D, 17, clusters=2)
    gb, bq, words, present = build(ctx, v, D, max_degree, 1.0, beam=100, batch=256)
    cap = J.BQBuildScorer(ctx, None, bq).max_candidates(max_degree)
    assert cap == 571
    ids, sc, db = gb.working_rows()
    # chosen on the CPU: the node whose neighbours' rows name the most distinct nodes; all its neighbours are marked
    best, best_n = -1, 0
    for i in range(0, N, 7):
        one = ids[i][ids[i] >= 0]
        k = len(np.setdiff1d(np.unique(ids[one][ids[one] >= 0]), np.append(one, i)))
        if k > best_n:
            best, best_n = i, k
    one = ids[best][ids[best] >= 0]
    marked = mask(N, one)
    lens = {m["node"]: len(m["ids"]) for m in merged_lists(words, D, ids, sc, present, marked, max_degree)}
    assert max(lens.values()) > cap, (best, best_n, max(lens.values()))       # the precondition
    gb.mark_deleted(one.astype(np.int32))
    entry = gb.entry
    with pytest.raises(UnsupportedError, match=r"node \d+ would merge \d+ .* above the 571"):
        gb.remove_deleted()
    same_lists(gb.working_rows(), (ids, sc, db))
    assert gb.deleted_counts() == (len(one), 0) and gb.entry == entry and gb.stats()["inserted"] == N
    assert np.array_equal(gb.live_bits(), np.packbits(np.pad(present & ~marked, (0, (-N) % 64)), bitorder="little").view(np.uint64))
    gb.close()
    bq.close()
    # the same marks in two halves, where the yardstick says each half fits (if one does not, this sub-step has no case and is skipped)
    gb, bq, words, present = build(ctx, v, D, max_degree, 1.0, beam=100, batch=256)
    for half in (one[:len(one) // 2], one[len(one) // 2:]):
        rows = gb.working_rows()
        m = mask(N, half)
        fits = max(len(x["ids"]) for x in merged_lists(words, D, *rows[:2], present, m, max_degree)) <= cap
        print("half of", len(half), "marks fits:", fits)
        if not fits:
            break
        present, _ = remove_and_compare(ctx, gb, words, D, max_degree, alpha, present, m, cap, allow_fallback=True)
    gb.close()
    bq.close()


# ---------------------------------------------------- errors, live_bits, inserts after a removal ----------------------------------------------------

def test_errors_live_bits_and_inserts_after_a_removal(ctx):
    N, D, max_degree, alpha, upto = 2000, 64, 8, 1.2, 1500
    v = cluster_data(N, D, 23, dup=30)
    gb, bq, words, present = build(ctx, v, D, max_degree, 1.2, upto=upto)
    before = gb.working_rows()
    assert gb.remove_deleted() == dict(removed=0, rewritten=0, candidates=0, fallback=0)       # nothing marked: nothing changes
    same_lists(gb.working_rows(), before)
    for bad in ([upto], [N], [-1], [5, upto + 3]):                                                # never inserted, outside the rows
        with pytest.raises(ValueError):
            gb.mark_deleted(np.array(bad, np.int32))
    assert gb.deleted_counts() == (0, 0)
    rng = np.random.default_rng(2)
    gone = rng.choice(upto, 150, replace=False).astype(np.int32)
    gb.mark_deleted(gone)
    gb.mark_deleted(gone[:10])                                                                    # marking twice is not an error
    assert gb.deleted_counts() == (150, 0)
    marked = mask(N, gone)
    # before the removal: live_bits as accept_bits hides the marked nodes
    bits = gb.live_bits()
    assert np.array_equal(bits, np.packbits(np.pad(present & ~marked, (0, (-N) % 64)), bitorder="little").view(np.uint64))
    ids, _, _ = gb.working_rows()
    g = J.GraphIndex(ctx, N, [(None, np.ascontiguousarray(ids))], gb.entry, 0)
    q = (v[gone[:32]] + 0.05 * rng.standard_normal((32, D))).astype(np.float32)                   # queries AT marked nodes
    searcher = J.BQGraphSearcher(ctx, g, bq)
    plain, _ = searcher.search(q, VSF.DOT_PRODUCT, 10, 40)
    assert marked[plain[plain >= 0]].any()
    hidden, _ = searcher.search(q, VSF.DOT_PRODUCT, 10, 40, accept_bits=bits)
    assert (hidden >= 0).all() and not marked[hidden].any()
    g.close()
    cap = J.BQBuildScorer(ctx, None, bq).max_candidates(max_degree)
    gb2, bq2, _, _ = build(ctx, v, D, max_degree, 1.2, upto=upto)                                 # the same graph, for the yardstick round
    present, _ = remove_and_compare(ctx, gb2, words, D, max_degree, alpha, present, marked, cap, allow_fallback=True)
    gb2.close()
    bq2.close()
    gb.remove_deleted()
    assert gb.deleted_counts() == (0, 150)
    # after the removal: an unfiltered search returns no removed id
    ids, _, _ = gb.working_rows()
    g = J.GraphIndex(ctx, N, [(None, np.ascontiguousarray(ids))], gb.entry, 0)
    after, _ = J.BQGraphSearcher(ctx, g, bq).search(q, VSF.DOT_PRODUCT, 10, 40)
    assert (after >= 0).all() and not marked[after].any()
    g.close()
    with pytest.raises(ValueError, match="removed"):
        gb.mark_deleted(gone[:1])                                                                 # already removed
    with pytest.raises(ValueError, match="removed"):
        gb.insert_batch(np.array([upto, int(gone[0])], np.int32))
    with pytest.raises(ValueError, match="removed"):
        gb.improve_batch(gone[:2])
    # inserts after the removal: the structural checks of the builder test, and nothing removed comes back
    gb.insert_batch(np.arange(upto, upto + 200, dtype=np.int32))
    gb.insert_batch(np.arange(upto + 200, N, dtype=np.int32))
    gb.improve_batch(np.setdiff1d(np.arange(N, dtype=np.int32), gone)[:300])
    present[upto:] = True
    assert gb.stats()["inserted"] == N - 150
    ids, sc, db = gb.working_rows()
    check_structure(ids, sc, db, present, marked)
    out = gb.finish(np.empty((N, max_degree), np.int32))
    deg = (out >= 0).sum(axis=1)
    assert deg.max() <= max_degree and deg[present].min() >= 1 and (deg[marked] == 0).all()
    assert all((out[i, :deg[i]] >= 0).all() and (out[i, deg[i]:] == -1).all() for i in range(N))
    assert not marked[out[out >= 0]].any() and not (out == np.arange(N)[:, None]).any()
    gb.close()
    bq.close()


def test_removing_everything_empties_the_graph_and_it_can_be_seeded_again(ctx):
    N, D = 65, 64
    v = cluster_data(N, D, 3)
    gb, bq, words, present = build(ctx, v, D, 4, 1.5, beam=20, upto=40)
    gb.mark_deleted(np.arange(40, dtype=np.int32))
    assert gb.remove_deleted() == dict(removed=40, rewritten=0, candidates=0, fallback=0)
    assert gb.entry == -1 and gb.stats()["inserted"] == 0 and not gb.live_bits().any()
    ids, sc, db = gb.working_rows()
    assert (ids == -1).all() and (sc == 0).all() and (db == 0).all()
    with pytest.raises(ValueError):
        gb.seed(3)                                      # a removed id is not reused
    gb.seed(40)
    gb.insert_batch(np.arange(41, N, dtype=np.int32))
    assert gb.entry == 40 and gb.stats()["inserted"] == N - 40
    gb.close()
    bq.close()


# ------------------------------------------------------------------- quality -------------------------------------------------------------------

# recall@10 of the repaired graph may fall below the recall of a graph REBUILT from the survivors by at most M: the largest gap observed
# on the MI355X over data seeds 1, 2, 3 (quality_pair below) plus 0.02 for seed-to-seed spread, never above 0.10.
# Measured: gaps +0.0000, +0.0031, +0.0000 -> M = 0.0031 + 0.02.
MEASURED = [(1.0000, 1.0000), (0.9969, 1.0000), (1.0000, 1.0000)]   # (recall_repaired, recall_rebuilt) for data seeds 1, 2, 3
M = 0.0231

QUALITY = dict(N=4000, D=256, max_degree=16, beam=60, alpha=1.2, overflow=1.2, batch=256)


def quality_pair(ctx, data_seed):
    p = QUALITY
    N, D = p["N"], p["D"]
    v = cluster_data(N, D, data_seed, clusters=20)
    rng = np.random.default_rng(1000 + data_seed)
    gone = np.sort(rng.choice(N, N // 5, replace=False)).astype(np.int32)
    keep = np.setdiff1d(np.arange(N), gone)
    q = (v[rng.choice(keep, 64, replace=False)] + 0.1 * rng.standard_normal((64, D))).astype(np.float32)
    truth = keep[np.argsort(-(q @ v[keep].T), axis=1, kind="stable")[:, :10]]        # ground truth over the survivors only
    vs = J.VectorSet(ctx, v)

    def recall(graph, bq, vectors, ids_map=None):
        ids, _ = J.BQGraphSearcher(ctx, graph, bq, vectors).search(q, VSF.DOT_PRODUCT, 10, 200)
        ids = ids if ids_map is None else np.where(ids >= 0, ids_map[np.maximum(ids, 0)], -1)
        return float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / 10.0 for i in range(len(q))]))

    gb, bq, _, _ = build(ctx, v, D, p["max_degree"], p["overflow"], beam=p["beam"], alpha=p["alpha"], batch=p["batch"])
    gb.mark_deleted(gone)
    gb.remove_deleted()
    rows = gb.finish(np.empty((N, p["max_degree"]), np.int32))
    g = J.GraphIndex(ctx, N, [(None, rows)], gb.entry, 0)
    repaired = recall(g, bq, vs)
    g.close()
    gb.close()
    bq.close()
    gb, bq, _, _ = build(ctx, v[keep], D, p["max_degree"], p["overflow"], beam=p["beam"], alpha=p["alpha"], batch=p["batch"])
    rows = gb.finish(np.empty((len(keep), p["max_degree"]), np.int32))
    g = J.GraphIndex(ctx, len(keep), [(None, rows)], gb.entry, 0)
    vk = J.VectorSet(ctx, v[keep])
    rebuilt = recall(g, bq, vk, keep)
    g.close()
    gb.close()
    bq.close()
    return repaired, rebuilt


def test_a_repaired_graph_searches_as_well_as_a_rebuilt_one(ctx):
    repaired, rebuilt = quality_pair(ctx, 1)
    print(f"recall@10 repaired {repaired:.4f} rebuilt {rebuilt:.4f} gap {rebuilt - repaired:+.4f}")
    assert M <= 0.10
    assert repaired >= rebuilt - M, (repaired, rebuilt, M)
