"""The BQ builder on the MI355X (include/jvector_bq_builder.h through BQGraphBuilder / build_bq_layered) against the yardstick of
tests/bq_builder_yardstick.py: with ONE node per batch the working lists — ids, order, score bits, diverseBefore marks — and the
adjacency after finish equal the oracle's one-thread GraphIndexBuilder byte for byte, under the scaled sign quantizer for any alpha and
under the plain one at alpha = 1.0 for row widths the scaled form does not cover.  Larger batches are pinned structurally, by
reproducibility, and by the recall of a search over them against the oracle's graph of the same rows.  The CPU twin (ABI, the
yardstick's own pins, the entry-point body on the lane emulator) is tests/test_bq_builder_cpu.py."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from bq_builder_yardstick import check_bq_reference_order, cluster_data, np_majority, np_nearest_row, oracle_builder
from bq_graph_yardstick import np_encode


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


# ---------------------------------------------------- one node per batch: the reference ----------------------------------------------------

@pytest.mark.parametrize("D,N,max_degree,beam,alpha,overflow,dup,improve", [
    (64, 1200, 8, 30, 1.2, 1.2, 40, 0),
    (256, 1200, 16, 40, 1.4, 2.0, 0, 0),
    (64, 600, 8, 30, 1.2, 1.2, 40, 1),
])
def test_one_node_batches_equal_the_reference_at_any_alpha(ctx, D, N, max_degree, beam, alpha, overflow, dup, improve):
    v = cluster_data(N, D, 11 + D, dup=dup)
    out, st, info = check_bq_reference_order(J, ctx, v, D, max_degree, beam, alpha, overflow, improve=improve)
    assert st["reprunes"] > 0 and st["inserted"] == N and (out >= 0).sum(axis=1).max() <= max_degree


@pytest.mark.parametrize("D", [100, 768])
def test_one_node_batches_generic_and_odd_widths(ctx, D):
    """W = 2 through the generic path with padding bits, and W = 12: the plain sign quantizer at alpha = 1.0 — ids, order and marks
    against the oracle, scores against np_similarity"""
    v = cluster_data(600, D, 5 + D, dup=20)
    _, st, _ = check_bq_reference_order(J, ctx, v, D, 8, 30, 1.0, 1.5, scaled=False)
    assert st["reprunes"] > 0


def test_forced_second_pass_of_the_search_inside_a_build(ctx):
    N, D = 300, 64
    v = cluster_data(N, D, 11 + D, dup=40)
    want, _, _ = check_bq_reference_order(J, ctx, v, D, 8, 30, 1.2, 1.2)
    ctx.set_option("bq_gs_vcap_log2", 8)
    ctx.set_option("bq_gs_cand_cap", 128)
    try:
        ctx.reset_stats()
        out, _, _ = check_bq_reference_order(J, ctx, v, D, 8, 30, 1.2, 1.2)
        assert ctx.stat("bq_gs_queries_retried") > 0
    finally:
        ctx.set_option("bq_gs_vcap_log2", None)
        ctx.set_option("bq_gs_cand_cap", None)
    assert np.array_equal(out, want)


# ------------------------------------------------------------- the layered build -------------------------------------------------------------

_MASK = (1 << 64) - 1


def _splitmix(st):
    st = (st + 0x9E3779B97F4A7C15) & _MASK
    z = st
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return st, z ^ (z >> 31)


def splitmix_permutation(n, seed):
    """jv_internal.h seeded_permutation"""
    st, p = seed & _MASK, list(range(n))
    for i in range(n - 1, 0, -1):
        st, z = _splitmix(st)
        j = z % (i + 1)
        p[i], p[j] = p[j], p[i]
    return p


GS_MAX_LEVELS = 32   # gs_params.h: the graph's device view holds at most this many levels


def splitmix_levels(n, max_degree, seed, min_top):
    """jv_internal.h layered_draw_levels: (level of every node, top level kept; at most GS_MAX_LEVELS levels exist)"""
    ml = 1.0 / math.log(max_degree)
    st, lv = (seed ^ 0xA5A5A5A55A5A5A5A) & _MASK, []
    for _ in range(n):
        u = 0.0
        while u == 0.0:
            st, z = _splitmix(st)
            u = (z >> 11) * (1.0 / 9007199254740992.0)
        lv.append(min(int(-math.log(u) * ml), 31))
    lv = np.array(lv)
    top = 0
    while top + 1 < GS_MAX_LEVELS and top + 1 <= 31 and (lv >= top + 1).sum() >= min_top:
        top += 1
    return np.minimum(lv, top), top


def test_layered_build_with_one_node_batches(ctx):
    """jv_hip_bq_build_layered with max_batch = 1.  The level draws are restated here and fed to OracleBuilder(add_hierarchy = True)
    through set_levels: every level must hold exactly the nodes the oracle puts on it.  The hierarchical oracle is used for that level
    membership ONLY: its adjacency is NOT compared.  Byte equality is per level against FLAT oracles, as in
    test_builder_reference_order.check_layered_reference_order: each level of the engine is a graph of its own (the reference hands
    entry points from level to level inside one insert), so each level's adjacency equals the oracle's one-thread build of that
    level's rows, inserted in the engine's seeded order, improved, degree-enforced.  The ENTRY NODE is checked against the numpy
    majority / nearest-row restatement, not against the oracle: the oracle enters at the first node of the top level, the engine at
    the top level's member nearest to its bitwise-majority row — different by design."""
    N, D, max_degree, beam, alpha, overflow, seed, min_top, improve = 1000, 64, 8, 30, 1.2, 1.2, 11, 4, 1
    v = cluster_data(N, D, 77, dup=20)
    words = np_encode(v, D)
    bq = J.BQVectors(ctx, D, words=words)
    g = J.build_bq_layered(ctx, bq, max_degree, beam, alpha, overflow, max_batch=1, improve=improve, seed=seed, min_top=min_top)
    lv, top = splitmix_levels(N, max_degree, seed, min_top)
    assert len(g.levels) == top + 1 >= 2 and g.entry_level == top
    oh = oracle_builder(v, D, max_degree, beam, alpha, overflow, add_hierarchy=True, levels=lv.astype(np.int8))
    for i in splitmix_permutation(N, seed):
        assert oh.add(i) == lv[i]
    for l, (ids, rows) in enumerate(g.levels):
        gids = np.arange(N, dtype=np.int32) if ids is None else np.asarray(ids)
        assert np.array_equal(gids, np.flatnonzero(lv >= l))
        assert [i for i in range(N) if (oh.row(l, i) is None) != (lv[i] < l)] == []
        ob = oracle_builder(v[gids], D, max_degree, beam, alpha, overflow, improve=improve > 0)
        order = splitmix_permutation(len(gids), seed + l)
        for i in order:
            ob.add(i)
        for _ in range(improve):
            for i in order:
                ob.improve(i)
        ob.cleanup()
        want = ob.rows(0, max_degree)
        want = np.where(want >= 0, gids[np.maximum(want, 0)], -1).astype(np.int32)
        assert np.array_equal(np.asarray(rows), want), (l, np.argwhere((np.asarray(rows) != want).any(axis=1))[:5])
    members = np.flatnonzero(lv >= top).astype(np.int32)
    want_entry, _h = np_nearest_row(words, members, np_majority(words[members]))
    assert g.entry_node == want_entry
    g.close()
    bq.close()


# -------------------------------------------------------------- batched builds --------------------------------------------------------------

# recall@10 of the batched build may fall below the recall of the oracle's one-thread graph of the same rows by at most M.  M is meant
# to be the largest gap observed on the MI355X over data seeds 1, 2, 3 (recall_pair below) plus 0.02 for seed variation, and may never
# exceed 0.10: a batched build that loses more than that to batching is a defect to find, not a tolerance to widen.
# NOT MEASURED: there are no three pairs to quote, and M is the ceiling itself, the widest value the rule allows.  The test prints its
# pair before it asserts; recall_pair for seeds 1, 2, 3 is the measurement, and its pairs and the lowered M belong here and in DESIGN §9.
MEASURED = None   # [(recall_batched, recall_oracle_graph)] for data seeds 1, 2, 3
M = 0.10

BATCHED = dict(N=4000, D=256, max_degree=16, beam=60, alpha=1.2, overflow=1.2, max_batch=256, improve=1, seed=11, min_top=8)


def batched_problem(data_seed):
    p = BATCHED
    v = cluster_data(p["N"], p["D"], data_seed, clusters=20)
    rng = np.random.default_rng(1000 + data_seed)
    q = (v[rng.choice(p["N"], 64, replace=False)] + 0.1 * rng.standard_normal((64, p["D"]))).astype(np.float32)
    truth = np.argsort(-(q @ v.T), axis=1, kind="stable")[:, :10]
    return v, q, truth


def build_batched(ctx, bq):
    p = BATCHED
    return J.build_bq_layered(ctx, bq, p["max_degree"], p["beam"], p["alpha"], p["overflow"], max_batch=p["max_batch"], improve=p["improve"],
                              seed=p["seed"], min_top=p["min_top"])


def oracle_graph(ctx, v):
    """the oracle's one-thread build of the same rows (CPU), one improve pass, as a GraphIndex"""
    p = BATCHED
    ob = oracle_builder(v, p["D"], p["max_degree"], p["beam"], p["alpha"], p["overflow"], improve=True)
    for i in range(p["N"]):
        ob.add(i)
    for i in range(p["N"]):
        ob.improve(i)
    ob.cleanup()
    return J.GraphIndex(ctx, p["N"], [(None, ob.rows(0, p["max_degree"]))], 0, 0)


def recall_at_10(ctx, graph, bq, vs, q, truth):
    ids, _ = J.BQGraphSearcher(ctx, graph, bq, vs).search(q, VSF.DOT_PRODUCT, 10, 200)
    return float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / 10.0 for i in range(len(q))]))


def recall_pair(ctx, data_seed):
    """(recall of the batched build, recall of the oracle's graph, the batched GraphIndex, its BQVectors)"""
    v, q, truth = batched_problem(data_seed)
    bq = J.BQVectors(ctx, BATCHED["D"], words=np_encode(v, BATCHED["D"]))
    vs = J.VectorSet(ctx, v)
    g = build_batched(ctx, bq)
    og = oracle_graph(ctx, v)
    rb, ro = recall_at_10(ctx, g, bq, vs, q, truth), recall_at_10(ctx, og, bq, vs, q, truth)
    og.close()
    return rb, ro, g, bq


def test_batched_build_is_reproducible_well_formed_and_searchable(ctx):
    N, Rf = BATCHED["N"], BATCHED["max_degree"]
    rb, ro, g, bq = recall_pair(ctx, 1)
    print(f"recall@10 batched {rb:.4f} oracle graph {ro:.4f} gap {ro - rb:+.4f}")
    g2 = build_batched(ctx, bq)
    assert len(g.levels) == len(g2.levels) >= 2 and (g.entry_node, g.entry_level) == (g2.entry_node, g2.entry_level)
    for (ids, rows), (ids2, rows2) in zip(g.levels, g2.levels):
        assert (ids is None and ids2 is None) or np.array_equal(ids, ids2)
        assert np.array_equal(rows, rows2)
    for ids, rows in g.levels:
        gids = np.arange(N, dtype=np.int32) if ids is None else ids
        assert rows.shape == (len(gids), Rf) and rows.max() < N and rows.min() >= -1
        deg = (rows >= 0).sum(axis=1)
        assert deg.max() <= Rf and all((rows[i, :deg[i]] >= 0).all() and (rows[i, deg[i]:] == -1).all() for i in range(len(gids)))   # packed
        assert not (rows == gids[:, None]).any()                                                                                  # no self loop
        srt = np.sort(rows, axis=1)
        assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()                                                          # no duplicate
        if ids is not None:
            assert np.isin(rows[rows >= 0], gids).all()
    assert M <= 0.10
    assert rb >= ro - M, (rb, ro, M)
    g.close()
    g2.close()
    bq.close()


# ----------------------------------------------------------------- refusals -----------------------------------------------------------------

def test_refusals_leave_the_builder_usable(ctx):
    D, N = 64, 200
    v = cluster_data(N, D, 9)
    bq = J.BQVectors(ctx, D, words=np_encode(v, D))
    g0 = J.GraphIndex(ctx, N, [(None, np.full((N, 4), -1, np.int32))], 0, 0)
    # a beam the builder's own range (1..4096) allows and the traversal kernel's LDS block does not hold.  With the default candidate
    # tier (2048 entries) the limit is (65536 - 8 (2048 + 320)) / 8 = 5824, above every legal beam; it follows bq_gs_cand_cap, and with
    # the widest tier, 4096, it is (65536 - 8 (4096 + 320)) / 8 = 3776
    searcher = J.BQGraphSearcher(ctx, g0, bq)
    ctx.set_option("bq_gs_cand_cap", 4096)
    try:
        max_k = searcher.max_rerank_k()
        assert max_k < 4096, max_k
        for beam in (max_k + 1, 4096):
            with pytest.raises(UnsupportedError, match="beamWidth .* above the .* results"):
                J.BQGraphBuilder(ctx, bq, 8, beam, 1.2, 1.2)
        J.BQGraphBuilder(ctx, bq, 8, 30, 1.2, 1.2).close()    # a legal beam under the same option
    finally:
        ctx.set_option("bq_gs_cand_cap", None)
    assert searcher.max_rerank_k() >= 4096                    # the default tier refuses no legal beam ...
    J.BQGraphBuilder(ctx, bq, 8, 30, 1.2, 1.2).close()        # ... and the builder can still be created
    g0.close()
    wide = J.BQVectors(ctx, 16383, words=np.zeros((4, 256), np.uint64))   # rows too wide for any candidate list
    assert J.BQBuildScorer(ctx, None, wide).max_candidates(8) < 30 + 9
    with pytest.raises(UnsupportedError, match="candidates"):
        J.BQGraphBuilder(ctx, wide, 8, 30, 1.2, 1.2)
    wide.close()
    for bad in (dict(max_degree=1), dict(max_degree=65), dict(beam_width=0), dict(alpha=0.9), dict(overflow=9.0)):
        with pytest.raises(ValueError):
            J.BQGraphBuilder(ctx, bq, **{**dict(max_degree=8, beam_width=30, alpha=1.2, overflow=1.2), **bad})
    gb = J.BQGraphBuilder(ctx, bq, 8, 30, 1.2, 1.2)
    with pytest.raises(ValueError):
        gb.insert_batch(np.array([1], np.int32))              # insert before seed
    gb.seed(0)
    gb.insert_batch(np.array([1, 2], np.int32))
    for nodes in ([3, 4, 3], [3, N], [-1, 3]):                # a repeated id, an id out of range
        with pytest.raises(ValueError):
            gb.insert_batch(np.array(nodes, np.int32))
        with pytest.raises(ValueError):
            gb.improve_batch(np.array(nodes, np.int32))
    assert gb.stats()["inserted"] == 3
    ids, _, _ = gb.working_rows()
    assert (ids[3:] == -1).all()                              # nothing of a refused batch reached the lists
    for lo in range(3, N, 50):
        gb.insert_batch(np.arange(lo, min(N, lo + 50), dtype=np.int32))
    gb.improve_batch(np.arange(N, dtype=np.int32))
    out = gb.finish(np.empty((N, 8), np.int32))
    assert gb.stats()["inserted"] == N and (out >= 0).sum(axis=1).min() >= 1 and out.max() < N
    gb.close()
    bq.close()
