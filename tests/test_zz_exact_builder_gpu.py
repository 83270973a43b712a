"""The exact-score builder on the MI355X (include/jvector_exact_builder.h through ExactGraphBuilder / build_exact_layered).

Yardstick: oracle.OracleBuilder, the one-thread restatement of GraphIndexBuilder, driven by a bridge quantizer whose centroids ARE the
rows, so that every score it forms is the exact similarity.  test_builder_reference_goldens.py's bridge (ONE sub-space over all D
dimensions) is exact only for D < 8: the oracle's sub-space sums are sequential, VectorSimilarityFunction.compare adds in blocks of
eight.  The bridge here splits the dimensions where compare's chain does — DOT_PRODUCT: the D % 8 front remainder, then the 8-blocks;
EUCLIDEAN: the 8-blocks, then D % 8 sub-spaces of one — and asserts on the CPU, before a case uses it, that jvo_pq_direct_score equals
jvo_compare bit for bit on the case's rows.  That holds for DOT_PRODUCT and EUCLIDEAN at every D; for COSINE no split makes it hold
(the quantizer's query norm is a blocked sum, compare's a sequential one), so COSINE gets the batch and layered checks only, against
oracle.compare_many.  Every comparison is exact: no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd.exact_builder import gather_rows
from oracle import oracle as O
from bq_graph_yardstick import np_encode
from exact_build_ref import clustered
from test_builder_reference_goldens import CASES
from test_zz_bq_builder_gpu import splitmix_levels

# GraphIndexBuilderTest.testRescore (:82-104), the part before the rescore: node 0's list is [1, 2] in that order, scores 0.5 and 0.2
LITERALS = dict(CASES, testRescoreFirstHalf=(O.EUCLIDEAN, 2, [[0, 0], [0, 1], [2, 0]], [([0, 1, 2], {0: [1, 2]})]))


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def bridge(v, vsf):
    """(OraclePQ, codes) scoring exactly compare(v[i], v[j]); asserted bit for bit on every pair of rows"""
    n, D = v.shape
    assert n <= 256 and int(vsf) in (O.EUCLIDEAN, O.DOT_PRODUCT)
    sizes = [D % 8] * (D % 8 > 0) + [8] * (D // 8) if int(vsf) == O.DOT_PRODUCT else [8] * (D // 8) + [1] * (D % 8)
    off = np.concatenate([[0], np.cumsum(sizes)])
    cb = np.concatenate([v[:, off[m]:off[m + 1]].reshape(-1) for m in range(len(sizes))])
    opq = O.OraclePQ(D, len(sizes), cb, None, n, sizes=np.asarray(sizes, np.int32))
    codes = np.repeat(np.arange(n, dtype=np.uint8)[:, None], len(sizes), axis=1)
    for i in range(n):
        got = np.float32([O.lib().jvo_pq_direct_score(opq.ref, O._f(v[i]), int(vsf), O._u8(codes[j])) for j in range(n)])
        assert np.array_equal(got.view(np.int32), pair_scores(vsf, v, i, np.arange(n)).view(np.int32)), (int(vsf), D, i)
    return opq, codes


def pair_scores(vsf, v, u, ids):
    return np.asarray(O.compare_many(int(vsf), v[u], v[np.asarray(ids, np.int64)]), np.float32)


def assert_lists_equal_the_oracle(gb, ob, nodes, tag):
    ids, sc, db = gb.working_rows()
    for u in nodes:
        oi, osc, odb = ob.row(0, u)
        n = int((ids[u] >= 0).sum())
        assert n == oi.size and np.array_equal(ids[u, :n], oi) and (ids[u, n:] == -1).all(), (tag, u, ids[u], oi)
        assert np.array_equal(sc[u, :n].view(np.int32), osc.view(np.int32)), (tag, u, sc[u, :n], osc)
        assert int(db[u]) == odb, (tag, u, int(db[u]), odb)


# ------------------------------------------------ one node per batch: the reference itself ------------------------------------------------

@pytest.mark.parametrize("name", sorted(LITERALS))
def test_reference_literals_one_node_per_batch(ctx, name):
    vsf, max_degree, vectors, steps = LITERALS[name]
    v = np.asarray(vectors, np.float32)
    opq, codes = bridge(v, vsf)
    ob = O.OracleBuilder(opq, codes, v, vsf, max_degree, 10, alpha=1.0, neighbor_overflow=1.0)
    gb = J.ExactGraphBuilder(ctx, J.VectorSet(ctx, v), J.VectorSimilarityFunction(int(vsf)), max_degree, 10, 1.0, 1.0)
    for add, expected in steps:
        for node in add:
            ob.add(node)
            gb.seed(node) if gb.stats()["inserted"] == 0 else gb.insert_batch(np.array([node], np.int32))
        ids, sc, _db = gb.working_rows()
        for node, want in expected.items():
            row = ids[node][ids[node] >= 0]
            assert sorted(row.tolist()) == want, (name, add, node, row.tolist(), want)
            assert np.array_equal(sc[node, :len(row)].view(np.int32), pair_scores(vsf, v, node, row).view(np.int32))
        assert_lists_equal_the_oracle(gb, ob, expected, (name, add))
    if name == "testRescoreFirstHalf":
        assert ids[0].tolist() == [1, 2] and sc[0].tolist() == [0.5, np.float32(0.2)]
    gb.close()


# D = 3 and 65: rows that are not 16-byte aligned; 24: one short chunk; 128: two full chunks; 260: past one 256-dimension tile.  Every D
# once and every (maxDegree, overflow, alpha) once per similarity; dup: the last rows repeat the first, scores tie everywhere
@pytest.mark.parametrize("vsf", [O.EUCLIDEAN, O.DOT_PRODUCT])
@pytest.mark.parametrize("D,max_degree,overflow,alpha,beam,dup,improve", [
    (3, 4, 1.0, 1.0, 10, 0, 0),
    (24, 8, 1.2, 1.2, 40, 30, 0),
    (65, 16, 1.5, 1.4, 10, 0, 1),
    (128, 8, 1.2, 1.2, 40, 0, 1),
    (260, 16, 1.5, 1.4, 40, 0, 0),
])
def test_one_node_batches_equal_the_reference(ctx, vsf, D, max_degree, overflow, alpha, beam, dup, improve):
    N = 200
    v = clustered(100 + D, N, D)
    if dup:
        v[N - dup:] = v[:dup]
    opq, codes = bridge(v, vsf)
    # (the engine's three stated deviations of improve_batch are switched on in the oracle)
    ob = O.OracleBuilder(opq, codes, v, vsf, max_degree, beam, alpha, overflow, dedupe_ids=improve > 0, improve_full_vectors=improve > 0,
                         improve_sorted_candidates=improve > 0)
    gb = J.ExactGraphBuilder(ctx, J.VectorSet(ctx, v), J.VectorSimilarityFunction(int(vsf)), max_degree, beam, alpha, overflow)
    gb.seed(0)
    ob.add(0)
    for i in range(1, N):
        gb.insert_batch(np.array([i], np.int32))
        ob.add(i)
    assert_lists_equal_the_oracle(gb, ob, range(N), "inserts")
    for _ in range(improve):
        for i in range(N):
            gb.improve_batch(np.array([i], np.int32))
            ob.improve(i)
        assert_lists_equal_the_oracle(gb, ob, range(N), "improve")
    out = gb.finish(np.empty((N, max_degree), np.int32))
    ob.cleanup()
    assert_lists_equal_the_oracle(gb, ob, range(N), "finish")
    assert np.array_equal(out, ob.rows(0, max_degree))
    assert overflow == 1.0 or gb.stats()["reprunes"] > 0
    gb.close()


# ----------------------------------------------------------- larger batches -----------------------------------------------------------

def unit_rows(v):
    """DOT_PRODUCT is for unit vectors: (1 + dot) / 2 below zero is a score the search walks past and never keeps"""
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def build_in_batches(ctx, vs, vsf, N, max_degree, beam, alpha, overflow, max_batch):
    gb = J.ExactGraphBuilder(ctx, vs, vsf, max_degree, beam, alpha, overflow)
    gb.seed(0)
    lo = 1
    while lo < N:   # prefix doubling
        hi = min(N, lo + min(max_batch, lo))
        gb.insert_batch(np.arange(lo, hi, dtype=np.int32))
        lo = hi
    return gb


@pytest.mark.parametrize("vsf", [O.EUCLIDEAN, O.DOT_PRODUCT, O.COSINE])
def test_batched_build_scores_order_and_reproducibility(ctx, vsf):
    N, D, max_degree, beam, alpha, overflow = 2000, 64, 16, 40, 1.2, 1.2
    v = unit_rows(clustered(7, N, D))
    vs = J.VectorSet(ctx, v)
    outs = []
    for _ in range(2):
        gb = build_in_batches(ctx, vs, J.VectorSimilarityFunction(int(vsf)), N, max_degree, beam, alpha, overflow, 256)
        outs.append(gb.finish(np.empty((N, max_degree), np.int32)))
        ids, sc, _db = gb.working_rows()
        gb.close()
    assert np.array_equal(outs[0], outs[1])
    deg = (ids >= 0).sum(axis=1)
    assert deg.min() >= 1 and deg.max() <= max_degree and np.array_equal(ids[:, :max_degree], outs[1])
    for u in range(N):
        row = ids[u, :deg[u]]
        assert (row >= 0).all() and (ids[u, deg[u]:] == -1).all() and u not in row and len(set(row.tolist())) == len(row)
        assert np.array_equal(sc[u, :deg[u]].view(np.int32), pair_scores(vsf, v, u, row).view(np.int32)), u
        assert (np.diff(sc[u, :deg[u]]) <= 0).all()                     # NodeArray order


# --------------------------------------------------------- the layered build ---------------------------------------------------------

LAYERED = dict(N=3000, max_degree=8, seed=11)
_bq_counts = {}


def bq_level_counts(ctx, min_top):
    """the level counts of jv_hip_bq_build_layered for the same (N, maxDegree, seed, min_top): the same draw; built once per min_top"""
    if min_top not in _bq_counts:
        p = LAYERED
        bq = J.BQVectors(ctx, 32, words=np_encode(clustered(1, p["N"], 32), 32))
        g = J.build_bq_layered(ctx, bq, p["max_degree"], 20, 1.2, 1.2, max_batch=256, seed=p["seed"], min_top=min_top)
        _bq_counts[min_top] = g.build_stats["levels"]
        g.close()
        bq.close()
    return _bq_counts[min_top]


def assert_gathered_rows(ctx, vs, v, ids, VSF, max_degree=8):
    """gather_rows(ids), through a builder over the gathered set: every stored score is the similarity of the two GLOBAL rows"""
    gb = build_in_batches(ctx, gather_rows(ctx, vs, ids), VSF, len(ids), max_degree, 20, 1.2, 1.2, 64)
    lids, sc, _db = gb.working_rows()
    gb.close()
    for u in range(len(ids)):
        n = int((lids[u] >= 0).sum())
        assert n >= 1 and np.array_equal(sc[u, :n].view(np.int32), pair_scores(int(VSF), v, ids[u], ids[lids[u, :n]]).view(np.int32)), u


def np_entry(vsf, v, members):
    """the f32 sequential mean in ascending id, times 1 / count; the best compare(c, row), ties to the smaller id"""
    c = np.zeros(v.shape[1], np.float32)
    for i in members:
        c = c + v[i]
    c = c * (np.float32(1) / np.float32(len(members)))
    sc = np.asarray(O.compare_many(int(vsf), c, v[members]), np.float32)
    assert (sc == sc.max()).sum() >= 2                                    # the case holds a tie at the top
    return int(members[np.lexsort((members, -sc))[0]])


# D = 32 for each similarity; 28: 16-byte rows that the row tile does not take (D % 8 != 0); 27: rows that are not 16-byte aligned; 100
# and 136: the gather's groups of 32 and 64 lanes.  The draw gives levels of 3000 / 371 / 43 / 7 nodes: min_top 4 enters among 7 members
# (the mean's tail loop, one group); 40 among 43 (the mean's pipelined loop: five blocks of eight, then three); 300 among 371 (46
# blocks, six one-wave workgroups of the scan, the two equal rows in groups 1 and 5: the tie is decided among the per-wave winners)
@pytest.mark.parametrize("vsf,D,min_top", [(O.EUCLIDEAN, 32, 4), (O.DOT_PRODUCT, 32, 4), (O.COSINE, 32, 4), (O.EUCLIDEAN, 28, 4),
                                           (O.COSINE, 27, 4), (O.EUCLIDEAN, 100, 4), (O.DOT_PRODUCT, 136, 4),
                                           (O.EUCLIDEAN, 32, 40), (O.COSINE, 27, 40), (O.DOT_PRODUCT, 136, 40),
                                           (O.EUCLIDEAN, 32, 300), (O.DOT_PRODUCT, 32, 300), (O.COSINE, 32, 300), (O.EUCLIDEAN, 28, 300)])
def test_layered_build(ctx, vsf, D, min_top):
    p = LAYERED
    N, max_degree = p["N"], p["max_degree"]
    lv, top = splitmix_levels(N, max_degree, p["seed"], min_top)
    members = np.flatnonzero(lv >= top).astype(np.int32)
    assert (top, len(members)) == {4: (3, 7), 40: (2, 43), 300: (1, 371)}[min_top]
    v = unit_rows(clustered(3, N, D))
    m = v[members].mean(axis=0)
    twins = members[[len(members) // 5, len(members) - 2]]                       # two equal rows, the nearest to the mean
    v[twins] = m / np.linalg.norm(m) if int(vsf) == O.DOT_PRODUCT else m
    vs = J.VectorSet(ctx, v)
    VSF = J.VectorSimilarityFunction(int(vsf))
    g = J.build_exact_layered(ctx, vs, VSF, max_degree, 20, 1.2, 1.2, max_batch=256, improve=1, seed=p["seed"], min_top=min_top)
    assert g.build_stats["levels"] == bq_level_counts(ctx, min_top) and len(g.levels) == top + 1 and g.entry_level == top
    assert g.entry_node == np_entry(vsf, v, members) == twins[0]
    for l, (ids, rows) in enumerate(g.levels):
        gids = np.arange(N, dtype=np.int32) if ids is None else ids
        assert np.array_equal(gids, np.flatnonzero(lv >= l)) and rows.shape == (len(gids), max_degree)
        assert np.isin(rows[rows >= 0], gids).all() and not (rows == gids[:, None]).any() and (rows >= 0).any(axis=1).all()
    g.close()
    if min_top == 4:
        assert_gathered_rows(ctx, vs, v, g.levels[1][0], VSF)


# the gather's shapes the layered cases do not reach: dwords in groups of 16 (D 13) and 64 lanes (65), and a second trip of the piece
# loop, more than 4 x 64 pieces per row (261 dwords, 1028 / 4 = 257 float4)
@pytest.mark.parametrize("D", [13, 65, 261, 1028])
def test_gathered_rows(ctx, D):
    v = clustered(5, 300, D)
    ids = np.random.default_rng(D).permutation(300)[:150].astype(np.int32)
    assert_gathered_rows(ctx, J.VectorSet(ctx, v), v, ids, J.VectorSimilarityFunction.EUCLIDEAN)


# -------------------------------------------------------------- refusals --------------------------------------------------------------

def test_refusals_leave_the_builder_as_it_was(ctx):
    N, D = 200, 24
    v = clustered(9, N, D)
    vs = J.VectorSet(ctx, v)
    g0 = J.GraphIndex(ctx, N, [(None, np.full((N, 4), -1, np.int32))], 0, 0)
    max_k = J.ExactGraphSearcher(ctx, g0, vs).max_beam_k()
    g0.close()
    assert max_k < 4096
    with pytest.raises(UnsupportedError, match="beamWidth .* above the .* results"):
        J.ExactGraphBuilder(ctx, vs, J.VectorSimilarityFunction.EUCLIDEAN, 8, max_k + 1, 1.2, 1.2)
    nvq = J.NVQuantization.compute(ctx, vs, 2).encode_all(vs).as_vector_set()
    with pytest.raises(UnsupportedError, match="NVQ rows"):
        J.ExactGraphBuilder(ctx, nvq, J.VectorSimilarityFunction.EUCLIDEAN, 8, 30, 1.2, 1.2)
    gb = J.ExactGraphBuilder(ctx, vs, J.VectorSimilarityFunction.EUCLIDEAN, 8, 30, 1.2, 1.2)
    before = gb.working_rows()
    with pytest.raises(ValueError, match="seed the graph first"):
        gb.insert_batch(np.array([1], np.int32))
    assert all(np.array_equal(a, b) for a, b in zip(before, gb.working_rows()))
    gb.seed(0)
    gb.insert_batch(np.array([1, 2], np.int32))
    after = gb.working_rows()
    assert not np.array_equal(before[0], after[0])
    for nodes in ([3, 4, 3], [3, N], [-1, 3]):                  # an id listed twice, an id outside the rows
        for call in (gb.insert_batch, gb.improve_batch):
            with pytest.raises(ValueError):
                call(np.array(nodes, np.int32))
    assert gb.stats()["inserted"] == 3 and all(np.array_equal(a, b) for a, b in zip(after, gb.working_rows()))
    gb.close()
