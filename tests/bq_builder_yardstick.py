"""Shared by the BQ builder tests: the yardstick — the oracle's one-thread restatement of GraphIndexBuilder (oracle.OracleBuilder)
driven by a sign quantizer so that every score it forms is a BQ similarity — and the driver that compares a jv_bq_builder with it.

bq_graph_yardstick.sign_pq (centroids +-1, euclidean) walks in BQ order because its score 1 / (1 + 4 h) is strictly decreasing in the
Hamming distance h.  That pins searches, and a builder at alpha = 1.0 only: the prune test sim(c, j) > score(c) * alpha is not invariant
under a monotone map of the scores once alpha > 1.

The exact quantizer for any alpha: for D in {16, 64, 256, 1024}, where 1 / sqrt(D) is a power of two, the same sign quantizer with
centroids +-1 / sqrt(D) (scaled_sign_pq), the oracle given the vectors where(v > 0, 1 / sqrt(D), -1 / sqrt(D)) (scaled_sign_vectors),
under DOT_PRODUCT.  Every product is +-1 / D and every partial sum an exact multiple of 1 / D, so the oracle's score (1 + dot) / 2
equals 1 - (float) h / D bit for bit, on the ADC side (the insert's search) and on the code-to-code side (the diversity score)."""
import numpy as np

from oracle import oracle as O

from bq_build_yardstick import pair_similarity
from bq_graph_yardstick import np_encode, sign_codes, sign_pq, sign_queries

SCALED_DIMS = (16, 64, 256, 1024)


def scaled_sign_pq(D):
    assert D in SCALED_DIMS, D
    s = np.float32(1.0) / np.float32(np.sqrt(np.float32(D)))
    c = np.arange(256)
    cb = np.where((c[:, None] >> np.arange(8)[None, :]) & 1, s, -s).astype(np.float32).reshape(-1)   # [256][8], centroid-major
    return O.OraclePQ(D, D // 8, np.tile(cb, D // 8), None, 256, sizes=np.full(D // 8, 8, np.int32))


def scaled_sign_vectors(v, D):
    s = np.float32(1.0) / np.float32(np.sqrt(np.float32(D)))
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(v, np.float32) > 0, s, -s).astype(np.float32)


def cluster_data(N, D, seed, clusters=6, dup=0):
    """`clusters` Gaussian clusters; the last `dup` rows repeat the first `dup`: equal words, tied scores everywhere"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((clusters, D)).astype(np.float32)
    v = (centers[rng.integers(0, clusters, N)] + 0.7 * rng.standard_normal((N, D))).astype(np.float32)
    if dup:
        v[N - dup:] = v[:dup]
    return v


def oracle_builder(v, D, max_degree, beam, alpha, overflow, scaled=True, improve=False, **kw):
    """OracleBuilder over the sign quantizer: scaled (exact for any alpha, D in SCALED_DIMS) or plain (+-1, euclidean: alpha = 1 only)"""
    words = np_encode(v, D)
    codes = sign_codes(words, D)
    if scaled:
        return O.OracleBuilder(scaled_sign_pq(D), codes, scaled_sign_vectors(v, D), O.DOT_PRODUCT, max_degree, beam, alpha, overflow,
                               dedupe_ids=improve, improve_full_vectors=improve, improve_sorted_candidates=improve, **kw)
    return O.OracleBuilder(sign_pq(D), codes, sign_queries(v), O.EUCLIDEAN, max_degree, beam, alpha, overflow, dedupe_ids=improve,
                           improve_full_vectors=improve, improve_sorted_candidates=improve, **kw)


def score_bit_mismatches(ob, words, D, nodes):
    """(stored entries, entries whose score differs in any bit from np_similarity(hamming(row u, row id)))"""
    total = bad = 0
    for u in nodes:
        ids, sc, _db = ob.row(0, u)
        want = pair_similarity(words, D, u, ids)
        total += ids.size
        bad += int((sc.view(np.int32) != want.view(np.int32)).sum())
    return total, bad


def _compare_lists(gb, ob, words, D, nodes, scaled, tag):
    ids, sc, db = gb.working_rows()
    for u in nodes:
        oi, osc, odb = ob.row(0, u)
        n = int((ids[u] >= 0).sum())
        assert n == oi.size and np.array_equal(ids[u, :n], oi), (tag, u, ids[u], oi)
        assert int(db[u]) == odb, (tag, u, int(db[u]), odb)
        want = osc if scaled else pair_similarity(words, D, u, oi)   # (the plain quantizer's own scores are 1 / (1 + 4 h))
        assert np.array_equal(sc[u, :n].view(np.int32), want.view(np.int32)), (tag, u, sc[u, :n], want)
        assert len(set(oi.tolist())) == oi.size


def check_bq_reference_order(J, ctx, v, D, max_degree, beam, alpha, overflow, improve=0, scaled=True):
    """ONE node per batch == addGraphNode; finish == cleanup's enforceDegree; `improve` passes of improveConnections over every node in
    between, with the engine's three stated deviations switched on in the oracle.  Compared: the working lists (ids, order, score bits,
    diverseBefore marks) at inserts 1, 2, 3, N / 3, N / 2 and N - 1 and after the improve of nodes 0, 1, N / 2 and N - 1, then the
    final adjacency.  Returns (engine rows, builder stats, oracle info)."""
    assert scaled or alpha == 1.0, "the plain sign quantizer pins a builder at alpha = 1.0 only"
    N = len(v)
    words = np_encode(v, D)
    bq = J.BQVectors(ctx, D, words=words)
    gb = J.BQGraphBuilder(ctx, bq, max_degree, beam, alpha, overflow)
    ob = oracle_builder(v, D, max_degree, beam, alpha, overflow, scaled=scaled, improve=improve > 0)
    gb.seed(0)
    ob.add(0)
    for i in range(1, N):
        gb.insert_batch(np.array([i], np.int32))
        ob.add(i)
        if i in (1, 2, 3, N // 3, N // 2, N - 1):
            _compare_lists(gb, ob, words, D, range(i + 1), scaled, ("insert", i))
    for _ in range(improve):
        for i in range(N):
            gb.improve_batch(np.array([i], np.int32))
            ob.improve(i)
            if i in (0, 1, N // 2, N - 1):
                _compare_lists(gb, ob, words, D, range(N), scaled, ("improve", i))
    out = np.empty((N, max_degree), np.int32)
    gb.finish(out)
    st = gb.stats()
    gb.close()
    bq.close()
    ob.cleanup()
    want = ob.rows(0, max_degree)
    assert np.array_equal(out, want), np.argwhere((out != want).any(axis=1))[:5]
    info = ob.info()
    assert st["reprunes"] <= info["reprunes"]   # (the oracle also counts the insertDiverse prunes of the inserts; callers pin > 0)
    return out, st, info


def np_majority(words):
    """bit b set iff strictly more than half of the rows have it set (integer counts)"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")
    cnt = bits.astype(np.int64).sum(axis=0)
    maj = (2 * cnt > len(words)).astype(np.uint8)
    return np.packbits(maj, bitorder="little").view("<u8").astype(np.uint64)


def np_nearest_row(words, ids, centroid):
    """(id, hamming) of the member at minimum Hamming distance to centroid; ties to the smaller id"""
    x = np.bitwise_xor(np.ascontiguousarray(words[ids]), centroid[None, :])
    h = np.unpackbits(x.view(np.uint8), axis=1).astype(np.int64).sum(axis=1)
    order = np.lexsort((np.asarray(ids, np.int64), h))
    return int(np.asarray(ids)[order[0]]), int(h[order[0]])
