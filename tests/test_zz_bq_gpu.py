"""Binary quantization on the MI355X against numpy restated from the reference (BinaryQuantization.encodeTo, BQVectors.similarityBetween /
write / load, DefaultVectorUtilSupport.hammingDistance), with no tolerance: encode bit for bit, the byte format both ways, the gather
scorers, and jv_hip_bq_search_flat against the pipeline BQ similarities -> top-rerankK (NodeQueue order) -> exact rerank -> top-K."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import bq as B
from oracle import oracle as O

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def np_encode(v, D):
    """encodeTo: bit j of word i set iff v[64 i + j] > 0"""
    v = np.asarray(v, np.float32).reshape(-1, D)
    W = (D + 63) // 64
    bits = np.zeros((v.shape[0], W * 64), bool)
    with np.errstate(invalid="ignore"):
        bits[:, :D] = v > 0
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1, W).astype(np.uint64)


def np_hamming(q_words, rows):
    """hammingDistance of one query's words against every row -> int64 [N]"""
    x = np.bitwise_xor(rows, q_words[None, :])
    return _POP8[x.view(np.uint8)].reshape(len(rows), -1).sum(axis=1)


def np_similarity(h, D):
    return np.float32(1) - np.float32(h).astype(np.float32) / np.float32(D)


def java_block(D, words):
    n = len(words)
    out = struct.pack(">i", D) + b"\0" * (4 * D) + struct.pack(">i", n)
    if n:
        out += struct.pack(">i", words.shape[1]) + np.asarray(words, np.uint64).astype(">u8").tobytes()
    return out


def special_rows(rng, n, D):
    v = rng.standard_normal((n, D)).astype(np.float32)
    specials = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -np.nan], np.float32)
    m = rng.random((n, D)) < 0.2
    v[m] = specials[rng.integers(0, len(specials), int(m.sum()))]
    return v


@pytest.mark.parametrize("D", [1, 63, 64, 65, 127, 768, 1021, 1536])
def test_encode_bit_exact(ctx, D):
    import torch
    rng = np.random.default_rng(D)
    v = special_rows(rng, 37, D)
    want = np_encode(v, D)
    q = B.BinaryQuantization(ctx, D)
    assert np.array_equal(q.encode(v), want)                                    # host in, host out
    assert np.array_equal(q.encode(v[3]), want[3])                               # one vector
    dv = torch.from_numpy(v).cuda()
    got = q.encode(dv)                                                           # device in, device out
    torch.cuda.synchronize()
    assert got.is_cuda and np.array_equal(got.cpu().numpy().view(np.uint64), want)
    vs = J.VectorSet(ctx, v)                                                     # encodeAll from a jv_vectors range
    bv = q.encode_all(vs)
    assert bv.count() == 37 and np.array_equal(bv.get(), want)
    part = q.encode_all(vs, first=5, count=7)
    assert np.array_equal(part.get(), want[5:12])


@pytest.mark.parametrize("D", [1, 64, 65, 768])
def test_load_write_round_trip(ctx, D):
    rng = np.random.default_rng(7 + D)
    W = (D + 63) // 64
    words = np_encode(rng.standard_normal((11, D)).astype(np.float32), D)
    assert words.shape == (11, W)
    blob = java_block(D, words)
    bv = B.BQVectors.load(ctx, blob + b"next")
    assert bv.bytes_consumed == len(blob) and bv.dimension == D and bv.count() == 11
    assert np.array_equal(bv.get(), words)
    assert bv.write() == blob
    empty = B.BQVectors.load(ctx, java_block(D, np.zeros((0, W), np.uint64)))
    assert empty.count() == 0 and empty.write() == java_block(D, np.zeros((0, W), np.uint64))
    # upload / download of raw words, host and device
    import torch
    other = B.BQVectors(ctx, D, count=11)
    other.upload(0, torch.from_numpy(words.view(np.int64)).cuda())
    assert np.array_equal(other.get(), words) and other.write() == blob


def rows_hitting_every_distance(D, rng):
    """query words q and one row per h in [0, D]: the row flips the first h of D shuffled dimensions"""
    q = np.where(rng.random(D) < 0.5, 1.0, -1.0).astype(np.float32)
    perm = rng.permutation(D)
    rows = np.repeat(q[None, :], D + 1, axis=0)
    for h in range(D + 1):
        rows[h, perm[:h]] *= -1
    return q, rows


@pytest.mark.parametrize("D", [1, 63, 64, 65, 100, 768, 1021])
def test_scores_hit_every_distance(ctx, D):
    rng = np.random.default_rng(D + 100)
    q, rows = rows_hitting_every_distance(D, rng)
    qb = np_encode(q, D)[0]
    rb = np_encode(rows, D)
    h = np_hamming(qb, rb)
    assert np.array_equal(h, np.arange(D + 1))
    bv = B.BQVectors(ctx, D, words=rb)
    N = D + 1
    queries = np.stack([q, rows[N // 2]])
    ords = np.stack([np.arange(N, dtype=np.int32), rng.permutation(N).astype(np.int32)])
    ords[1, 0], ords[0, -1] = -1, N      # out of range: -inf
    got = bv.score_function_for(queries, ords)
    for i in range(2):
        qw = np_encode(queries[i], D)[0]
        ok = (ords[i] >= 0) & (ords[i] < N)
        want = np.full(N, -np.inf, np.float32)
        want[ok] = np_similarity(np_hamming(qw, rb[ords[i][ok]]), D)
        assert np.array_equal(got[i], want)
    # diversityFunctionFor: node vs node
    node1 = np.array([0, N - 1, N // 3, -1], np.int32)
    node2 = np.stack([rng.permutation(N)[:N] for _ in range(4)]).astype(np.int32)
    node2[2, 1] = -5
    got = bv.diversity_function_for(node1, node2)
    for p in range(4):
        if node1[p] < 0:
            assert np.all(got[p] == -np.inf)
            continue
        ok = node2[p] >= 0
        want = np.full(N, -np.inf, np.float32)
        want[ok] = np_similarity(np_hamming(rb[node1[p]], rb[node2[p][ok]]), D)
        assert np.array_equal(got[p], want)


def expected_search(words, D, vecs, queries, vsf, top_k, rerank_k, accept=None, id_base=0):
    Q = len(queries)
    qw = np_encode(queries, D)
    ids = np.full((Q, top_k), -1, np.int32)
    sc = np.full((Q, top_k), -np.inf, np.float32)
    rerank = vecs is not None and rerank_k > 0
    k1 = rerank_k if rerank else top_k
    for q in range(Q):
        sims = np_similarity(np_hamming(qw[q], words), D)
        if accept is None:
            keep = np.arange(len(words), dtype=np.int32)
        else:
            keep = np.nonzero(accept if accept.ndim == 1 else accept[q])[0].astype(np.int32)
        cand, cs = O.topk(keep, sims[keep], k1)
        if rerank and len(cand):
            exact = O.compare_many(int(vsf), queries[q], vecs[cand])
            wi, ws = O.topk(cand, exact, top_k)
        else:
            wi, ws = cand[:top_k], cs[:top_k]
        ids[q, :len(wi)] = wi + id_base
        sc[q, :len(ws)] = ws
    return ids, sc


def problem(seed, N, D, Q, dup=0):
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((N, D)).astype(np.float32)
    if dup:
        at = rng.choice(N, dup, replace=False)
        vecs[at] = vecs[at[0]]                              # dup identical rows: one distance shared by all of them
    queries = (vecs[rng.integers(0, N, Q)] + 0.3 * rng.standard_normal((Q, D))).astype(np.float32)
    if dup:
        queries[0] = vecs[at[0]] + 0.01 * rng.standard_normal(D).astype(np.float32)
    return vecs, queries


def run_case(ctx, vecs, queries, vsf, top_k, rerank_k, accept=None, id_base=0, with_vectors=True, device_out=False):
    N, D = vecs.shape
    q = B.BinaryQuantization(ctx, D)
    vs = J.VectorSet(ctx, vecs)
    bv = q.encode_all(vs)
    words = np_encode(vecs, D)
    assert np.array_equal(bv.get(), words)
    s = B.BQFlatSearcher(ctx, bv, vs if with_vectors else None, id_base=id_base)
    if device_out:
        import torch
        tq = torch.from_numpy(queries).cuda()
        gi, gs = s.search(tq, vsf, top_k, rerank_k, accept=accept)
        torch.cuda.synchronize()
        gi, gs = gi.cpu().numpy(), gs.cpu().numpy()
    else:
        gi, gs = s.search(queries, vsf, top_k, rerank_k, accept=accept)
    wi, ws = expected_search(words, D, vecs if with_vectors else None, queries, vsf, top_k, rerank_k, accept, id_base)
    assert np.array_equal(gi, wi), (gi, wi)
    assert np.array_equal(gs, ws), (gs, ws)
    return gi


@pytest.mark.parametrize("vsf", [VSF.DOT_PRODUCT, VSF.COSINE, VSF.EUCLIDEAN])
@pytest.mark.parametrize("N,D,Q", [(1, 64, 1), (100, 65, 7), (100, 128, 300), (100003, 128, 7), (100003, 96, 1)])
def test_search_flat_matches_pipeline(ctx, vsf, N, D, Q):
    vecs, queries = problem(N + D + Q, N, D, Q)
    top_k = 10
    for rerank_k in (0, top_k, 10 * top_k):
        run_case(ctx, vecs, queries, vsf, top_k, rerank_k)


def test_search_flat_top_k_above_count_and_no_vectors(ctx):
    vecs, queries = problem(5, 37, 70, 4)
    gi = run_case(ctx, vecs, queries, VSF.COSINE, 50, 60)
    assert np.all(gi[:, 37:] == -1)
    run_case(ctx, vecs, queries, VSF.DOT_PRODUCT, 50, 0)
    run_case(ctx, vecs, queries, VSF.DOT_PRODUCT, 5, 40, with_vectors=False)


@pytest.mark.parametrize("dup", [3000, 20000])
def test_search_flat_duplicate_rows_straddle_the_threshold(ctx, dup):
    # 3000 identical rows: every tie fits the list; 20000: more ties than the list holds, they go in by rank (smallest ids)
    vecs, queries = problem(dup, 100003, 128, 5, dup=dup)
    for vsf, top_k, rerank_k in ((VSF.EUCLIDEAN, 10, 0), (VSF.DOT_PRODUCT, 10, 100), (VSF.COSINE, 7, 1000)):
        run_case(ctx, vecs, queries, vsf, top_k, rerank_k)


def test_search_flat_accept_bits_id_base_device_outputs(ctx):
    N, D, Q = 100003, 192, 7
    vecs, queries = problem(11, N, D, Q)
    rng = np.random.default_rng(3)
    shared = rng.random(N) < 0.3
    run_case(ctx, vecs, queries, VSF.COSINE, 10, 100, accept=shared, id_base=1000)
    per_query = rng.random((Q, N)) < 0.5
    per_query[2] = False
    per_query[2, [5, 77, 99999]] = True                 # three accepted rows: a (-1, -inf) tail
    gi = run_case(ctx, vecs, queries, VSF.DOT_PRODUCT, 10, 20, accept=per_query, id_base=-3, device_out=True)
    assert sorted(gi[2, :3]) == [2, 74, 99996] and np.all(gi[2, 3:] == -1)
    run_case(ctx, vecs, queries, VSF.EUCLIDEAN, 10, 0, accept=per_query, device_out=True)


def test_search_flat_one_million_rows(ctx):
    vecs, queries = problem(12, 1_000_003, 64, 3)
    run_case(ctx, vecs, queries, VSF.DOT_PRODUCT, 10, 100)


def test_bad_arguments_are_errors(ctx):
    import ctypes as C
    lib = B.lib()
    vecs, queries = problem(1, 50, 64, 2)
    bv = B.BinaryQuantization(ctx, 64).encode_all(J.VectorSet(ctx, vecs))
    other = J.VectorSet(ctx, np.zeros((50, 65), np.float32))
    ids, sc = np.zeros((2, 5), np.int32), np.zeros((2, 5), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    args = (p(queries), 2, int(VSF.DOT_PRODUCT), 5, 10, None, 0, 0, p(ids), p(sc))
    assert lib.jv_hip_bq_search_flat(ctx._h, bv._h, other._h, *args) == -1                 # D mismatch
    assert "dimension" in J._lib.last_error()
    assert lib.jv_hip_bq_search_flat(ctx._h, None, None, *args) == -1                     # NULL handle
    assert lib.jv_hip_bq_search_flat(None, bv._h, None, *args) == -1                      # NULL context
    assert lib.jv_hip_bq_search_flat(ctx._h, bv._h, None, p(queries), 0, 1, 5, 10, None, 0, 0, p(ids), p(sc)) == 0   # Q = 0
    assert lib.jv_hip_bq_search_flat(ctx._h, bv._h, None, p(queries), 2, 1, 0, 10, None, 0, 0, p(ids), p(sc)) == -1  # topK 0
    assert lib.jv_hip_bq_search_flat(ctx._h, bv._h, None, p(queries), 2, 1, 5, 10, p(ids), 0 + 0, 0, None, p(sc)) == -1
    assert lib.jv_hip_bq_encode_into(ctx._h, other._h, 0, 50, bv._h, 0) == -1             # D mismatch
    assert lib.jv_hip_bq_scores(ctx._h, None, p(queries), 2, p(ids), 5, p(sc)) == -1
    assert lib.jv_hip_bq_create(ctx._h, 0, 5, C.byref(C.c_void_p())) == -1
    with pytest.raises(ValueError):
        B.BQFlatSearcher(ctx, bv, J.VectorSet(ctx, vecs)).search(queries, VSF.COSINE, 10, 5)   # rerankK < topK
