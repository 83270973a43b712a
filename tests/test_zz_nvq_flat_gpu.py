"""The NVQ flat search on the MI355X (jv_hip_nvq_search_flat, include/jvector_nvq_flat.h, through NVQVectors.search_flat): the tile
kernel nvq_select_kernel (jvector_amd/csrc/k_nvq_flat.hip) against the oracle's NVQScorer (ids and score bits, with rescoring) and
against a float64 evaluation of the tile formula on the oracle's de-quantised rows (without)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import nvq_flat
from jvector_amd.flat_filtered import pack_accept
from oracle import oracle as O

TOPK = 10
VSFS = [VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE]
STATS = ("nvq_flat_fused_calls", "nvq_flat_fallbacks")


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def problem(D, S, N, Q):
    """(oracle with encoded rows, queries, de-quantised rows in float64), as test_zz_nvq_gpu.py::test_scores_bit_exact makes them"""
    rng = np.random.default_rng(D + S + N)
    if D % 2 == 0:   # clustered, unit norm
        cen = rng.standard_normal((20, D)).astype(np.float32)
        X = cen[rng.integers(0, 20, N)] + 0.3 * rng.standard_normal((N, D)).astype(np.float32)
        X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    else:
        X = rng.standard_normal((N, D)).astype(np.float32)
    queries = (X[rng.integers(0, N, Q)] + 0.1 * rng.standard_normal((Q, D))).astype(np.float32)
    o = O.OracleNVQ.compute(X, S)
    o.encode_all(X)
    sub = np.repeat(np.arange(S), o.sizes())
    deq, val = O.lib().jvo_nvq_dequantize, np.empty((N, D))
    for n in range(N):
        prm = [[float(x) for x in o.params[n, s]] for s in range(S)]   # min, max, growthRate, midpoint
        val[n] = [deq(int(b), prm[s][2], prm[s][3], prm[s][0], prm[s][1]) for b, s in zip(o.bytes[n], sub)]
    return o, queries, val


@functools.lru_cache(maxsize=None)
def scorer_scores(D, S, N, Q, vsf):
    """NVQScorer's scores of every row: the reference's own bits"""
    o, queries, _ = problem(D, S, N, Q)
    return o.scores(queries, int(vsf), np.tile(np.arange(N, dtype=np.int32), (Q, 1)))


def tile_scores64(D, S, N, Q, vsf):
    """the header's step-1 formula in float64"""
    o, queries, val = problem(D, S, N, Q)
    q, mean = queries.astype(np.float64), o.mean.astype(np.float64)
    if vsf == VSF.DOT_PRODUCT:
        return (1 + q @ val.T + (q @ mean)[:, None]) / 2
    if vsf == VSF.EUCLIDEAN:
        return 1 / (1 + (((q - mean)[:, None, :] - val[None]) ** 2).sum(2))
    b = val + mean
    return (1 + (q @ b.T) / np.linalg.norm(q, axis=1)[:, None] / np.linalg.norm(b, axis=1)[None, :]) / 2


def ref_topk(scores, accept, k):
    """NodeQueue order among the accepted rows: higher score first, ties to the smaller id; a tail of (-1, -inf)"""
    s = np.where(accept, scores, -np.inf).astype(np.float32)
    order = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))[:k]
    return np.where(s[order] > -np.inf, order, -1).astype(np.int32), s[order]


def want(shape, vsf, accept=None, id_base=0):
    """what cand_k = 4 * TOPK must return; asserts on the oracle alone that the candidates cannot miss it"""
    sc, N = scorer_scores(*shape, vsf), shape[2]
    ids, out = [], []
    for q in range(shape[3]):
        acc = np.ones(N, bool) if accept is None else (accept if accept.ndim == 1 else accept[q])
        top = ref_topk(sc[q], acc, 4 * TOPK + 1)[1]
        assert top[4 * TOPK] == -np.inf or top[TOPK - 1] - top[4 * TOPK] > 1e-4, "the seed leaves no gap: change the seed"
        i, s = ref_topk(sc[q], acc, TOPK)
        ids.append(np.where(i >= 0, i + id_base, -1))
        out.append(s)
    return np.stack(ids), np.stack(out)


def run(ctx, nv, queries, vsf, cand_k, fused=None, cap=None, **kw):
    """one call under the given options: (ids, scores), then the rise of the fused-call and fallback counters"""
    before = [ctx.stat(n) for n in STATS]
    opts = {"nvq_flat_fused": fused, "nvq_flat_cap": cap}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        got = nv.search_flat(queries, vsf, TOPK, cand_k, **kw)
    finally:
        for k in opts:
            ctx.set_option(k, None)
    return (got, *[ctx.stat(n) - b for n, b in zip(STATS, before)])


def same(got, wanted):
    return np.array_equal(got[0], wanted[0]) and np.array_equal(np.asarray(got[1]).view(np.int32), wanted[1].view(np.int32))


def device_rows(ctx, shape):
    o, queries, _ = problem(*shape)
    return J.NVQVectors(ctx, J.NVQuantization.create(ctx, o.mean, shape[1]), o.bytes, o.params), queries


# D, S, N, Q: one partial tile, D below a piece boundary and ld padding; sub-vector boundaries inside a thread's piece and a partial last
# tile; a second query tile with idle wavefronts and one row in the last tile; many K chunks; many sub-vectors
SHAPES = [(33, 5, 90, 2), (100, 3, 300, 3), (64, 1, 257, 130), (768, 2, 400, 4), (256, 8, 1000, 9)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("vsf", VSFS)
def test_against_the_scorer_and_float64(ctx, vsf, shape):
    wanted = want(shape, vsf)
    nv, queries = device_rows(ctx, shape)
    for fused in (1, -1):   # N is below the auto gate: both routes are asked for
        got, n_fused, fallbacks = run(ctx, nv, queries, vsf, 4 * TOPK, fused=fused)
        assert same(got, wanted) and (n_fused, fallbacks) == (int(fused == 1), 0)
        # step 1 alone: the scores against float64 (ed_body.h's bound for the tile form), the ids a top-k under that tolerance
        (ids, sc), _, _ = run(ctx, nv, queries, vsf, 0, fused=fused)
        ref = tile_scores64(*shape, vsf)
        for q in range(shape[3]):
            assert len(set(ids[q])) == TOPK and ids[q].min() >= 0
            np.testing.assert_allclose(sc[q], ref[q][ids[q]], rtol=1e-5, atol=0)
            assert np.delete(ref[q], ids[q]).max() <= sc[q].min() * (1 + 1e-5)
            assert (np.diff(sc[q]) <= 0).all()


def masks(kind, Q, N, rng):
    """(bool mask the reference sees, what the call gets, stride in words)"""
    words = (N + 63) // 64
    if kind == "none":
        return None, None, 0
    if kind == "shared":
        m = rng.random(N) < 0.6
        return m, pack_accept(m), 0
    if kind == "tile":   # the second tile of 128 rows rejected as a whole
        m = np.ones(N, bool)
        m[128:256] = False
        return m, pack_accept(m), 0
    if kind == "few":    # fewer accepted rows than TOPK
        m = np.zeros(N, bool)
        m[[5, 130, N - 1]] = True
        return m, pack_accept(m), 0
    m = rng.random((Q, N)) < np.linspace(0.5, 0.9, Q)[:, None]   # per query, a wider stride, junk in the slack words and tail bits
    w = rng.integers(0, 2 ** 63, (Q, words + 2), dtype=np.int64).view(np.uint64)
    w[:, :words] = pack_accept(m)
    w[:, words - 1] |= np.uint64((~((1 << (N % 64)) - 1)) & (2 ** 64 - 1))
    return m, np.ascontiguousarray(w), words + 2


@pytest.mark.parametrize("kind,vsf,id_base", [("none", VSF.DOT_PRODUCT, 0), ("shared", VSF.EUCLIDEAN, 1000), ("junk", VSF.COSINE, 0),
                                              ("tile", VSF.DOT_PRODUCT, 7), ("few", VSF.COSINE, 1000)])
def test_routes_and_masks(ctx, kind, vsf, id_base):
    shape = (100, 3, 300, 3)
    m, words, stride = masks(kind, shape[3], shape[2], np.random.default_rng(3))
    wanted = want(shape, vsf, m, id_base)
    if kind == "few":
        assert (wanted[0][:, 3:] == -1).all() and (wanted[1][:, 3:] == -np.inf).all()
    nv, queries = device_rows(ctx, shape)
    kw = dict(accept=words, accept_stride_words=stride, id_base=id_base)
    fused, n_fused, fallbacks = run(ctx, nv, queries, vsf, 4 * TOPK, fused=1, **kw)
    assert same(fused, wanted) and (n_fused, fallbacks) == (1, 0)
    chunked, n_fused, fallbacks = run(ctx, nv, queries, vsf, 4 * TOPK, fused=-1, **kw)
    assert same(chunked, wanted) and (n_fused, fallbacks) == (0, 0)
    over, n_fused, fallbacks = run(ctx, nv, queries, vsf, 4 * TOPK, fused=1, cap=1, **kw)   # every list overflows
    assert same(over, wanted) and (n_fused, fallbacks) == (0, 1)
    a, _, _ = run(ctx, nv, queries, vsf, 0, fused=1, **kw)   # step 1 alone: the routes agree bit for bit
    b, _, _ = run(ctx, nv, queries, vsf, 0, fused=-1, **kw)
    assert same(a, b)


def test_refusals_leave_the_outputs_untouched(ctx):
    nv, queries = device_rows(ctx, (33, 5, 90, 2))
    ids, sc, lib = np.full((2, TOPK), 77, np.int32), np.full((2, TOPK), 7.0, np.float32), nvq_flat.lib()
    bits = np.zeros(4, np.uint64)

    def call(h=nv._h, c=ctx._h, Q=2, vsf=int(VSF.COSINE), top_k=TOPK, cand_k=0, accept=None, stride=0, oi=ids, osc=sc):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
        return lib.jv_hip_nvq_search_flat(c, h, p(queries), Q, vsf, top_k, cand_k, p(accept), stride, 0, p(oi), p(osc))

    invalid = [dict(c=None), dict(h=None), dict(oi=None), dict(osc=None), dict(top_k=0), dict(cand_k=-1), dict(cand_k=TOPK - 1),
               dict(accept=bits, stride=-1), dict(accept=bits, stride=1), dict(Q=-1), dict(vsf=9)]
    assert [call(**kw) for kw in invalid] == [-1] * len(invalid)   # JV_ERR_INVALID
    assert call(top_k=100000) != 0                                   # the top-k's own refusal
    assert call(Q=0) == 0
    assert (ids == 77).all() and (sc == 7.0).all()
