"""The exact flat search on the MI355X (jv_hip_search_exact, include/jvector_exact_flat.h, through VectorSet.search_exact): the fused
route's exact_select_kernel (jvector_amd/csrc/k_exact_flat.hip) against a plain float64 numpy reference on small-integer data, where
every f32 chain is exact, and against the composition it replaces on real-valued data.  Equality is exact: ids and score bits."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import exact_flat
from jvector_amd.flat_filtered import pack_accept
from oracle import oracle as O

TOPK = 10
VSFS = [VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE]


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def problem(Q, N, D, seed=7):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, (N, D)).astype(np.float32), rng.integers(-8, 9, (Q, D)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ref_scores(Q, N, D, vsf):
    """float64 dot products and norms (exact on these integers), then ed_finish's last operations in float32"""
    vecs, queries = problem(Q, N, D)
    v, q = vecs.astype(np.float64), queries.astype(np.float64)
    dot, qn, vn = q @ v.T, (q * q).sum(1)[:, None], (v * v).sum(1)[None, :]
    assert qn.max() * vn.max() < 2 ** 24 and qn.min() > 0 and vn.min() > 0
    f = np.float32
    if vsf == VSF.EUCLIDEAN:
        return f(1) / (f(1) + np.maximum(qn + vn - 2 * dot, 0).astype(f))
    if vsf == VSF.COSINE:
        dot = (dot / np.sqrt((qn * vn).astype(f).astype(np.float64))).astype(f)
    return (f(1) + dot.astype(f)) / f(2)


def ref_topk(scores, ids, k):
    """stable sort by (-score, id); a tail of (-1, -inf)"""
    order = np.lexsort((ids, -scores.astype(np.float64)))[:k]
    oi, osc = np.full(k, -1, np.int32), np.full(k, -np.inf, np.float32)
    oi[:len(order)], osc[:len(order)] = ids[order], scores[order]
    return oi, osc


def reference(Q, N, D, vsf, cand_k, accept=None, g=1):
    """(ids, scores) as the call must return them, and the longest list the select pass may build"""
    vecs, queries = problem(Q, N, D)
    sc, kc = ref_scores(Q, N, D, vsf), cand_k or TOPK
    sampled = (np.arange(N) // 128) % g == 0
    want_i, want_s, longest = [], [], 0
    for q in range(Q):
        acc = np.ones(N, bool) if accept is None else (accept if accept.ndim == 1 else accept[q])
        ids = np.flatnonzero(acc).astype(np.int32)
        samp = np.sort(sc[q][acc & sampled])[::-1]
        longest = max(longest, int((sc[q][ids] >= (samp[kc - 1] if len(samp) >= kc else -np.inf)).sum()))
        ci, cs = ref_topk(sc[q][ids], ids, kc)
        if cand_k:   # step 2: the bit-exact scalar-order scores of the candidates (the oracle's), then the top-k
            ci = ci[ci >= 0]
            ci, cs = ref_topk(O.compare_many(int(vsf), queries[q], vecs[ci]), ci, TOPK)
        want_i.append(ci)
        want_s.append(cs)
    return np.stack(want_i), np.stack(want_s), longest


def run(ctx, vs, queries, vsf, cand_k, fused=1, g=None, cap=None, **kw):
    """one call under the given options: (ids, scores), then the rise of the fused-call, fallback and listed counters"""
    names = ("exact_flat_fused_calls", "exact_flat_fallbacks", "exact_flat_listed")
    before = [ctx.stat(n) for n in names]
    opts = {"exact_flat_fused": fused, "exact_flat_sample_stride": g, "exact_flat_cap": cap}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        got = vs.search_exact(queries, vsf, TOPK, cand_k, **kw)
    finally:
        for k in opts:
            ctx.set_option(k, None)
    return (got, *[ctx.stat(n) - b for n, b in zip(names, before)])


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(np.asarray(got[1]).view(np.int32), want[1].view(np.int32))


def check(ctx, Q, N, D, vsf, cand_k, ref_accept=None, id_base=0, **kw):
    g = 4 if N > 128 else 1
    wi, ws, longest = reference(Q, N, D, vsf, cand_k, ref_accept, g)
    assert longest <= (4 * (cand_k or TOPK) * g + 63) // 64 * 64, "the seed overflows a list: change the seed, not the cap"
    vecs, queries = problem(Q, N, D)
    vs = J.VectorSet(ctx, vecs)
    got, fused, fallbacks, listed = run(ctx, vs, queries, vsf, cand_k, g=g, id_base=id_base, **kw)
    assert same(got, (np.where(wi >= 0, wi + id_base, -1), ws))
    assert fused == 1 and fallbacks == 0
    return listed


# Q: one query, a partial second wavefront, a second query tile; N: one partial tile, 21 tiles and 37 rows; D: below a K chunk and no
# multiple of 4, a multiple of the chunk, several chunks and a partial one
@pytest.mark.parametrize("Q,N,D", [(1, 100, 30), (33, 2725, 64), (130, 2725, 100), (130, 100, 64), (33, 100, 100), (1, 2725, 30)])
@pytest.mark.parametrize("cand_k", [0, 4 * TOPK])
@pytest.mark.parametrize("vsf", VSFS)
def test_integer_data_against_float64(ctx, vsf, cand_k, Q, N, D):
    listed = check(ctx, Q, N, D, vsf, cand_k, id_base=1000 if (Q, D) == (33, 64) else 0)
    if N == 2725:
        assert listed < Q * N   # the threshold acted


def masks(kind, Q, N, rng):
    """(bool mask the reference sees, what the call gets, stride in words)"""
    words = (N + 63) // 64
    if kind == "shared":
        m = rng.random(N) < 0.5
        m[128:384] = False   # two whole tiles rejected
        return m, pack_accept(m), 0
    if kind == "zero":
        return np.zeros(N, bool), np.zeros(words, np.uint64), 0
    if kind == "few":
        m = np.zeros(N, bool)
        m[[5, 700, 2724]] = True
        return m, pack_accept(m), 0
    m = rng.random((Q, N)) < np.linspace(0.02, 0.9, Q)[:, None]
    if kind == "perq":
        return m, pack_accept(m), words
    w = rng.integers(0, 2 ** 63, (Q, words + 2), dtype=np.int64).view(np.uint64)   # junk: slack words, and bits at and beyond N
    w[:, :words] = pack_accept(m)
    w[:, words - 1] |= np.uint64((~((1 << (N % 64)) - 1)) & (2 ** 64 - 1))
    return m, np.ascontiguousarray(w), words + 2


@pytest.mark.parametrize("device_mask", [False, True])
@pytest.mark.parametrize("kind,vsf,cand_k", [("shared", VSF.EUCLIDEAN, 40), ("perq", VSF.COSINE, 0), ("zero", VSF.DOT_PRODUCT, 0),
                                             ("few", VSF.DOT_PRODUCT, 40), ("junk", VSF.EUCLIDEAN, 40)])
def test_masks(ctx, kind, vsf, cand_k, device_mask):
    import torch
    Q, N, D = 33, 2725, 64
    m, words, stride = masks(kind, Q, N, np.random.default_rng(3))
    accept = torch.from_numpy(words.view(np.int64)).cuda() if device_mask else words
    check(ctx, Q, N, D, vsf, cand_k, ref_accept=m, accept=accept, accept_stride_words=stride)


@pytest.mark.parametrize("vsf", VSFS)
def test_real_data_equals_the_composition(ctx, vsf):
    rng = np.random.default_rng(11)
    vecs, queries = rng.standard_normal((2725, 100)).astype(np.float32), rng.standard_normal((130, 100)).astype(np.float32)
    vs = J.VectorSet(ctx, vecs)
    ci, cs = J.topk(ctx, vs.scan(queries, vsf, dense=True), 4 * TOPK)
    for cand_k, want in ((0, (ci[:, :TOPK], cs[:, :TOPK])), (4 * TOPK, J.topk(ctx, vs.scores(queries, vsf, ci), TOPK, ids=ci))):
        got, fused, fallbacks, _ = run(ctx, vs, queries, vsf, cand_k, g=4)
        assert same(got, want) and fused == 1 and fallbacks == 0
        chunked, fused, fallbacks, _ = run(ctx, vs, queries, vsf, cand_k, fused=-1)
        assert same(chunked, want) and fused == 0 and fallbacks == 0


def test_list_overflow_takes_the_chunked_route(ctx):
    vecs = np.tile(np.arange(1, 31, dtype=np.float32), (2725, 1))
    queries = np.ones((3, 30), np.float32)
    got, fused, fallbacks, _ = run(ctx, J.VectorSet(ctx, vecs), queries, VSF.DOT_PRODUCT, 0, g=4, cap=TOPK)
    assert (fused, fallbacks) == (0, 1)
    assert np.array_equal(got[0], np.tile(np.arange(TOPK, dtype=np.int32), (3, 1)))
    assert np.array_equal(got[1], np.full((3, TOPK), (1 + 465) / 2, np.float32))


def test_refusals_leave_the_outputs_untouched(ctx):
    vecs, queries = problem(33, 100, 30)
    vs = J.VectorSet(ctx, vecs)
    nvq = J.NVQuantization.compute(ctx, vs, 2).encode_all(vs).as_vector_set()
    ids, sc, lib = np.full((33, TOPK), 77, np.int32), np.full((33, TOPK), 7.0, np.float32), exact_flat.lib()
    bits = np.zeros(4, np.uint64)

    def call(h=vs._h, c=ctx._h, Q=33, top_k=TOPK, cand_k=0, accept=None, stride=0, oi=ids, osc=sc):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
        return lib.jv_hip_search_exact(c, h, p(queries), Q, int(VSF.COSINE), top_k, cand_k, p(accept), stride, 0, p(oi), p(osc))

    invalid = [dict(c=None), dict(h=None), dict(oi=None), dict(osc=None), dict(top_k=0), dict(cand_k=-1), dict(cand_k=TOPK - 1),
               dict(accept=bits, stride=-1), dict(accept=bits, stride=1), dict(Q=-1)]
    assert [call(**kw) for kw in invalid] == [-1] * len(invalid)   # JV_ERR_INVALID
    assert call(h=nvq._h) == -5                                      # JV_ERR_UNSUPPORTED
    assert call(top_k=100000) != 0                                   # the top-k's own refusal
    assert call(Q=0) == 0
    assert (ids == 77).all() and (sc == 7.0).all()
