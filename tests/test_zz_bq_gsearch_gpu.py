"""Graph search over binary-quantized vectors on the MI355X (jv_hip_bq_graph_search through BQGraphSearcher) against the yardstick of
bq_graph_yardstick.py — the oracle's sequential GraphSearcher driven by a sign quantizer, which walks in BQ order exactly — with no
tolerance: ids, scores and {visitedCount, expandedCount} are compared with np.array_equal.  Approximate results carry
BQVectors.similarityBetween in f32; reranked ones the exact scores of the oracle's rerank over the walk's rerankK results."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import bq as B
from jvector_amd import bq_graph as BG
from bq_graph_yardstick import Yardstick, build_problem, np_encode

N, Q, K = 2000, 33, 10
ALL_VSF = [VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE]


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


class Problem:
    def __init__(self, ctx, seed, n, D, degree, levels, nq=Q, dup=False, device_level0=False):
        self.v, self.lv, self.entry, self.el, self.q = build_problem(seed, n, D, degree, levels, nq, dup=dup)
        self.D, self.n = D, n
        self.ys = Yardstick(self.v, self.lv, self.entry, self.el, D)
        if device_level0:
            import torch
            self.keep = torch.from_numpy(np.ascontiguousarray(self.lv[0][1])).cuda()
            self.graph = J.GraphIndex.on_device(ctx, self.keep, self.entry)
        else:
            self.graph = J.GraphIndex(ctx, n, self.lv, self.entry, self.el)
        self.vs = J.VectorSet(ctx, self.v)
        self.bq = B.BinaryQuantization(ctx, D).encode_all(self.vs)
        assert np.array_equal(self.bq.get(), self.ys.words)
        self.approx = BG.BQGraphSearcher(ctx, self.graph, self.bq)
        self.exact = BG.BQGraphSearcher(ctx, self.graph, self.bq, self.vs)
        self._want = {}

    def want_approx(self, k, rk, accept=None, key=None):
        kk = ("a", k, rk, key)
        if accept is not None and key is None:
            return self.ys.approx(self.q, k, rk, accept=accept)
        if kk not in self._want:
            self._want[kk] = self.ys.approx(self.q, k, rk, accept=accept)
        return self._want[kk]

    def want_reranked(self, vsf, k, rk):
        kk = ("r", int(vsf), k, rk)
        if kk not in self._want:
            self._want[kk] = self.ys.reranked(self.q, self.v, vsf, k, rk)
        return self._want[kk]


@pytest.fixture(scope="module")
def problems(ctx):
    cache = {}

    def get(D, degree, levels=3, **kw):
        key = (D, degree, levels, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Problem(ctx, 7000 + D + degree + levels, kw.pop("n", N), D, degree, levels, **kw)
        return cache[key]
    return get


def same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("rk", [10, 50])
@pytest.mark.parametrize("degree", [16, 80])
@pytest.mark.parametrize("D", [64, 100, 768])
def test_approximate_parity(ctx, problems, D, degree, rk):
    P = problems(D, degree)
    ctx.reset_stats()
    same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, rk, return_stats=True), P.want_approx(K, rk))
    assert ctx.stat("bq_gs_calls") == 1 and ctx.stat("bq_gs_queries") == Q and ctx.stat("bq_gs_queries_retried") == 0


@pytest.mark.parametrize("vsf", ALL_VSF)
@pytest.mark.parametrize("rk", [10, 50])
@pytest.mark.parametrize("degree", [16, 80])
@pytest.mark.parametrize("D", [64, 100, 768])
def test_reranked_parity(ctx, problems, D, degree, rk, vsf):
    P = problems(D, degree)
    same(P.exact.search(P.q, vsf, K, rk, return_stats=True), P.want_reranked(vsf, K, rk))


def test_single_level_graph(ctx, problems):
    P = problems(100, 16, levels=1)
    same(P.approx.search(P.q, VSF.EUCLIDEAN, K, 50, return_stats=True), P.want_approx(K, 50))
    same(P.exact.search(P.q, VSF.COSINE, K, 50, return_stats=True), P.want_reranked(VSF.COSINE, K, 50))


def test_caller_owned_device_level0(ctx, problems):
    P = problems(64, 16, levels=1, device_level0=True)
    same(P.approx.search(P.q, VSF.EUCLIDEAN, K, 50, return_stats=True), P.want_approx(K, 50))
    same(P.exact.search(P.q, VSF.DOT_PRODUCT, K, 50, return_stats=True), P.want_reranked(VSF.DOT_PRODUCT, K, 50))


def test_ties(ctx, problems):
    P = problems(7, 16, dup=True)
    for rk in (10, 50):
        want = P.want_approx(K, rk)
        assert all(len(np.unique(s)) < len(s) for s in want[1])   # every query's top K holds equal scores
        same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, rk, return_stats=True), want)


def test_filters(ctx, problems):
    P = problems(100, 16)
    rng = np.random.default_rng(11)
    shared = rng.random(N) < 0.25
    per_query = rng.random((Q, N)) < 0.25
    same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, 50, accept=shared, return_stats=True), P.want_approx(K, 50, accept=shared))
    same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, 50, accept=per_query, return_stats=True), P.want_approx(K, 50, accept=per_query))
    got = P.exact.search(P.q, VSF.EUCLIDEAN, K, 50, accept=per_query, return_stats=True)
    same(got, P.ys.reranked(P.q, P.v, VSF.EUCLIDEAN, K, 50, accept=per_query))
    for i in range(Q):
        assert per_query[i][got[0][i][got[0][i] >= 0]].all()
    none = np.zeros(N, bool)
    ids, sc, st = P.approx.search(P.q, VSF.DOT_PRODUCT, K, 50, accept=none, return_stats=True)
    assert (ids == -1).all() and np.isneginf(sc).all()
    # nothing is ever kept, so the walk has no stop rule to apply: the counters of the yardstick's own run under the same mask
    assert np.array_equal(st, P.want_approx(K, 50, accept=none)[2])


def test_one_node(ctx):
    v = np.array([[0.5, -1.0, 2.0, -0.25, 1.0]], np.float32)
    lv = [(None, np.array([[-1]], np.int32))]
    graph = J.GraphIndex(ctx, 1, lv, 0, 0)
    vs = J.VectorSet(ctx, v)
    bqv = B.BinaryQuantization(ctx, 5).encode_all(vs)
    q = np.array([[1.0, 1.0, 1.0, -1.0, -1.0]], np.float32)
    ids, sc, st = BG.BQGraphSearcher(ctx, graph, bqv).search(q, VSF.DOT_PRODUCT, 3, 4, return_stats=True)
    assert ids.tolist() == [[0, -1, -1]] and st.tolist() == [[0, 1]]
    assert sc[0, 0] == np.float32(1) - np.float32(2) / np.float32(5) and np.isneginf(sc[0, 1:]).all()
    same(BG.BQGraphSearcher(ctx, graph, bqv, vs).search(q, VSF.DOT_PRODUCT, 1, 1, return_stats=True),
         Yardstick(v, lv, 0, 0, 5).reranked(q, v, VSF.DOT_PRODUCT, 1, 1))


def test_rerank_k_beyond_the_reachable_nodes(ctx, problems):
    P = problems(64, 16, n=150, levels=2)
    want = P.want_approx(200, 300)
    assert (want[0][:, 150:] == -1).all()
    same(P.approx.search(P.q, VSF.DOT_PRODUCT, 200, 300, return_stats=True), want)
    same(P.exact.search(P.q, VSF.EUCLIDEAN, 200, 300, return_stats=True), P.want_reranked(VSF.EUCLIDEAN, 200, 300))


def test_no_queries(ctx, problems):
    P = problems(64, 16)
    ids, sc = P.approx.search(np.zeros((0, 64), np.float32), VSF.DOT_PRODUCT, K, 50)
    assert ids.shape == (0, K) and sc.shape == (0, K)


def test_device_tensors_in_and_out(ctx, problems):
    import torch
    P = problems(100, 16)
    dq = torch.from_numpy(P.q).cuda()
    ids, sc, st = P.exact.search(dq, VSF.COSINE, K, 50, return_stats=True)
    torch.cuda.synchronize()
    assert ids.is_cuda and sc.is_cuda
    same((ids.cpu().numpy(), sc.cpu().numpy(), st), P.want_reranked(VSF.COSINE, K, 50))
    out_i = torch.empty((Q, K), dtype=torch.int32, device="cuda")
    out_s = torch.empty((Q, K), dtype=torch.float32, device="cuda")
    P.approx.search(P.q, VSF.COSINE, K, 50, out_ids=out_i, out_scores=out_s)   # host queries, device outputs
    torch.cuda.synchronize()
    same((out_i.cpu().numpy(), out_s.cpu().numpy()), P.want_approx(K, 50)[:2])


def test_max_rerank_k(ctx, problems):
    P = problems(64, 16)
    m = P.approx.max_rerank_k()
    assert m >= 1000
    same(P.approx.search(P.q[:3], VSF.DOT_PRODUCT, K, m, return_stats=True), [a[:3] for a in P.ys.approx(P.q[:3], K, m)])
    with pytest.raises(UnsupportedError, match="rerankK"):
        P.approx.search(P.q[:3], VSF.DOT_PRODUCT, K, m + 1)


def test_invalid_arguments(ctx, problems):
    P = problems(64, 16)
    lib = BG.lib()
    q = np.ascontiguousarray(P.q[:2])
    ids, sc = np.empty((2, K), np.int32), np.empty((2, K), np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def call(ctx_h=ctx._h, g=P.graph._h, bqh=P.bq._h, vh=None, qp=vp(q), nq=2, k=K, rk=50, oi=vp(ids), osc=vp(sc)):
        return lib.jv_hip_bq_graph_search(ctx_h, g, bqh, vh, qp, nq, int(VSF.DOT_PRODUCT), k, rk, None, 0, oi, osc, None)

    assert call() == 0
    JV_ERR_INVALID = J._lib.JV_ERR_INVALID
    assert call(ctx_h=None) == JV_ERR_INVALID and call(g=None) == JV_ERR_INVALID and call(bqh=None) == JV_ERR_INVALID
    assert call(qp=None) == JV_ERR_INVALID and call(oi=None) == JV_ERR_INVALID and call(osc=None) == JV_ERR_INVALID
    assert call(k=0) == JV_ERR_INVALID and call(k=K, rk=K - 1) == JV_ERR_INVALID and call(nq=-1) == JV_ERR_INVALID
    assert call(nq=0, qp=None, oi=None, osc=None) == 0   # Q == 0 returns at once
    out = C.c_int()
    assert lib.jv_hip_bq_graph_max_rerank_k(ctx._h, P.graph._h, None) == JV_ERR_INVALID
    assert lib.jv_hip_bq_graph_max_rerank_k(None, P.graph._h, C.byref(out)) == JV_ERR_INVALID
    rng = np.random.default_rng(0)
    other_d = J.VectorSet(ctx, rng.standard_normal((N, 65)).astype(np.float32))
    few_vecs = J.VectorSet(ctx, P.v[:N - 1])
    few_rows = B.BinaryQuantization(ctx, 64).encode_all(few_vecs)
    with pytest.raises(ValueError, match="dimension"):
        BG.BQGraphSearcher(ctx, P.graph, P.bq, other_d).search(q, VSF.DOT_PRODUCT, K, 50)
    with pytest.raises(ValueError, match="vectors for a graph"):
        BG.BQGraphSearcher(ctx, P.graph, P.bq, few_vecs).search(q, VSF.DOT_PRODUCT, K, 50)
    with pytest.raises(ValueError, match="BQ rows for a graph"):
        BG.BQGraphSearcher(ctx, P.graph, few_rows).search(q, VSF.DOT_PRODUCT, K, 50)
    with pytest.raises(ValueError, match="accept_stride_words"):
        mask = np.zeros((2, 4), np.uint64)
        J._lib.check(lib.jv_hip_bq_graph_search(ctx._h, P.graph._h, P.bq._h, None, vp(q), 2, int(VSF.DOT_PRODUCT), K, 50, vp(mask), 4,
                                                vp(ids), vp(sc), None))
    # a graph without an entry node
    h = C.c_void_p()
    J._lib.check(ctx._lib.jv_hip_graph_create(ctx._h, N, 1, C.byref(h)))
    nb = np.ascontiguousarray(P.lv[0][1])
    J._lib.check(ctx._lib.jv_hip_graph_set_level(ctx._h, h, 0, N, None, vp(nb), nb.shape[1]))
    try:
        with pytest.raises(ValueError, match="entry"):
            J._lib.check(call(g=h))
    finally:
        ctx._lib.jv_hip_graph_destroy(h)


def test_retry_gives_the_same_answer(ctx, problems):
    P = problems(100, 80)
    want_a, want_r = P.want_approx(K, 50), P.want_reranked(VSF.EUCLIDEAN, K, 50)
    ctx.reset_stats()
    same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, 50, return_stats=True), want_a)
    assert ctx.stat("bq_gs_queries_retried") == 0
    ctx.set_option("bq_gs_vcap_log2", 8)
    ctx.set_option("bq_gs_cand_cap", 128)
    try:
        ctx.reset_stats()
        same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, 50, return_stats=True), want_a)
        assert ctx.stat("bq_gs_queries_retried") > 0
        same(P.exact.search(P.q, VSF.EUCLIDEAN, K, 50, return_stats=True), want_r)
        # a roomy table with the smallest candidate storage: the spill slice is what overflows (or the partition / refill paths run)
        ctx.set_option("bq_gs_vcap_log2", 13)
        same(P.approx.search(P.q, VSF.DOT_PRODUCT, K, 50, return_stats=True), want_a)
    finally:
        ctx.set_option("bq_gs_vcap_log2", None)
        ctx.set_option("bq_gs_cand_cap", None)
