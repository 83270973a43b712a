"""Exact-score graph search on the MI355X (jv_hip_exact_graph_search through ExactGraphSearcher) against the plain sequential
yardstick of exact_graph_ref.py — the CPU oracle's scalar scores walked by a restatement of GraphSearcher — with no tolerance: ids,
score bits and {visitedCount, expandedCount} are compared with np.array_equal.

Negative scores: (1 + s) / 2 cannot round to -0.0 for any s (1 + s is +0.0 when it vanishes and never underflows when halved), nor can
the other two similarities, so the boundary rows of test_negative_scores score exactly +0.0 — kept, while every negative score is not."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import exact_graph as XG
from bq_graph_yardstick import build_problem
import exact_graph_ref as R

N, Q, K = 2000, 33, 10
ALL_VSF = [VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE]


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


class Problem:
    def __init__(self, ctx, seed, n, D, degree, levels, dup=False, device_level0=False, edit=None):
        self.v, self.lv, self.entry, self.el, self.q = build_problem(seed, n, D, degree, levels, Q, dup=dup)
        if edit:
            edit(self.v, self.q)
        if device_level0:
            import torch
            self.keep = torch.from_numpy(np.ascontiguousarray(self.lv[0][1])).cuda()
            self.graph = J.GraphIndex.on_device(ctx, self.keep, self.entry)
        else:
            self.graph = J.GraphIndex(ctx, n, self.lv, self.entry, self.el)
        self.vs = J.VectorSet(ctx, self.v)
        self.searcher = J.ExactGraphSearcher(ctx, self.graph, self.vs)
        self._S = {}

    def S(self, vsf):
        if int(vsf) not in self._S:
            self._S[int(vsf)] = R.score_matrix(vsf, self.q, self.v)
        return self._S[int(vsf)]

    def want(self, vsf, k, beam, accept=None, nq=None):
        return R.search(self.S(vsf)[:nq], self.lv, self.entry, self.el, k, beam, accept)

    def got(self, vsf, k, beam, **kw):
        return self.searcher.search(self.q, vsf, k, beam, return_stats=True, **kw)


@pytest.fixture(scope="module")
def problems(ctx):
    cache = {}

    def get(D, degree, levels=3, n=N, **kw):
        key = (D, degree, levels, n, tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in cache:
            cache[key] = Problem(ctx, 9000 + D + degree + levels, n, D, degree, levels, **kw)
        return cache[key]
    return get


def same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("beam", [10, 50])
@pytest.mark.parametrize("vsf", ALL_VSF)
@pytest.mark.parametrize("degree", [16, 80])
@pytest.mark.parametrize("D", [5, 64, 72, 100, 768])
def test_parity(ctx, problems, D, degree, vsf, beam):
    P = problems(D, degree)
    ctx.reset_stats()
    same(P.got(vsf, K, beam), P.want(vsf, K, beam))
    assert ctx.stat("exact_gs_calls") == 1 and ctx.stat("exact_gs_queries") == Q and ctx.stat("exact_gs_queries_retried") == 0


@pytest.mark.parametrize("device_level0", [False, True])
def test_single_level_graphs(ctx, problems, device_level0):
    P = problems(64, 16, levels=1, device_level0=device_level0)
    same(P.got(VSF.COSINE, K, 50), P.want(VSF.COSINE, K, 50))
    same(P.got(VSF.EUCLIDEAN, K, 0), P.want(VSF.EUCLIDEAN, K, 0))   # beamK 0 = topK


def _copies(v, q):
    v[:] = v[np.arange(len(v)) % 64]   # 64 distinct rows, each some thirty times


def test_ties(ctx, problems):
    P = problems(8, 16, edit=_copies)
    for beam in (10, 50):
        want = P.want(VSF.EUCLIDEAN, K, beam)
        assert all(len(np.unique(s)) < len(s) for s in want[1])   # every query's top K holds equal scores
        same(P.got(VSF.EUCLIDEAN, K, beam), want)


def _negative(v, q):
    np.abs(v, out=v)
    q[:] = -0.05 * np.abs(q)
    q[:, 0] = 1.0
    v[::97] = 0.0
    v[::97, 0] = -1.0   # s = -1 exactly: (1 + s) / 2 = +0.0, the smallest score that is kept


def test_negative_scores(ctx, problems):
    P = problems(64, 16, edit=_negative)
    S = P.S(VSF.DOT_PRODUCT)
    assert (S < 0).mean() > 0.5 and (S == 0).any() and (S > 0).any()
    for beam in (10, 50):
        got = P.got(VSF.DOT_PRODUCT, K, beam)
        same(got, P.want(VSF.DOT_PRODUCT, K, beam))
        assert not (got[1][got[0] >= 0] < 0).any()


def test_filters(ctx, problems):
    P = problems(100, 16)
    rng = np.random.default_rng(11)
    shared, per_query, none = rng.random(N) < 0.25, rng.random((Q, N)) < 0.25, np.zeros(N, bool)
    same(P.got(VSF.DOT_PRODUCT, K, 50, accept=shared), P.want(VSF.DOT_PRODUCT, K, 50, shared))
    got = P.got(VSF.EUCLIDEAN, K, 50, accept=per_query)
    same(got, P.want(VSF.EUCLIDEAN, K, 50, per_query))
    assert all(per_query[i][got[0][i][got[0][i] >= 0]].all() for i in range(Q))
    ids, sc, st = P.got(VSF.EUCLIDEAN, K, 50, accept=none)
    assert (ids == -1).all() and np.isneginf(sc).all() and np.array_equal(st, P.want(VSF.EUCLIDEAN, K, 50, none)[2])


def test_beam_k_beyond_the_reachable_nodes(ctx, problems):
    P = problems(64, 16, levels=2, n=150)
    want = P.want(VSF.EUCLIDEAN, 200, 300)
    assert (want[0][:, 150:] == -1).all()
    same(P.got(VSF.EUCLIDEAN, 200, 300), want)


def test_one_node(ctx):
    v = np.array([[0.5, -1.0, 2.0, -0.25, 1.0]], np.float32)
    lv = [(None, np.array([[-1]], np.int32))]
    q = np.array([[1.0, 1.0, 1.0, -1.0, -1.0]], np.float32)
    s = J.ExactGraphSearcher(ctx, J.GraphIndex(ctx, 1, lv, 0, 0), J.VectorSet(ctx, v))
    same(s.search(q, VSF.DOT_PRODUCT, 3, 4, return_stats=True), R.search(R.score_matrix(VSF.DOT_PRODUCT, q, v), lv, 0, 0, 3, 4))


def test_no_queries(ctx, problems):
    ids, sc = problems(64, 16).searcher.search(np.zeros((0, 64), np.float32), VSF.DOT_PRODUCT, K, 50)
    assert ids.shape == (0, K) and sc.shape == (0, K)


def test_device_tensors_in_and_out(ctx, problems):
    import torch
    P = problems(100, 16)
    ids, sc, st = P.searcher.search(torch.from_numpy(P.q).cuda(), VSF.COSINE, K, 50, return_stats=True)
    torch.cuda.synchronize()
    assert ids.is_cuda and sc.is_cuda
    same((ids.cpu().numpy(), sc.cpu().numpy(), st), P.want(VSF.COSINE, K, 50))
    out_i = torch.empty((Q, K), dtype=torch.int32, device="cuda")
    out_s = torch.empty((Q, K), dtype=torch.float32, device="cuda")
    P.searcher.search(P.q, VSF.COSINE, K, 50, out_ids=out_i, out_scores=out_s)   # host queries, device outputs
    torch.cuda.synchronize()
    same((out_i.cpu().numpy(), out_s.cpu().numpy()), P.want(VSF.COSINE, K, 50)[:2])


def test_forced_retry_gives_the_same_answer(ctx, problems):
    P = problems(100, 80)
    want = P.want(VSF.EUCLIDEAN, K, 50)
    ctx.reset_stats()
    same(P.got(VSF.EUCLIDEAN, K, 50), want)
    assert ctx.stat("exact_gs_queries_retried") == 0
    ctx.set_option("exact_gs_vcap_log2", 8)
    ctx.set_option("exact_gs_cand_cap", 128)
    try:
        ctx.reset_stats()
        same(P.got(VSF.EUCLIDEAN, K, 50), want)
        assert ctx.stat("exact_gs_queries_retried") > 0
    finally:
        ctx.set_option("exact_gs_vcap_log2", None)
        ctx.set_option("exact_gs_cand_cap", None)


def test_max_beam_k(ctx, problems):
    P = problems(64, 16)
    m = P.searcher.max_beam_k()
    assert m >= 1000
    same(P.searcher.search(P.q[:3], VSF.DOT_PRODUCT, K, m, return_stats=True), P.want(VSF.DOT_PRODUCT, K, m, nq=3))
    with pytest.raises(UnsupportedError, match="beamK"):
        P.searcher.search(P.q[:3], VSF.DOT_PRODUCT, K, m + 1)


def test_invalid_arguments(ctx, problems):
    P = problems(64, 16)
    lib = XG.lib()
    q = np.ascontiguousarray(P.q[:2])
    ids, sc = np.full((2, K), 77, np.int32), np.full((2, K), 77, np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def call(ctx_h=ctx._h, g=P.graph._h, vh=P.vs._h, qp=vp(q), nq=2, k=K, beam=50, oi=vp(ids), osc=vp(sc), mask=None, stride=0):
        return lib.jv_hip_exact_graph_search(ctx_h, g, vh, qp, nq, int(VSF.DOT_PRODUCT), k, beam, mask, stride, oi, osc, None)

    INVALID, UNSUPPORTED = J._lib.JV_ERR_INVALID, J._lib.JV_ERR_UNSUPPORTED
    assert call(ctx_h=None) == INVALID and call(g=None) == INVALID and call(vh=None) == INVALID
    assert call(qp=None) == INVALID and call(oi=None) == INVALID and call(osc=None) == INVALID
    assert call(k=0) == INVALID and call(beam=K - 1) == INVALID and call(nq=-1) == INVALID
    assert call(mask=vp(np.zeros((2, 4), np.uint64)), stride=4) == INVALID
    few = J.VectorSet(ctx, P.v[:N - 1])
    assert call(vh=few._h) == INVALID
    h = C.c_void_p()   # a graph without an entry node
    J._lib.check(ctx._lib.jv_hip_graph_create(ctx._h, N, 1, C.byref(h)))
    nb = np.ascontiguousarray(P.lv[0][1])
    J._lib.check(ctx._lib.jv_hip_graph_set_level(ctx._h, h, 0, N, None, vp(nb), nb.shape[1]))
    try:
        assert call(g=h) == INVALID
    finally:
        ctx._lib.jv_hip_graph_destroy(h)
    nvq = J.NVQuantization.compute(ctx, P.vs, 2).encode_all(P.vs).as_vector_set()
    assert call(vh=nvq._h) == UNSUPPORTED
    out = C.c_int()
    assert lib.jv_hip_exact_graph_max_beam_k(ctx._h, P.graph._h, 64, None) == INVALID
    assert lib.jv_hip_exact_graph_max_beam_k(None, P.graph._h, 64, C.byref(out)) == INVALID
    assert (ids == 77).all() and (sc == 77).all()   # a refused call leaves the outputs untouched
    assert call(nq=0, qp=None, oi=None, osc=None) == 0 and call() == 0


def test_scores_are_exact_scores_bits(ctx, problems):
    P = problems(72, 16)
    for vsf in ALL_VSF:
        ids, sc, _ = P.got(vsf, K, 50)
        assert (ids >= 0).all() and np.array_equal(sc, P.vs.scores(P.q, vsf, ids))
