"""NVQ-score graph search on the MI355X (jv_hip_nvq_graph_search through NVQGraphSearcher) against the plain sequential yardstick of
exact_graph_ref.py walked over the CPU oracle's NVQScorer scores of oracle-encoded rows, with no tolerance: ids, score bits and
{visitedCount, expandedCount} are compared with np.array_equal.  The device gets the oracle's bytes and params, so its encoder is not
in the path."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import nvq_graph as NG
from oracle import oracle as O
from bq_graph_yardstick import build_problem
import exact_graph_ref as R

N, Q, K = 600, 9, 10
ALL_VSF = [VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE]
SHAPES = [(5, 1, 16), (33, 5, 16), (100, 3, 80), (64, 1, 16), (256, 8, 16), (768, 2, 16)]


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


class Problem:
    def __init__(self, ctx, seed, n, D, S, degree, levels, edit=None):
        self.v, self.lv, self.entry, self.el, self.q = build_problem(seed, n, D, degree, levels, Q)
        if edit:
            edit(self.v, self.q)
        self.o = O.OracleNVQ.compute(self.v, S)
        self.o.encode_all(self.v)
        self.graph = J.GraphIndex(ctx, n, self.lv, self.entry, self.el)
        self.nv = J.NVQVectors(ctx, J.NVQuantization.create(ctx, self.o.mean, S), self.o.bytes, self.o.params)
        self.searcher = J.NVQGraphSearcher(ctx, self.graph, self.nv)
        self.all = np.tile(np.arange(n, dtype=np.int32), (Q, 1))
        self._S = {}

    def S(self, vsf):
        if int(vsf) not in self._S:
            self._S[int(vsf)] = self.o.scores(self.q, int(vsf), self.all)
        return self._S[int(vsf)]

    def want(self, vsf, k, beam, accept=None, nq=None):
        return R.search(self.S(vsf)[:nq], self.lv, self.entry, self.el, k, beam, accept)

    def got(self, vsf, k, beam, **kw):
        return self.searcher.search(self.q, vsf, k, beam, return_stats=True, **kw)


@pytest.fixture(scope="module")
def problems(ctx):
    cache = {}

    def get(D, S, degree, levels=3, n=N, edit=None):
        key = (D, S, degree, levels, n, edit)
        if key not in cache:
            cache[key] = Problem(ctx, 7100 + D + S + degree + levels, n, D, S, degree, levels, edit)
        return cache[key]
    return get


def same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("beam", [10, 50])
@pytest.mark.parametrize("vsf", ALL_VSF)
@pytest.mark.parametrize("D,S,degree", SHAPES)
def test_parity(ctx, problems, D, S, degree, vsf, beam):
    P = problems(D, S, degree)
    want = P.want(vsf, K, beam)
    assert (want[0] >= 0).all()
    ctx.reset_stats()
    same(P.got(vsf, K, beam), want)
    assert ctx.stat("nvq_gs_calls") == 1 and ctx.stat("nvq_gs_queries") == Q and ctx.stat("nvq_gs_queries_retried") == 0


def test_single_level_graph(ctx, problems):
    P = problems(64, 1, 16, levels=1)
    same(P.got(VSF.COSINE, K, 50), P.want(VSF.COSINE, K, 50))
    same(P.got(VSF.EUCLIDEAN, K, 0), P.want(VSF.EUCLIDEAN, K, 0))   # beamK 0 = topK


def test_one_node(ctx):
    v = np.array([[0.5, -1.0, 2.0, -0.25, 1.0]], np.float32)
    lv = [(None, np.array([[-1]], np.int32))]
    q = np.array([[1.0, 1.0, 1.0, -1.0, 1.0]], np.float32)
    o = O.OracleNVQ(np.zeros(5, np.float32), 2)
    o.encode_all(v)
    nv = J.NVQVectors(ctx, J.NVQuantization.create(ctx, o.mean, 2), o.bytes, o.params)
    s = J.NVQGraphSearcher(ctx, J.GraphIndex(ctx, 1, lv, 0, 0), nv)
    S = o.scores(q, int(VSF.DOT_PRODUCT), np.zeros((1, 1), np.int32))
    assert S[0, 0] > 0
    same(s.search(q, VSF.DOT_PRODUCT, 3, 4, return_stats=True), R.search(S, lv, 0, 0, 3, 4))


def test_filters(ctx, problems):
    P = problems(100, 3, 80)
    rng = np.random.default_rng(11)
    shared, per_query, none = rng.random(N) < 0.25, rng.random((Q, N)) < 0.25, np.zeros(N, bool)
    same(P.got(VSF.DOT_PRODUCT, K, 50, accept=shared), P.want(VSF.DOT_PRODUCT, K, 50, shared))
    got = P.got(VSF.EUCLIDEAN, K, 50, accept=per_query)
    same(got, P.want(VSF.EUCLIDEAN, K, 50, per_query))
    assert all(per_query[i][got[0][i][got[0][i] >= 0]].all() for i in range(Q))
    ids, sc, st = P.got(VSF.EUCLIDEAN, K, 50, accept=none)
    assert (ids == -1).all() and np.isneginf(sc).all() and np.array_equal(st, P.want(VSF.EUCLIDEAN, K, 50, none)[2])


def test_forced_retry_gives_the_same_answer(ctx, problems):
    P = problems(100, 3, 80)
    ctx.set_option("nvq_gs_vcap_log2", 8)
    ctx.set_option("nvq_gs_cand_cap", 128)
    try:
        for vsf in ALL_VSF:
            ctx.reset_stats()
            same(P.got(vsf, K, 50), P.want(vsf, K, 50))
            assert ctx.stat("nvq_gs_queries_retried") > 0
    finally:
        ctx.set_option("nvq_gs_vcap_log2", None)
        ctx.set_option("nvq_gs_cand_cap", None)


def _negative(v, q):
    np.abs(v, out=v)
    q[:] = -0.05 * np.abs(q)
    q[:, 0] = 1.0


def test_negative_scores(ctx, problems):
    P = problems(64, 1, 16, edit=_negative)
    S = P.S(VSF.DOT_PRODUCT)
    assert (S < 0).mean() > 0.25 and (S > 0).mean() > 0.05
    whole = P.want(VSF.DOT_PRODUCT, N, N)   # a list nothing is evicted from: an expanded node it lacks had a negative score
    kept = (whole[0] >= 0).sum(1)
    assert (kept > 0).all() and (whole[2][:, 1] > kept).all()
    same(P.got(VSF.DOT_PRODUCT, N, N), whole)
    for beam in (10, 50):
        got = P.got(VSF.DOT_PRODUCT, K, beam)
        same(got, P.want(VSF.DOT_PRODUCT, K, beam))
        assert not (got[1][got[0] >= 0] < 0).any()


def test_device_tensors_in_and_out(ctx, problems):
    import torch
    P = problems(33, 5, 16)
    ids, sc, st = P.searcher.search(torch.from_numpy(P.q).cuda(), VSF.COSINE, K, 50, return_stats=True)
    torch.cuda.synchronize()
    assert ids.is_cuda and sc.is_cuda
    same((ids.cpu().numpy(), sc.cpu().numpy(), st), P.want(VSF.COSINE, K, 50))
    out_i = torch.empty((Q, K), dtype=torch.int32, device="cuda")
    out_s = torch.empty((Q, K), dtype=torch.float32, device="cuda")
    P.searcher.search(P.q, VSF.COSINE, K, 50, out_ids=out_i, out_scores=out_s)   # host queries, device outputs
    torch.cuda.synchronize()
    same((out_i.cpu().numpy(), out_s.cpu().numpy()), P.want(VSF.COSINE, K, 50)[:2])


@pytest.mark.parametrize("vsf", ALL_VSF)
def test_scores_are_nvq_scores_bits(ctx, problems, vsf):
    P = problems(256, 8, 16)
    ids, sc, _ = P.got(vsf, K, 50)
    assert (ids >= 0).all() and np.array_equal(sc, P.nv.scores(P.q, vsf, ids))


def test_max_beam_k(ctx, problems):
    P = problems(64, 1, 16)
    m = P.searcher.max_beam_k()
    assert m >= 1000
    same(P.searcher.search(P.q[:3], VSF.DOT_PRODUCT, K, m, return_stats=True), P.want(VSF.DOT_PRODUCT, K, m, nq=3))   # beamK above N
    with pytest.raises(UnsupportedError, match="beamK"):
        P.searcher.search(P.q[:3], VSF.DOT_PRODUCT, K, m + 1)


def test_invalid_arguments(ctx, problems):
    P = problems(64, 1, 16)
    lib = NG.lib()
    q = np.ascontiguousarray(P.q[:2])
    ids, sc = np.full((2, K), 77, np.int32), np.full((2, K), 77, np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def call(ctx_h=ctx._h, g=P.graph._h, vh=P.nv._h, qp=vp(q), nq=2, k=K, beam=50, oi=vp(ids), osc=vp(sc), mask=None, stride=0):
        return lib.jv_hip_nvq_graph_search(ctx_h, g, vh, qp, nq, int(VSF.DOT_PRODUCT), k, beam, mask, stride, oi, osc, None)

    INVALID = J._lib.JV_ERR_INVALID
    assert call(ctx_h=None) == INVALID and call(g=None) == INVALID and call(vh=None) == INVALID
    assert call(qp=None) == INVALID and call(oi=None) == INVALID and call(osc=None) == INVALID
    assert call(k=0) == INVALID and call(beam=K - 1) == INVALID and call(nq=-1) == INVALID
    assert call(mask=vp(np.zeros((2, 4), np.uint64)), stride=4) == INVALID
    few = J.NVQVectors(ctx, P.nv.nvq, P.o.bytes[:N - 1], P.o.params[:N - 1])
    assert call(vh=few._h) == INVALID
    h = C.c_void_p()   # a graph without an entry node
    J._lib.check(ctx._lib.jv_hip_graph_create(ctx._h, N, 1, C.byref(h)))
    nb = np.ascontiguousarray(P.lv[0][1])
    J._lib.check(ctx._lib.jv_hip_graph_set_level(ctx._h, h, 0, N, None, vp(nb), nb.shape[1]))
    try:
        assert call(g=h) == INVALID
    finally:
        ctx._lib.jv_hip_graph_destroy(h)
    out = C.c_int()
    assert lib.jv_hip_nvq_graph_max_beam_k(ctx._h, P.graph._h, None) == INVALID
    assert lib.jv_hip_nvq_graph_max_beam_k(None, P.graph._h, C.byref(out)) == INVALID
    assert (ids == 77).all() and (sc == 77).all()   # a refused call leaves the outputs untouched
    assert call(nq=0, qp=None, oi=None, osc=None) == 0 and call() == 0
