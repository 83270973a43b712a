"""Build-time scoring over binary-quantized vectors on the MI355X (include/jvector_bq_build.h through BQBuildScorer), bit for bit
against the yardsticks of bq_build_yardstick.py: the numpy restatement of retainDiverse / isDiverse over BQ rows for the batched
prune (selections, n_selected, short_edges with NaN equal to NaN), and the oracle's sequential GraphSearcher driven by a sign
quantizer (bq_graph_yardstick.Yardstick.approx on the nodes' own vectors) for the node-seeded search (ids, BQ similarities, both
counters).  The CPU twin, on the lane emulator, is tests/test_bq_build_emulated.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import UnsupportedError
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import bq as B
from jvector_amd import bq_build as BB
from jvector_amd import bq_graph as BG
from bq_graph_yardstick import Yardstick, build_problem, np_encode
from bq_build_yardstick import candidate_lists, pair_similarity, retain_diverse, same, self_mask

N, P = 2000, 37


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


# ---------------------------------------------------------------- prune ----------------------------------------------------------------

class Rows:
    def __init__(self, ctx, D, dup=False):
        v = np.random.default_rng(900 + D).standard_normal((N, D)).astype(np.float32)
        if dup:
            v[N // 2:] = v[:N - N // 2]
        self.D = D
        self.words = np_encode(v, D)
        self.bq = B.BinaryQuantization(ctx, D).encode_all(J.VectorSet(ctx, v))
        assert np.array_equal(self.bq.get(), self.words)
        self.scorer = BB.BQBuildScorer(ctx, None, self.bq)
        self._lists = {}

    def lists(self, Cn, n_nodes=P, seed=0):
        key = (Cn, n_nodes, seed)
        if key not in self._lists:
            self._lists[key] = candidate_lists(self.words, self.D, n_nodes, Cn, 31 * self.D + Cn + seed)
        return self._lists[key]

    def check(self, nodes, scores, max_degree, alpha, **kw):
        same(self.scorer.retain_diverse(nodes, scores, max_degree, alpha, **kw),
             retain_diverse(self.words, self.D, nodes, scores, max_degree, alpha, **kw))


@pytest.fixture(scope="module")
def rows(ctx):
    cache = {}

    def get(D, dup=False):
        if (D, dup) not in cache:
            cache[(D, dup)] = Rows(ctx, D, dup)
        return cache[(D, dup)]
    return get


@pytest.mark.parametrize("max_degree", [1, 8, 32, 64])
@pytest.mark.parametrize("Cn", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("D", [64, 100, 768, 1000])
def test_prune_parity(rows, D, Cn, max_degree):
    R = rows(D)
    nodes, scores = R.lists(Cn)
    for alpha in (1.0, 1.2, 1.4):
        R.check(nodes, scores, max_degree, alpha)


def test_prune_generic_row_width(rows):
    R = rows(300)   # five words: no build of its own
    for Cn, md in ((65, 32), (200, 64)):
        nodes, scores = R.lists(Cn)
        R.check(nodes, scores, md, 1.2)


@pytest.mark.parametrize("D", [64, 100, 768])
def test_the_prune_cases_are_not_vacuous(rows, D):
    R = rows(D)
    nodes, scores = R.lists(65)
    sel, cnt, _ = retain_diverse(R.words, D, nodes, scores, 32, 1.0)
    not_prefix = sum(1 for p in range(P) if not np.array_equal(sel[p, :cnt[p]], np.arange(cnt[p])))
    assert 2 * not_prefix >= P, not_prefix
    _, cnt2, _ = retain_diverse(R.words, D, nodes, scores, 32, 1.2)
    assert (cnt2 > cnt).any()


def test_prune_loop_that_never_runs(rows):
    R = rows(100)
    nodes, scores = R.lists(65)
    before = np.full(P, 3, np.int32)
    sel, cnt, se = R.scorer.retain_diverse(nodes, scores, 8, 0.9, diverse_before=before)
    assert np.isnan(se).all() and (cnt == 3).all() and (sel[:, :3] == np.arange(3)).all() and (sel[:, 3:] == -1).all()
    R.check(nodes, scores, 8, 0.9, diverse_before=before)
    R.check(nodes, scores, 8, 0.9)


@pytest.mark.parametrize("max_degree", [8, 32])
def test_prune_ragged_counts_and_diverse_before(rows, max_degree):
    R = rows(100)
    nodes, scores = R.lists(65)
    rng = np.random.default_rng(1)
    count = rng.integers(0, 66, P).astype(np.int32)
    count[:4] = [0, 1, 65, 70]
    before = np.resize(np.array([0, 3, max_degree, max_degree + 2], np.int32), P)
    for alpha in (1.0, 1.2):
        R.check(nodes, scores, max_degree, alpha, cand_count=count)
        R.check(nodes, scores, max_degree, alpha, diverse_before=before)
        R.check(nodes, scores, max_degree, alpha, cand_count=count, diverse_before=before)


def test_prune_repeated_ids_bad_ordinals_and_arbitrary_scores(rows):
    R = rows(768)
    nodes, scores = (a.copy() for a in R.lists(65))
    rng = np.random.default_rng(2)
    for p in range(P):
        a, b = rng.choice(65, 2, replace=False)
        nodes[p, b] = nodes[p, a]   # an id listed twice
    for alpha in (1.0, 1.2, 1.4):
        R.check(nodes, scores, 32, alpha)
    for p in range(P):
        nodes[p, rng.integers(0, 65)] = -1
        nodes[p, rng.integers(0, 65)] = -1
        nodes[p, rng.integers(0, 65)] = N
    for alpha in (1.0, 1.4):
        R.check(nodes, scores, 32, alpha)
    wild = rng.standard_normal(scores.shape).astype(np.float32)   # unsorted, negative
    wild[:, 7] = -np.inf
    wild[:, 19] = np.inf
    wild[:, 23] = np.nan
    for alpha in (1.0, 1.4):
        R.check(nodes, wild, 32, alpha)
        R.check(nodes, wild, 64, alpha)


def test_prune_ties_and_the_strict_comparison(rows):
    R = rows(64, dup=True)
    nodes, scores = R.lists(65)
    hits = sum(int((pair_similarity(R.words, 64, int(nodes[p, i]), nodes[p, :i]) == scores[p, i]).any()) for p in range(P) for i in range(1, 65))
    assert hits > 0   # sim == score * alpha at alpha = 1: the strict > decides
    for md in (8, 32):
        for alpha in (1.0, 1.2):
            R.check(nodes, scores, md, alpha)


def test_prune_device_tensors(rows):
    import torch
    R = rows(100)
    nodes, scores = R.lists(65)
    count = np.random.default_rng(3).integers(0, 66, P).astype(np.int32)
    before = np.resize(np.array([0, 2], np.int32), P)
    dev = [torch.from_numpy(a).cuda() for a in (nodes, scores, count, before)]
    sel, cnt, se = R.scorer.retain_diverse(dev[0], dev[1], 32, 1.2, cand_count=dev[2], diverse_before=dev[3])
    torch.cuda.synchronize()
    assert sel.is_cuda and cnt.is_cuda and se.is_cuda
    same((sel.cpu().numpy(), cnt.cpu().numpy(), se.cpu().numpy()),
         retain_diverse(R.words, 100, nodes, scores, 32, 1.2, cand_count=count, diverse_before=before))


def test_prune_blocks_stride_over_many_nodes(rows):
    R = rows(64)
    nodes, scores = R.lists(8, n_nodes=5000, seed=5)
    R.check(nodes, scores, 4, 1.2)


def test_prune_limits(ctx, rows):
    R = rows(768)
    m = R.scorer.max_candidates(32)
    assert 200 <= m <= 4096
    nodes, scores = R.lists(m, n_nodes=3, seed=9)
    R.check(nodes, scores, 32, 1.2)
    nodes1 = np.zeros((3, m + 1), np.int32)
    with pytest.raises(UnsupportedError, match="candidates"):
        R.scorer.retain_diverse(nodes1, np.zeros((3, m + 1), np.float32), 32, 1.2)
    with pytest.raises(UnsupportedError, match="maxDegree"):
        R.scorer.retain_diverse(nodes[:, :8], scores[:, :8], 65, 1.2)
    assert rows(64).scorer.max_candidates(8) > m


def test_prune_invalid_arguments(ctx, rows):
    R = rows(64)
    lib = BB.lib()
    nodes, scores = (np.ascontiguousarray(a[:2]) for a in R.lists(8, n_nodes=5000, seed=5))
    sel, cnt = np.empty((2, 4), np.int32), np.empty(2, np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def call(ctx_h=ctx._h, bqh=R.bq._h, np_=2, cn=8, n=vp(nodes), s=vp(scores), md=4, so=vp(sel), co=vp(cnt)):
        return lib.jv_hip_bq_retain_diverse(ctx_h, bqh, np_, cn, n, s, None, None, md, C.c_float(1.2), so, co, None)

    inv = J._lib.JV_ERR_INVALID
    assert call() == 0
    assert call(ctx_h=None) == inv and call(bqh=None) == inv and call(np_=-1) == inv and call(cn=0) == inv and call(md=0) == inv
    assert call(n=None) == inv and call(s=None) == inv and call(so=None) == inv and call(co=None) == inv
    assert call(np_=0, n=None, s=None, so=None, co=None) == 0   # P == 0 returns at once
    out = C.c_int()
    assert lib.jv_hip_bq_retain_diverse_max_candidates(ctx._h, R.bq._h, 8, None) == inv
    assert lib.jv_hip_bq_retain_diverse_max_candidates(None, R.bq._h, 8, C.byref(out)) == inv


def test_prune_alpha_range(ctx, rows):
    # the rounds are a loop on the device and an f32 stepped by 0.2f stops moving at 2^22: alpha above 64 is refused, as in
    # jv_hip_retain_diverse; 64 itself runs all its rounds on lists that never fill maxDegree; NaN and alpha < 1 mean no round
    R = rows(100)
    nodes, scores = (a.copy() for a in R.lists(5, n_nodes=4, seed=11))
    scores[:, 1:] = -np.inf
    nodes[1, 2] = -1
    count = np.array([0, 1, 5, 3], np.int32)
    for alpha in (65.0, 64.001, 1e6, 4194304.0, 1e30, np.inf):
        with pytest.raises(ValueError, match="alpha"):
            R.scorer.retain_diverse(nodes, scores, 8, alpha)
        with pytest.raises(ValueError, match="alpha"):
            R.scorer.retain_diverse(nodes, scores, 8, alpha, cand_count=count)
    want = retain_diverse(R.words, 100, nodes, scores, 8, 64.0)
    assert (want[1] < 8).all()
    same(R.scorer.retain_diverse(nodes, scores, 8, 64.0), want)
    R.check(nodes, scores, 8, 64.0, cand_count=count)
    for alpha in (np.nan, -np.inf, 0.0):
        sel, cnt, se = R.scorer.retain_diverse(nodes, scores, 8, alpha)
        assert np.isnan(se).all() and (cnt == 0).all() and (sel == -1).all()


# ---------------------------------------------------------------- node-seeded search ----------------------------------------------------------------

Q = 33


class Problem:
    def __init__(self, ctx, seed, D, degree, levels, device_level0=False):
        self.v, self.lv, self.entry, self.el, self.q = build_problem(seed, N, D, degree, levels, 5)
        self.D = D
        self.ys = Yardstick(self.v, self.lv, self.entry, self.el, D)
        if device_level0:
            import torch
            self.keep = torch.from_numpy(np.ascontiguousarray(self.lv[0][1])).cuda()
            self.graph = J.GraphIndex.on_device(ctx, self.keep, self.entry)
        else:
            self.graph = J.GraphIndex(ctx, N, self.lv, self.entry, self.el)
        self.vs = J.VectorSet(ctx, self.v)
        self.bq = B.BinaryQuantization(ctx, D).encode_all(self.vs)
        self.scorer = BB.BQBuildScorer(ctx, self.graph, self.bq)
        nodes = np.random.default_rng(seed).choice(N, Q, replace=False).astype(np.int32)
        nodes[0] = self.entry
        nodes[5] = nodes[4]   # a repeated ordinal
        self.nodes = nodes
        self._want = {}

    def want(self, k, exclude):
        if (k, exclude) not in self._want:
            self._want[(k, exclude)] = self.ys.approx(self.v[self.nodes], k, k, accept=self_mask(self.nodes, N) if exclude else None)
        return self._want[(k, exclude)]


@pytest.fixture(scope="module")
def problems(ctx):
    cache = {}

    def get(D, degree, levels=3, **kw):
        key = (D, degree, levels, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = Problem(ctx, 8000 + D + degree + levels, D, degree, levels, **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("k", [10, 50])
@pytest.mark.parametrize("levels", [3, 1])
@pytest.mark.parametrize("degree", [16, 80])
@pytest.mark.parametrize("D", [64, 100, 768])
def test_search_nodes_parity(ctx, problems, D, degree, levels, k):
    Pb = problems(D, degree, levels)
    ctx.reset_stats()
    plain = Pb.want(k, False)
    same(Pb.scorer.search_nodes(Pb.nodes, k, return_stats=True), plain)
    assert ctx.stat("bq_gs_calls") == 1 and ctx.stat("bq_gs_queries") == Q and ctx.stat("bq_gs_queries_retried") == 0
    assert any(Pb.nodes[q] in plain[0][q] for q in range(Q))   # the exclusion has something to exclude
    got = Pb.scorer.search_nodes(Pb.nodes, k, exclude_self=True, return_stats=True)
    same(got, Pb.want(k, True))   # counters included: the self node is visited and expanded like a rejected node
    assert not any(Pb.nodes[q] in got[0][q] for q in range(Q))


def test_search_nodes_retry_gives_the_same_answer(ctx, problems):
    Pb = problems(100, 80)
    ctx.set_option("bq_gs_vcap_log2", 8)
    ctx.set_option("bq_gs_cand_cap", 128)
    try:
        ctx.reset_stats()
        same(Pb.scorer.search_nodes(Pb.nodes, 50, return_stats=True), Pb.want(50, False))
        assert ctx.stat("bq_gs_queries_retried") > 0
        ctx.reset_stats()
        same(Pb.scorer.search_nodes(Pb.nodes, 50, exclude_self=True, return_stats=True), Pb.want(50, True))
        assert ctx.stat("bq_gs_queries_retried") > 0
    finally:
        ctx.set_option("bq_gs_vcap_log2", None)
        ctx.set_option("bq_gs_cand_cap", None)


def test_search_nodes_caller_owned_device_level0(ctx, problems):
    Pb = problems(64, 16, levels=1, device_level0=True)
    same(Pb.scorer.search_nodes(Pb.nodes, 50, return_stats=True), Pb.want(50, False))
    same(Pb.scorer.search_nodes(Pb.nodes, 50, exclude_self=True, return_stats=True), Pb.want(50, True))


def test_search_nodes_device_tensors_and_bad_ordinals(ctx, problems):
    import torch
    Pb = problems(100, 16)
    dn = torch.from_numpy(Pb.nodes).cuda()
    ids, sc, st = Pb.scorer.search_nodes(dn, 10, exclude_self=True, return_stats=True)
    torch.cuda.synchronize()
    assert ids.is_cuda and sc.is_cuda
    same((ids.cpu().numpy(), sc.cpu().numpy(), st), Pb.want(10, True))
    bad = Pb.nodes.copy()
    bad[7], bad[20] = N, -1
    with pytest.raises(ValueError, match="ordinal"):
        Pb.scorer.search_nodes(bad, 10)
    # device ordinals are not brought back to be checked: such an item gets an empty row and zero counters, the others are untouched
    ids, sc, st = Pb.scorer.search_nodes(torch.from_numpy(bad).cuda(), 10, return_stats=True)
    torch.cuda.synchronize()
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    want = Pb.want(10, False)
    ok = np.ones(Q, bool)
    ok[[7, 20]] = False
    same((ids[ok], sc[ok], st[ok]), [w[ok] for w in want])
    assert (ids[~ok] == -1).all() and np.isneginf(sc[~ok]).all() and (st[~ok] == 0).all()


def test_search_nodes_invalid_arguments(ctx, problems):
    Pb = problems(64, 16)
    lib = BB.lib()
    nodes = np.ascontiguousarray(Pb.nodes[:2])
    ids, sc = np.empty((2, 10), np.int32), np.empty((2, 10), np.float32)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def call(ctx_h=ctx._h, g=Pb.graph._h, bqh=Pb.bq._h, n=vp(nodes), nq=2, k=10, oi=vp(ids), osc=vp(sc)):
        return lib.jv_hip_bq_graph_search_nodes(ctx_h, g, bqh, n, nq, k, 0, oi, osc, None)

    inv = J._lib.JV_ERR_INVALID
    assert call() == 0
    assert call(ctx_h=None) == inv and call(g=None) == inv and call(bqh=None) == inv and call(n=None) == inv
    assert call(oi=None) == inv and call(osc=None) == inv and call(k=0) == inv and call(nq=-1) == inv
    assert call(nq=0, n=None, oi=None, osc=None) == 0
    few = B.BinaryQuantization(ctx, 64).encode_all(J.VectorSet(ctx, Pb.v[:N - 1]))
    with pytest.raises(ValueError, match="BQ rows for a graph"):
        BB.BQBuildScorer(ctx, Pb.graph, few).search_nodes(nodes, 10)
    m = BG.BQGraphSearcher(ctx, Pb.graph, Pb.bq).max_rerank_k()
    with pytest.raises(UnsupportedError, match="rerankK"):
        Pb.scorer.search_nodes(nodes, m + 1)


def test_float_query_search_is_what_it_was(ctx, problems):
    # guard on the refactor of jv_hip_bq_graph_search around the shared second half
    Pb = problems(100, 16)
    s = BG.BQGraphSearcher(ctx, Pb.graph, Pb.bq)
    ctx.reset_stats()
    same(s.search(Pb.q, VSF.DOT_PRODUCT, 10, 50, return_stats=True), Pb.ys.approx(Pb.q, 10, 50))
    assert ctx.stat("bq_gs_calls") == 1 and ctx.stat("bq_gs_queries") == len(Pb.q) and ctx.stat("bq_gs_queries_retried") == 0
    e = BG.BQGraphSearcher(ctx, Pb.graph, Pb.bq, Pb.vs)
    same(e.search(Pb.q, VSF.EUCLIDEAN, 10, 50, return_stats=True), Pb.ys.reranked(Pb.q, Pb.v, VSF.EUCLIDEAN, 10, 50))
    acc = np.random.default_rng(4).random((len(Pb.q), N)) < 0.3
    same(s.search(Pb.q, VSF.DOT_PRODUCT, 10, 50, accept=acc, return_stats=True), Pb.ys.approx(Pb.q, 10, 50, accept=acc))
