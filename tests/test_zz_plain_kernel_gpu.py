"""The PLAIN-search instantiation of the register-table bound traversal (gs_body.h "PLAIN", k_gsearch_ubr_plain.hip; option gs_plain,
stat gs_last_plain) on the GPU.  A search without acceptOrds mask, excluded id, query map and speculative touch runs a kernel that has
none of them compiled in; everything else keeps the general kernel.  Three layers, N = 6 000, D = 768, PQ-96, degree 32, 96 queries:
  * unfiltered searches report gs_last_plain == 1 and equal the oracle's sequential GraphSearcher — ids, scores, visitedCount,
    expandedCount — for dot product and cosine, rerankK 1 / 10 / 74 / 150; gs_plain = 0 gives the same bytes from the general kernel;
  * accept bits, gs_prefetch = 1 and the builder's searches with an excluded id report gs_last_plain == 0 and equal the oracle;
  * the rare paths the plain kernel marks unlikely are each driven on it: a 128-key candidate tier at rerankK 150 (partition, spill
    tier, refill), a pinned small LDS tier (tier 2), a small tier-2 table with the growth pool, the retry pass (a query map: the
    general kernel), and the scrambled level 0 that makes deferred queries start over.
The plain kernel has no CPU twin (the lane emulator instantiates the general form): this file is its check."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from oracle import oracle as O
from test_graph_search import build_problem, fused_blocks

D, M, N = 768, 96, 6000
RERANK = (1, 10, 74, 150)
ONE_WAVE = ("gs_wgx", "gs_plain", "gs_prefetch", "gs_cand_cap", "gs_v1_log2", "gs_vcap_log2", "gs_grow", "gs_retry", "gs_defer", "gs_defer_min_level")


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


class Problem:
    def __init__(self, ctx, scramble):
        v, lv, entry, entry_level, cb, q = build_problem(31, N=N, D=D, M=M, deg=32, top_n=400, top_deg=32, levels=3)
        if scramble:   # a random level 0: most deferred queries start over (test_zz_ubr_gpu.py has the argument)
            lv[0] = (None, np.random.default_rng(5).integers(0, N, lv[0][1].shape).astype(np.int32))
        self.q = np.concatenate([q, q[::-1] * 0.5 + q * 0.5, -q[:16]]).astype(np.float32)   # 96 queries
        self.v = v
        self.opq = O.OraclePQ(D, M, cb)
        self.pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
        self.vs = J.VectorSet(ctx, v)
        self.cv = J.PQVectors.encode_and_build(ctx, self.pq, self.vs)
        self.codes = self.cv.get(0, N)
        self.graph = J.GraphIndex(ctx, N, lv, entry, entry_level).set_traversal("device")
        self.fused = J.FusedPQ(ctx, self.pq, fused_blocks(self.codes, lv[0][1]), lv[0][1])
        self.og = O.OracleGraph(N, lv, entry, entry_level)
        self.searcher = J.GraphSearcher(ctx, self.graph, self.pq, self.cv, self.fused, self.vs, max_queries=len(self.q))
        self._want = {}

    def want(self, vsf, top_k, rk, accept=None):
        """the oracle's answer, computed once per case and shared"""
        key = (int(vsf), top_k, rk, accept is not None)
        if key not in self._want:
            self._want[key] = self.og.search(self.opq, self.codes, self.v, self.q, int(vsf), top_k, rk, fused=True, accept=accept)
        return self._want[key]


@pytest.fixture(scope="module")
def prob(ctx):
    return Problem(ctx, scramble=False)


def _options(ctx, **kw):
    for k, val in kw.items():
        ctx.set_option(k, val)


def _clear(ctx):
    for k in ONE_WAVE:
        ctx.set_option(k, None)


def _same(got, want):
    ids, sc, st = got
    wi, ws, wst = want
    return np.array_equal(st, wst) and np.array_equal(ids, wi) and np.array_equal(sc, ws)


@pytest.mark.parametrize("vsf", [VSF.DOT_PRODUCT, VSF.COSINE])
@pytest.mark.parametrize("rk", RERANK)
def test_plain_search_equals_the_oracle_and_the_general_kernel(ctx, prob, vsf, rk):
    top_k = min(10, rk)
    try:
        _options(ctx, gs_wgx=0)
        d0 = ctx.stat("gs_ubr_dropped")
        got = prob.searcher.search(prob.q, vsf, top_k, rk, return_stats=True)
        dropped_plain = ctx.stat("gs_ubr_dropped") - d0
        assert ctx.stat("gs_last_ubr") == 1 and ctx.stat("gs_last_plain") == 1
        assert _same(got, prob.want(vsf, top_k, rk)), (vsf, rk)
        _options(ctx, gs_plain=0)
        d0 = ctx.stat("gs_ubr_dropped")
        gen = prob.searcher.search(prob.q, vsf, top_k, rk, return_stats=True)
        assert ctx.stat("gs_last_ubr") == 1 and ctx.stat("gs_last_plain") == 0
        for a, b in zip(got, gen):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (vsf, rk)
        assert ctx.stat("gs_ubr_dropped") - d0 == dropped_plain   # the same neighbours dropped behind their bound
    finally:
        _clear(ctx)


def test_filtered_and_prefetching_searches_keep_the_general_kernel(ctx, prob):
    try:
        _options(ctx, gs_wgx=0)
        accept = np.ones(N, bool)
        accept[::3] = False
        got = prob.searcher.search(prob.q, VSF.COSINE, 10, 74, return_stats=True, accept=accept)
        assert ctx.stat("gs_last_plain") == 0
        assert _same(got, prob.want(VSF.COSINE, 10, 74, accept=accept))
        for vsf in (VSF.DOT_PRODUCT, VSF.COSINE):
            _options(ctx, gs_prefetch=1)
            got = prob.searcher.search(prob.q, vsf, 10, 74, return_stats=True)
            assert ctx.stat("gs_last_ubr") == 1 and ctx.stat("gs_last_plain") == 0
            assert _same(got, prob.want(vsf, 10, 74)), vsf
            _options(ctx, gs_prefetch=None)
            got = prob.searcher.search(prob.q, vsf, 10, 74, return_stats=True)
            assert ctx.stat("gs_last_plain") == 1 and _same(got, prob.want(vsf, 10, 74)), vsf
    finally:
        _clear(ctx)


def test_searches_with_an_excluded_id_keep_the_general_kernel(ctx):
    """ExcludingBits(node) exists in the builder's own searches only (improveConnections): one node per batch in the reference's order,
    an improve pass over every node — working lists, scores and marks equal the oracle builder's (the yardstick's own assertions) —
    and none of those searches took the plain kernel"""
    import torch
    from test_builder_reference_order import check_reference_order
    try:
        ctx.set_option("gs_wgx", 0)   # (one-node batches would go to the workgroup form)
        check_reference_order(J, ctx, torch.device("cuda", 0), 300, D, M, 16, 40, VSF.COSINE, improve=1)
        assert ctx.stat("gs_last_plain") == 0 and ctx.stat("gs_last_wgx") == 0 and ctx.stat("gs_calls_host") == 0
    finally:
        _clear(ctx)


@pytest.mark.parametrize("name,opts,rk", [
    ("partition, spill tier, refill", dict(gs_cand_cap=128), 150),
    ("tier 2 behind a small LDS tier", dict(gs_v1_log2=7), 150),
    ("growth pool", dict(gs_v1_log2=7, gs_vcap_log2=9, gs_grow=1, gs_retry=1), 150),
    ("retry pass", dict(gs_v1_log2=7, gs_vcap_log2=9, gs_grow=0, gs_retry=1), 150),
])
def test_rare_paths_on_the_plain_kernel(ctx, prob, name, opts, rk):
    try:
        _options(ctx, gs_wgx=0, **opts)
        for vsf in (VSF.DOT_PRODUCT, VSF.COSINE):
            ctx.reset_stats()
            got = prob.searcher.search(prob.q, vsf, 10, rk, return_stats=True)
            assert ctx.stat("gs_last_ubr") == 1 and ctx.stat("gs_last_plain") == 1, name   # (the batch's first launch)
            assert _same(got, prob.want(vsf, 10, rk)), (name, vsf)
            if name == "retry pass":   # the tiny table overflowed in the plain kernel, the query map ran the general one
                assert ctx.stat("gs_queries_retried") > 0 and ctx.stat("gs_queries_host_fallback") == 0
            if name == "growth pool":   # (test_two_tier_visited_set_sizes' pinned sizes: the 512-slot table is outgrown inside the kernel)
                assert ctx.stat("gs_queries_host_fallback") == 0
    finally:
        _clear(ctx)


def test_restarts_of_deferred_queries_on_the_plain_kernel(ctx):
    """the scrambled level 0 of test_deferred_scores_above_level_0_on_the_device: with deferral forced on, queries start over inside
    the plain kernel and the answer is the oracle's"""
    sp = Problem(ctx, scramble=True)
    try:
        _options(ctx, gs_wgx=0, gs_defer=1, gs_defer_min_level=1)
        for vsf in (VSF.DOT_PRODUCT, VSF.COSINE):
            r0 = ctx.stat("gs_defer_restarts")
            got = sp.searcher.search(sp.q, vsf, 10, 40, return_stats=True)
            assert ctx.stat("gs_last_plain") == 1 and ctx.stat("gs_defer_restarts") - r0 > len(sp.q) // 10
            assert _same(got, sp.want(vsf, 10, 40)), vsf
    finally:
        _clear(ctx)
