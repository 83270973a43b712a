"""The flat PQ search under an accept filter on the MI355X (include/jvector_flat_filtered.h through FlatSearcher.search_filtered)
against the CPU oracle: OraclePQ.adc_scores -> mask -> topk -> compare_many -> topk (tests/flat_accept_ref.py).  Equality is exact, ids
and score bits; there is no tolerance anywhere.  The cases are the lettered ones of the feature's issue: mask shapes from empty to all
ones (A), three table slices (B), the shapes the multi-query list kernel takes and those it does not (C), per-query masks with junk at
and beyond N (D), the scan block boundaries (E), list lengths at a workgroup tile +- 1 (F), ties (G), id_base over a short list (H),
chunking (I), device-resident arguments (J), the unfiltered search as the limit (K), an NVQ rerank (L), the errors (M).  The data
generator is the one of tests/test_zz_flat_bq_gpu.py (every seventh vector twice), restated in flat_accept_ref.problem."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import flat_filtered
from jvector_amd.flat_filtered import SCAN_ROWS
from flat_accept_ref import Reference, pack, problem
from oracle import oracle as O


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    _cases.clear()      # the shared problems hold device memory: give it back before the context goes
    gc.collect()
    c.close()


class Case:
    """one problem on the device and its oracle twin"""

    def __init__(self, ctx, seed, N, D, M, Q, oracle=True):
        self.ctx, self.N, self.Q = ctx, N, Q
        self.vecs, self.queries, cb = problem(seed, N, D, M, Q)
        self.pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
        self.vs = J.VectorSet(ctx, self.vecs)
        self.cv = J.PQVectors.encode_and_build(ctx, self.pq, self.vs)
        self.s_rr = J.FlatSearcher(ctx, self.pq, self.cv, self.vs, max_queries=Q)
        self.s_nr = J.FlatSearcher(ctx, self.pq, self.cv, None, max_queries=Q)
        self.ref = None
        if oracle:
            opq = O.OraclePQ(D, M, cb)
            codes = self.cv.get(0, N)
            assert np.array_equal(codes, opq.encode_all(self.vecs))
            self.ref = Reference(opq, codes, self.vecs, self.queries)

    def check(self, vsf, top_k, rerank_k, accept, nq=None, rerank=True, what=None, **kw):
        """one filtered search of queries [0, nq) against the oracle; accept: bool [N] or [nq, N]"""
        nq = self.Q if nq is None else nq
        s = self.s_rr if rerank else self.s_nr
        ids, sc = s.search_filtered(self.queries[:nq], vsf, top_k, rerank_k if rerank else 0, accept, **kw)
        wi, ws = self.ref.search(vsf, top_k, rerank_k, accept, rerank=rerank, queries=range(nq))
        assert np.array_equal(ids, wi), (what, vsf, np.argwhere(ids != wi)[:4])
        assert np.array_equal(sc.view(np.int32), ws.view(np.int32)), (what, vsf)
        return ids, sc


_cases = {}


def case(ctx, *key, **kw):
    if key not in _cases:
        _cases[key] = Case(ctx, *key, **kw)
    return _cases[key]


def random_mask(N, density, seed):
    return np.random.default_rng(seed).random(N) < density


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


# ---- A ----
def masks_a(N):
    rng = np.random.default_rng(11)
    out = {"empty": np.zeros(N, bool), "row 0": np.zeros(N, bool), "row N-1": np.zeros(N, bool), "3 rows": np.zeros(N, bool),
           "37 rows": np.zeros(N, bool), "1 %": rng.random(N) < 0.01, "50 %": rng.random(N) < 0.5, "all ones": np.ones(N, bool)}
    out["row 0"][0] = True
    out["row N-1"][N - 1] = True
    out["3 rows"][rng.choice(N, 3, replace=False)] = True
    out["37 rows"][rng.choice(N, 37, replace=False)] = True
    return out


@pytest.mark.parametrize("rerank", [True, False])
@pytest.mark.parametrize("vsf", list(VSF))
def test_a_shared_masks_from_empty_to_all_ones(ctx, vsf, rerank):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    before = ctx.stat("flat_acc_generic")
    for name, m in masks_a(c.N).items():
        acc = np.full(5, -1, np.int64)
        ids, _ = c.check(vsf, 10, 50, m, nq=5, rerank=rerank, what=name, accepted_out=acc)
        assert acc.tolist() == [int(m.sum())] * 5, name
        assert ((ids >= 0).sum(axis=1) == min(10, int(m.sum()))).all(), name
    assert ctx.stat("flat_acc_generic") == before


# ---- B ----
@pytest.mark.parametrize("Q", [4, 1])
def test_b_three_table_slices(ctx, Q):
    c = case(ctx, 2, 9_001, 192, 96, 4)
    m = random_mask(c.N, 0.3, 21)
    for vsf in VSF:
        c.check(vsf, 10, 50, m, nq=Q)
        c.check(vsf, 10, 50, m, nq=Q, rerank=False)


# ---- C ----
@pytest.mark.parametrize("D,M,N,Q,generic", [(64, 32, 5_000, 3, 0), (48, 24, 5_000, 3, 1), (64, 8, 5_000, 3, 1), (384, 192, 5_000, 4, 0)])
def test_c_shapes_the_list_kernel_takes_and_those_it_does_not(ctx, D, M, N, Q, generic):
    c = case(ctx, 3, N, D, M, Q)
    m = random_mask(N, 0.2, M)
    for vsf in VSF:
        before = ctx.stat("flat_acc_generic"), ctx.stat("flat_acc_calls"), ctx.stat("flat_acc_rows")
        c.check(vsf, 10, 50, m)
        assert ctx.stat("flat_acc_generic") - before[0] == generic
        assert ctx.stat("flat_acc_calls") - before[1] == 1 and ctx.stat("flat_acc_rows") - before[2] == Q * int(m.sum())


# ---- D ----
def test_d_per_query_masks_with_junk_at_and_beyond_n(ctx):
    Q, N = 6, 12_801
    c = case(ctx, 4, N, 128, 16, Q)
    assert N % 64 == 1
    masks = np.zeros((Q, N), bool)
    masks[1] = True
    masks[2, 6_000] = True
    for q, density in ((3, 0.005), (4, 0.2), (5, 0.8)):
        masks[q] = random_mask(N, density, q)
    stride = (N + 63) // 64 + 3
    words = pack(masks, junk=True, stride_words=stride)
    assert words.shape == (Q, stride) and (words[:, -3:] == np.uint64(2 ** 64 - 1)).all() and (words[0, -4] == np.uint64(2 ** 64 - 2))
    for vsf in VSF:
        for rerank in (True, False):
            s = c.s_rr if rerank else c.s_nr
            acc = np.full(Q, -1, np.int64)
            got = s.search_filtered(c.queries, vsf, 10, 50 if rerank else 0, words, accept_stride_words=stride, accepted_out=acc)
            want = c.ref.search(vsf, 10, 50, masks, rerank=rerank)
            assert same(got, want), (vsf, rerank)
            assert acc.tolist() == masks.sum(axis=1).tolist()
            assert (got[0][0] == -1).all() and (got[0][2, 1:] == -1).all() and got[0][2, 0] == 6_000
    # the same masks as booleans (packed by the wrapper, no slack): the same answer
    c.check(VSF.COSINE, 10, 50, masks)


# ---- E ----
def masks_e(N):
    S = SCAN_ROWS
    out = {k: np.zeros(N, bool) for k in ("last block", "first rows", "last rows", "boundary words")}
    out["last block"][3 * S:] = True
    out["first rows"][0::S] = True
    out["last rows"][S - 1::S] = True
    for b in (S, 2 * S, 3 * S):
        out["boundary words"][b - 64: b + 64] = True
    return out


def test_e_scan_block_boundaries(ctx):
    N = 3 * SCAN_ROWS + 65
    assert N <= 50_000
    c = case(ctx, 5, N, 64, 16, 4)
    ms = masks_e(N)
    for name, m in ms.items():
        words = pack(m, junk=True)
        for vsf in (VSF.EUCLIDEAN, VSF.COSINE):
            got = c.s_rr.search_filtered(c.queries, vsf, 10, 50, words)
            assert same(got, c.ref.search(vsf, 10, 50, m)), (name, vsf)
    c.check(VSF.DOT_PRODUCT, 10, 50, np.stack(list(ms.values())))   # and the four as per-query masks


# ---- F ----
@pytest.mark.parametrize("N", [4095, 4096, 4097, 8193])
def test_f_list_lengths_around_a_workgroup_tile(ctx, N):
    c = case(ctx, 6, N, 64, 16, 5)
    for vsf in VSF:
        c.check(vsf, 10, 50, np.ones(N, bool))
        c.check(vsf, 64, 0, np.ones(N, bool), rerank=False)
    ones = pack(np.ones(N, bool), junk=True)                       # the same mask with junk in the tail of its last word
    assert same(c.s_rr.search_filtered(c.queries, VSF.COSINE, 10, 50, ones), c.ref.search(VSF.COSINE, 10, 50, np.ones(N, bool)))


# ---- G ----
def test_g_ties_go_to_the_smaller_accepted_id(ctx):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    N = c.N
    first = np.arange(0, N - 1, 7)
    assert np.array_equal(c.vecs[first], c.vecs[first + 1])
    m = np.ones(N, bool)
    m[first[0::2] + 1] = False      # even pairs: only the first of the two
    m[first[1::2]] = False          # odd pairs: only the second
    for vsf in VSF:
        for rerank in (True, False):
            ids, _ = c.check(vsf, 10, 50, m, rerank=rerank, what="alternating pairs")
            assert m[ids[ids >= 0]].all()
    # queries sit next to data rows: the best row of a query whose nearest vector is half of a pair is the accepted half
    ids, _ = c.check(VSF.DOT_PRODUCT, 10, 50, m)
    both, _ = c.check(VSF.DOT_PRODUCT, 10, 50, np.ones(N, bool))
    paired = [q for q in range(c.Q) if both[q, 0] % 7 == 0 and both[q, 0] + 1 < N]
    for q in paired:
        j = both[q, 0] // 7
        assert both[q, 1] == both[q, 0] + 1 and ids[q, 0] == both[q, 0] + (j % 2), q


# ---- H ----
def test_h_id_base_leaves_the_tail_at_minus_one(ctx):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    m = np.zeros(c.N, bool)
    m[[5, 4_000, 20_010]] = True
    for rerank in (True, False):
        s = J.FlatSearcher(ctx, c.pq, c.cv, c.vs if rerank else None, max_queries=c.Q, id_base=1000)
        got = s.search_filtered(c.queries, VSF.EUCLIDEAN, 10, 50 if rerank else 0, m)
        want = c.ref.search(VSF.EUCLIDEAN, 10, 50, m, id_base=1000, rerank=rerank)
        assert same(got, want)
        assert (got[0][:, 3:] == -1).all() and np.isneginf(got[1][:, 3:]).all()
        assert (np.sort(got[0][:, :3], axis=1) == [1005, 5000, 21010]).all()


# ---- I ----
def test_i_results_do_not_depend_on_the_chunking(ctx):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    shared = random_mask(c.N, 0.5, 31)
    per_query = np.stack([random_mask(c.N, 0.1 + 0.05 * q, 40 + q) for q in range(9)])
    for m in (shared, per_query):
        longest = int(m.sum(axis=-1).max())
        L = max(64, (longest + 63) // 64 * 64)
        one = c.check(VSF.COSINE, 10, 50, m)
        try:
            ctx.set_option("flat_acc_score_bytes", 4 * L * 4)     # four queries per chunk: 4 + 4 + 1
            before = ctx.stat("flat_acc_chunks")
            three = c.check(VSF.COSINE, 10, 50, m)
            assert ctx.stat("flat_acc_chunks") - before == 3
            ctx.set_option("flat_acc_score_bytes", 1)             # never less than one group of four queries
            before = ctx.stat("flat_acc_chunks")
            assert same(c.check(VSF.COSINE, 10, 50, m), one)
            assert ctx.stat("flat_acc_chunks") - before == 3
        finally:
            ctx.set_option("flat_acc_score_bytes", None)
        assert same(one, three)


# ---- J ----
def test_j_device_resident_arguments(ctx):
    import torch
    c = case(ctx, 1, 20_011, 128, 16, 9)
    m = random_mask(c.N, 0.05, 51)
    per_query = np.stack([random_mask(c.N, 0.02 * (q + 1), 60 + q) for q in range(9)])
    dq = torch.from_numpy(c.queries).cuda()
    for masks in (m, per_query):
        host = c.check(VSF.COSINE, 10, 50, masks)
        words = torch.from_numpy(pack(masks).view(np.int64)).cuda()
        oi = torch.full((9, 10), -7, dtype=torch.int32, device="cuda")
        osc = torch.zeros((9, 10), dtype=torch.float32, device="cuda")
        ids, sc = c.s_rr.search_filtered(dq, VSF.COSINE, 10, 50, words, out_ids=oi, out_scores=osc)
        torch.cuda.synchronize()
        assert ids is oi and sc is osc
        assert same((ids.cpu().numpy(), sc.cpu().numpy()), host)


# ---- K ----
@pytest.mark.parametrize("N,Q", [(20_011, 9), ((1 << 18) + 37, 4)])
def test_k_no_mask_and_all_ones_equal_the_unfiltered_search(ctx, N, Q):
    c = case(ctx, 1, 20_011, 128, 16, 9) if N == 20_011 else case(ctx, 7, N, 64, 16, Q, oracle=False)
    ones = pack(np.ones(N, bool), junk=True)
    for vsf in VSF:
        for s, k, rk in ((c.s_rr, 10, 50), (c.s_nr, 50, 0)):
            before = ctx.stat("flat_acc_calls")
            want = s.search(c.queries, vsf, k, rk)
            acc = np.zeros(Q, np.int64)
            assert same(s.search_filtered(c.queries, vsf, k, rk, None, accepted_out=acc), want), vsf
            assert ctx.stat("flat_acc_calls") == before and acc.tolist() == [N] * Q
            assert same(s.search_filtered(c.queries, vsf, k, rk, ones, accepted_out=acc), want), vsf
            assert ctx.stat("flat_acc_calls") == before + 1 and acc.tolist() == [N] * Q


# ---- L ----
def test_l_nvq_backed_rerank(ctx):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    nvq = J.NVQuantization.compute(ctx, c.vs, 2)
    nv = nvq.encode_all(c.vs)
    s = J.FlatSearcher(ctx, c.pq, c.cv, nv.as_vector_set(), max_queries=c.Q)
    for vsf in VSF:
        want = s.search(c.queries, vsf, 10, 50)
        assert same(s.search_filtered(c.queries, vsf, 10, 50, np.ones(c.N, bool)), want), vsf
    # and under a real filter the NVQ rerank returns accepted rows only
    m = random_mask(c.N, 0.1, 71)
    ids, _ = s.search_filtered(c.queries, VSF.COSINE, 10, 50, m)
    assert (ids >= 0).all() and m[ids].all()


# ---- M ----
def test_m_errors_return_their_status_and_leave_the_outputs_untouched(ctx):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    lib = flat_filtered.lib()
    N, Q = c.N, 3
    words = (N + 63) // 64
    other = J.VectorSet(ctx, np.zeros((N, 64), np.float32))       # wrong dimension
    short = J.VectorSet(ctx, c.vecs[:100])                        # fewer vectors than codes
    q = np.ascontiguousarray(c.queries[:Q])
    mask = pack(np.ones(N, bool))
    ids = np.full((Q, 10), -7, np.int32)
    sc = np.full((Q, 10), 3.5, np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    s = c.s_rr

    def call(ctx_h=ctx._h, luts=s.luts._h, codes=c.cv._h, vectors=c.vs._h, queries=q, nq=Q, top_k=10, rerank_k=50, accept=mask, stride=0,
             out_ids=ids, out_scores=sc):
        return lib.jv_hip_search_flat_filtered(ctx_h, luts, codes, vectors, p(queries), nq, int(VSF.COSINE), top_k, rerank_k, p(accept), stride,
                                               0, p(out_ids), p(out_scores), None)

    INVALID = -1
    assert call(ctx_h=None) == INVALID and call(luts=None) == INVALID and call(codes=None) == INVALID
    assert call(out_ids=None) == INVALID and call(out_scores=None) == INVALID and call(queries=None) == INVALID
    assert call(top_k=0) == INVALID and call(top_k=-3) == INVALID
    assert call(rerank_k=-1) == INVALID
    assert call(rerank_k=5) == INVALID                                # rerankK < topK with a rerank
    assert call(stride=-1) == INVALID and call(stride=words - 1) == INVALID
    assert call(vectors=other._h) == INVALID and call(vectors=short._h) == INVALID
    assert call(nq=-1) == INVALID
    assert (ids == -7).all() and (sc == 3.5).all()
    assert call(nq=0, queries=None, out_ids=None, out_scores=None) == 0          # Q == 0 returns at once
    # a k above what the top-k takes: the status of the unfiltered search, outputs untouched
    big_i, big_s = np.full((Q, 9000), -7, np.int32), np.full((Q, 9000), 3.5, np.float32)
    want = ctx._lib.jv_hip_search_flat(ctx._h, s.luts._h, c.cv._h, None, p(q), Q, int(VSF.COSINE), 9000, 0, 0, p(big_i), p(big_s))
    assert want != 0
    assert call(vectors=None, top_k=9000, rerank_k=0, out_ids=big_i, out_scores=big_s) == want
    assert (big_i == -7).all() and (big_s == 3.5).all()
    assert call(rerank_k=5, vectors=None) == 0                         # without a rerank rerankK is not compared with topK
    assert call() == 0 and (ids >= 0).all()
