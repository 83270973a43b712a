"""The dense route of the flat PQ search under an accept filter on the MI355X (adc_mq_mask_kernel and flat_mask_sample_kernel of
jvector_amd/csrc/k_flat_mask.hip, reached through FlatSearcher.search_filtered) against the CPU oracle of tests/flat_accept_ref.py.
Equality is exact, ids and score bits.  Small N reaches the route through the option flat_acc_dense = 1; every such case asserts that
the counter flat_acc_dense_calls rose, so none of them passes on a library without the route."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from flat_accept_ref import Reference, pack, problem
from oracle import oracle as O


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    _cases.clear()      # the shared problems hold device memory: give it back before the context goes
    gc.collect()
    c.close()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


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
        if oracle:
            opq = O.OraclePQ(D, M, cb)
            codes = self.cv.get(0, N)
            assert np.array_equal(codes, opq.encode_all(self.vecs))
            self.ref = Reference(opq, codes, self.vecs, self.queries)

    def search(self, s, vsf, accept, nq=None, dense=1, r=None, **kw):
        """one filtered search (top 10 of 50) under flat_acc_dense = dense: (ids, scores), dense calls, dense fallbacks"""
        ctx, before = self.ctx, (self.ctx.stat("flat_acc_dense_calls"), self.ctx.stat("flat_acc_dense_fallbacks"))
        ctx.set_option("flat_acc_dense", dense)
        ctx.set_option("flat_acc_dense_r", r)
        try:
            got = s.search_filtered(self.queries[:nq], vsf, 10, 50 if s.vectors is not None else 0, accept, **kw)
        finally:
            ctx.set_option("flat_acc_dense", None)
            ctx.set_option("flat_acc_dense_r", None)
        return got, ctx.stat("flat_acc_dense_calls") - before[0], ctx.stat("flat_acc_dense_fallbacks") - before[1]

    def check(self, vsf, mask, words=None, stride=0, nq=None, rerank=True, r=None, calls=1, fallbacks=0, s=None):
        """a forced search of queries [0, nq) against the oracle; mask: bool [N] or [nq, N]; words: the same mask packed by the test"""
        nq = self.Q if nq is None else nq
        s = s or (self.s_rr if rerank else self.s_nr)
        acc = np.full(nq, -1, np.int64)
        got, dc, df = self.search(s, vsf, mask if words is None else words, nq=nq, r=r, accept_stride_words=stride, accepted_out=acc)
        want = self.ref.search(vsf, 10, 50, mask, id_base=s.id_base, rerank=rerank, queries=range(nq))
        assert np.array_equal(got[0], want[0]), (vsf, np.argwhere(got[0] != want[0])[:4])
        assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), vsf
        assert acc.tolist() == (np.broadcast_to(mask, (nq, self.N)).sum(axis=1)).tolist()
        assert (dc, df) == (calls, fallbacks), (vsf, dc, df)
        return got


_cases = {}


def case(ctx, *key, **kw):
    if key not in _cases:
        _cases[key] = Case(ctx, *key, **kw)
    return _cases[key]


def random_mask(N, density, seed):
    return np.random.default_rng(seed).random(N) < density


@pytest.mark.parametrize("vsf", list(VSF))
@pytest.mark.parametrize("N", [4097, 8191, 8193])
def test_n_at_the_kernels_edges(ctx, N, vsf):
    """4096 rows are one R = 4 tile and the smallest N with valid sample parameters; N is never a multiple of 64"""
    c = case(ctx, 6, N, 64, 16, 5)
    clustered = np.zeros(N, bool)
    clustered[1000:3000] = True         # whole words of zeros on either side
    clustered[N // 64 * 64:] = True     # and every row of the last, partial word
    for rerank in (True, False):
        c.check(vsf, np.ones(N, bool), words=pack(np.ones(N, bool), junk=True), rerank=rerank)
        c.check(vsf, random_mask(N, 0.5, N), rerank=rerank)
        c.check(vsf, clustered, rerank=rerank)


@pytest.mark.parametrize("r", [4, 8])
@pytest.mark.parametrize("D,M,dense", [(64, 32, 1), (96, 48, 1), (192, 96, 1), (48, 24, 0)])
def test_table_slices_and_both_r(ctx, D, M, dense, r):
    """one, three (one-chunk) and three (two-chunk) table slices; one query and M = 24 are shapes the route does not take"""
    c = case(ctx, 2, 9_001, D, M, 6)
    m = random_mask(c.N, 0.3, 21)
    for vsf in VSF:
        c.check(vsf, m, nq=4, r=r, calls=dense)
        c.check(vsf, m, nq=6, r=r, calls=dense, rerank=False)
        c.check(vsf, m, nq=1, r=r, calls=0)


def test_stride_2_and_a_blind_sample(ctx):
    """N = 40 009 and k1 = 50: c_target 4096, S_target 16 384, so stride = 2 (even rows are sampled), S = 20 004, k_s = 2048 and
    cap = 16 384.  A mask of odd rows leaves the sample empty: tau = -inf and every accepted row is a survivor."""
    N = 40_009
    c = case(ctx, 8, N, 64, 16, 5)
    odd = np.arange(N) % 2 == 1
    blind = odd & (np.arange(N) < 30_000)
    assert blind.sum() == 15_000 and odd.sum() == 20_004
    for vsf in VSF:
        c.check(vsf, random_mask(N, 0.5, 81))           # about 4096 survivors per query: far inside [50, 16 384]
        c.check(vsf, blind)                             # 15 000 survivors: the list holds them
        c.check(vsf, odd, calls=0, fallbacks=1)         # 20 004 > cap: the list route answers


def test_per_query_masks_with_junk_at_and_beyond_n(ctx):
    Q, N = 6, 12_801
    c = case(ctx, 4, N, 128, 16, Q)
    masks = np.zeros((Q, N), bool)
    masks[1] = True
    masks[2, 6_000] = True
    for q, density in ((3, 0.2), (4, 0.5), (5, 0.8)):
        masks[q] = random_mask(N, density, q)
    stride = (N + 63) // 64 + 3
    words = pack(masks, junk=True, stride_words=stride)
    for vsf in VSF:
        for rerank in (True, False):
            ids, sc = c.check(vsf, masks, words=words, stride=stride, rerank=rerank)     # count = accepted: no fallback
            assert (ids[0] == -1).all() and np.isneginf(sc[0]).all()
            assert ids[2, 0] == 6_000 and (ids[2, 1:] == -1).all() and np.isneginf(sc[2, 1:]).all()


def test_ties_go_to_the_smaller_accepted_id_and_id_base_to_valid_ids(ctx):
    c = case(ctx, 1, 20_011, 128, 16, 9)
    N = c.N
    first = np.arange(0, N - 1, 7)
    assert np.array_equal(c.vecs[first], c.vecs[first + 1])
    m = np.ones(N, bool)
    m[first[0::2] + 1] = False      # even pairs: only the first of the two
    m[first[1::2]] = False          # odd pairs: only the second
    few = np.zeros(N, bool)
    few[[5, 4_000, 20_010]] = True
    for rerank in (True, False):
        s = J.FlatSearcher(ctx, c.pq, c.cv, c.vs if rerank else None, max_queries=c.Q, id_base=1000)
        for vsf in VSF:
            ids, _ = c.check(vsf, m, s=s, rerank=rerank)
            assert (ids >= 1000).all() and m[ids - 1000].all()
        ids, sc = c.check(VSF.EUCLIDEAN, few, s=s, rerank=rerank)
        assert (ids[:, 3:] == -1).all() and np.isneginf(sc[:, 3:]).all() and (np.sort(ids[:, :3], axis=1) == [1005, 5000, 21010]).all()
    # the best row of a query whose nearest vector is half of a pair is the accepted half
    ids, _ = c.check(VSF.DOT_PRODUCT, m)
    both, _ = c.check(VSF.DOT_PRODUCT, np.ones(N, bool))
    for q in (q for q in range(c.Q) if both[q, 0] % 7 == 0 and both[q, 0] + 1 < N):
        assert both[q, 1] == both[q, 0] + 1 and ids[q, 0] == both[q, 0] + (both[q, 0] // 7 % 2), q


def test_auto_route_takes_dense_masks_only(ctx):
    N = (1 << 18) + 37
    c = case(ctx, 7, N, 64, 16, 4, oracle=False)
    dense, sparse = random_mask(N, 0.6, 91), random_mask(N, 0.001, 92)
    for vsf in VSF:
        for s in (c.s_rr, c.s_nr):
            got, calls, fallbacks = c.search(s, vsf, dense, dense=None)
            assert (calls, fallbacks) == (1, 0), vsf
            want, calls, _ = c.search(s, vsf, dense, dense=-1)
            assert calls == 0 and same(got, want), vsf
            assert c.search(s, vsf, sparse, dense=None)[1] == 0, vsf
