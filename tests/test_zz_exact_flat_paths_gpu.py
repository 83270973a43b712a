"""The exact flat search's driver (jvector_amd/csrc/exact_flat.cpp) in the form it takes on large inputs, reached at small shapes through
exact_flat_score_bytes: the query chunks of the fused route, a list overflow in a chunk that is not the first, the row chunks and query
groups of the chunked route, the auto plan, the auto gate at 65536 rows, and special values.  The references are those of
test_zz_exact_flat_gpu.py (float64 numpy on small-integer data, the oracle's rescoring); equality is exact, ids and score bits.  Every
case restates the driver's documented chunking rule as a pure function, predicts the launch counts from it and compares them with the
counts of the profile regions `sample` (sample passes) and `exact` (select passes, dense scans, and one rescoring gather per call
with cand_k > 0): a call that silently ran one chunk fails."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd.flat_filtered import pack_accept

import test_zz_exact_flat_gpu as T
from test_zz_exact_flat_gpu import TOPK, VSFS

STATS = ("exact_flat_fused_calls", "exact_flat_fallbacks", "exact_flat_listed")
PREFIX = "exact_flat"
GATE = 65536   # kFusedMinRows


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


# ---------------- the drivers' chunking rules, restated (exact_flat.cpp and nvq_flat.cpp hold the same ones) ----------------
def ceil_div(a, b):
    return -(-a // b)


def fused_plan(Q, N, kc, budget, g=None, cap=None):
    """(g, cap, queries per chunk, chunks) of fused_route: the auto stride and cap, per_q = 4 S + 8 kc + 8 cap + 4"""
    n_tiles = ceil_div(N, 128)
    g = min(g or max(16, ceil_div(N, 1 << 18)), n_tiles)
    cap = min(cap or ceil_div(4 * kc * g, 64) * 64, max(N, 64))
    S = ceil_div(n_tiles, g) * 128
    qc = budget // (4 * S + 8 * kc + 8 * cap + 4)
    if qc >= 128:
        qc = qc // 128 * 128
    qc = min(max(qc, 1), Q)
    return g, cap, qc, ceil_div(Q, qc)


def fused_budget(Q, N, kc, qc, g=None, cap=None):
    """the smallest budget that gives qc queries per chunk"""
    g, cap, _, _ = fused_plan(Q, N, kc, 1, g, cap)
    budget = qc * (4 * ceil_div(ceil_div(N, 128), g) * 128 + 8 * kc + 8 * cap + 4)
    assert fused_plan(Q, N, kc, budget, g, cap)[2] == qc
    return budget


def chunked_plan(Q, N, budget, masked):
    """(rows per chunk C, queries per group qg, row chunks, query groups) of chunked_route"""
    cell = 8 if masked else 4
    C = min(N, 1 << 20)
    qg = budget // (cell * C)
    if qg < 128 and Q > qg:
        qg = min(Q, 128)
        C = min(max(128, budget // (cell * qg) // 128 * 128), N)
    qg = min(max(qg, 1), min(Q, 32768))
    return C, qg, ceil_div(N, C), ceil_div(Q, qg)


DEFAULT_BUDGET = 1 << 30


def run(ctx, search, prefix, stats, opts):
    """one call under the given options (None: unset): the result, the rise of the counters, the launches of `sample` and `exact`"""
    before = [ctx.stat(n) for n in stats]
    for k, v in opts.items():
        ctx.set_option(f"{prefix}_{k}", v)
    ctx.profile(True)
    try:
        got = search()
        launches = ctx.profile_read("sample")[1], ctx.profile_read("exact")[1]
    finally:
        ctx.profile(False)
        for k in opts:
            ctx.set_option(f"{prefix}_{k}", None)
    return (got, [ctx.stat(n) - b for n, b in zip(stats, before)], launches)


def run_exact(ctx, vs, queries, vsf, cand_k, fused=1, g=None, cap=None, budget=None, **kw):
    return run(ctx, lambda: vs.search_exact(queries, vsf, TOPK, cand_k, **kw), PREFIX, STATS,
               {"fused": fused, "sample_stride": g, "cap": cap, "score_bytes": budget})


# ---------------- masks and references, computed once ----------------
@functools.lru_cache(maxsize=None)
def mask(kind, Q, N):
    """(bool mask the reference sees or None, what the call gets, stride in words)"""
    if kind == "none":
        return None, None, 0
    return T.masks(kind, Q, N, np.random.default_rng(3))


def list_lengths(sc, accept, g, kc):
    """per query, the entries the select pass appends: the accepted rows that reach the kc-th best of the accepted sampled rows"""
    Q, N = sc.shape
    sampled = (np.arange(N) // 128) % g == 0
    out = np.zeros(Q, np.int64)
    for q in range(Q):
        acc = np.ones(N, bool) if accept is None else (accept if accept.ndim == 1 else accept[q])
        samp = np.sort(sc[q][acc & sampled])[::-1]
        out[q] = (sc[q][acc] >= (samp[kc - 1] if len(samp) >= kc else -np.inf)).sum()
    return out


@functools.lru_cache(maxsize=None)
def reference(Q, N, D, vsf, cand_k, kind, g):
    """(ids, scores) of T.reference and the per-query list lengths at stride g"""
    m = mask(kind, Q, N)[0]
    wi, ws, longest = T.reference(Q, N, D, vsf, cand_k, m, g)
    lengths = list_lengths(T.ref_scores(Q, N, D, vsf), m, g, cand_k or TOPK)
    assert lengths.max() == longest
    return wi, ws, lengths


def with_base(wi, id_base):
    return np.where(wi >= 0, wi + id_base, -1)


VS = {}


def vectors(ctx, Q, N, D):
    """one device copy of a problem's rows for the module"""
    if (id(ctx), Q, N, D) not in VS:
        VS[id(ctx), Q, N, D] = J.VectorSet(ctx, T.problem(Q, N, D)[0])
    return VS[id(ctx), Q, N, D]


# ---------------- 1. the fused route: query chunks ----------------
# qc = 1: a chunk per query; 50: chunks 50 / 50 / 30, no whole query tile; 128: a whole tile and a chunk of two queries
@pytest.mark.parametrize("Q,N,D,qc", [(33, 2725, 64, 1), (130, 2725, 100, 50), (130, 2725, 100, 128)])
@pytest.mark.parametrize("kind", ["none", "shared", "junk"])
@pytest.mark.parametrize("cand_k", [0, 4 * TOPK])
@pytest.mark.parametrize("vsf", VSFS)
def test_fused_query_chunks(ctx, vsf, cand_k, kind, Q, N, D, qc):
    g, kc = 4, cand_k or TOPK
    _, cap, _, _ = fused_plan(Q, N, kc, DEFAULT_BUDGET, g)
    wi, ws, lengths = reference(Q, N, D, vsf, cand_k, kind, g)
    assert lengths.max() <= cap, "the seed overflows a list: change the seed, not the cap"
    budget = fused_budget(Q, N, kc, qc, g)
    chunks = fused_plan(Q, N, kc, budget, g)[3]
    assert chunks == ceil_div(Q, qc) > 1 and fused_plan(Q, N, kc, DEFAULT_BUDGET, g)[3] == 1
    _, words, stride = mask(kind, Q, N)
    vs, queries = vectors(ctx, Q, N, D), T.problem(Q, N, D)[1]
    kw = dict(g=g, accept=words, accept_stride_words=stride)
    whole, (fused, fallbacks, listed0), launches = run_exact(ctx, vs, queries, vsf, cand_k, **kw)
    assert T.same(whole, (wi, ws)) and (fused, fallbacks) == (1, 0) and launches == (1, 1 + (cand_k > 0))
    got, (fused, fallbacks, listed), launches = run_exact(ctx, vs, queries, vsf, cand_k, budget=budget, **kw)
    assert T.same(got, (wi, ws))
    assert (fused, fallbacks) == (1, 0)
    assert listed == listed0 == lengths.sum()
    assert launches == (chunks, chunks + (cand_k > 0))


# ---------------- 2. a list overflow in a chunk that is not the first ----------------
@pytest.mark.parametrize("cand_k", [0, 4 * TOPK])
@pytest.mark.parametrize("vsf", VSFS)
def test_overflow_in_the_last_chunk(ctx, vsf, cand_k):
    """Q = 33 in chunks of 16 / 16 / 1.  Queries 0 .. 31 accept every row; the last accepts no row of a sampled tile, so its threshold
    is -inf and every row it accepts is listed: the third chunk overflows after two chunks have written their results."""
    Q, N, D, g, qc, kc = 33, 2725, 64, 4, 16, cand_k or TOPK
    m = np.ones((Q, N), bool)
    m[Q - 1] = (np.arange(N) // 128) % g != 0
    _, cap, _, _ = fused_plan(Q, N, kc, DEFAULT_BUDGET, g)
    lengths = list_lengths(T.ref_scores(Q, N, D, vsf), m, g, kc)
    assert lengths[:-1].max() <= cap < lengths[-1] == m[-1].sum(), "only the last query may overflow: change the seed, not the cap"
    wi, ws, _ = T.reference(Q, N, D, vsf, cand_k, m, g)
    budget = fused_budget(Q, N, kc, qc, g)
    assert fused_plan(Q, N, kc, budget, g)[2:] == (16, 3)
    _, _, row_chunks, groups = chunked_plan(Q, N, budget, True)
    got, (fused, fallbacks, listed), launches = run_exact(ctx, vectors(ctx, Q, N, D), T.problem(Q, N, D)[1], vsf, cand_k, g=g,
                                                          budget=budget, accept=pack_accept(m), accept_stride_words=ceil_div(N, 64))
    assert (fused, fallbacks) == (0, 1)
    assert T.same(got, (wi, ws))   # the queries of the first two chunks included
    assert listed == lengths.sum()
    assert launches == (3, 3 + row_chunks * groups + (cand_k > 0))


# ---------------- 3. the chunked route: row chunks and query groups ----------------
def chunked_budget(Q, N, masked, plan):
    cell = 8 if masked else 4
    if plan == "one byte":            # C = 128: 22 chunks, the last of 37 rows (below kc = 40); two query groups at Q = 130
        budget, expect = 1, (128, min(Q, 128), 22, ceil_div(Q, 128))
    elif plan == "C = 512":           # chunks of four tiles, a last chunk of 165 rows
        budget, expect = cell * min(Q, 128) * 512, (512, min(Q, 128), 6, ceil_div(Q, 128))
    else:                             # "two groups": a whole-N chunk for 128 queries, so each group's one top-k is its result
        budget, expect = cell * N * 128, (N, 128, 1, 2)
    assert chunked_plan(Q, N, budget, masked) == expect
    return budget, expect


@pytest.mark.parametrize("Q,N,D,plan", [(33, 2725, 64, "one byte"), (33, 2725, 64, "C = 512"), (130, 2725, 100, "one byte"),
                                        (130, 2725, 100, "two groups")])
@pytest.mark.parametrize("kind", ["none", "shared", "junk", "few"])
@pytest.mark.parametrize("vsf", VSFS)
def test_chunked_row_chunks_and_query_groups(ctx, vsf, kind, Q, N, D, plan):
    budget, (C, qg, row_chunks, groups) = chunked_budget(Q, N, kind != "none", plan)
    assert plan != "one byte" or N - (row_chunks - 1) * C == 37 < 4 * TOPK   # kk < kc where cand_k = 40
    _, words, stride = mask(kind, Q, N)
    vs, queries = vectors(ctx, Q, N, D), T.problem(Q, N, D)[1]
    for cand_k in (0, 4 * TOPK):
        wi, ws, _ = reference(Q, N, D, vsf, cand_k, kind, 1)
        if kind == "few":
            assert (wi[:, 3:] == -1).all() and (wi[:, :3] >= 0).all()   # the merge holds mostly -1
        for id_base in (0, 1000):
            got, (fused, fallbacks, _), launches = run_exact(ctx, vs, queries, vsf, cand_k, fused=-1, budget=budget, accept=words,
                                                             accept_stride_words=stride, id_base=id_base)
            assert T.same(got, (with_base(wi, id_base), ws)), (cand_k, id_base)
            assert (fused, fallbacks) == (0, 0)
            assert launches == (0, row_chunks * groups + (cand_k > 0))


# ---------------- 4. the auto plan at small N ----------------
# N = 2725: stride 16 of 22 tiles (tiles 0 and 16 sampled), cap 4 kc 16; N = 100: the stride clamped to the one tile, cap 64 or N
@pytest.mark.parametrize("Q,N,D", [(33, 2725, 64), (130, 2725, 100), (33, 100, 100)])
@pytest.mark.parametrize("cand_k", [0, 4 * TOPK])
@pytest.mark.parametrize("vsf", VSFS)
def test_auto_plan_at_small_n(ctx, vsf, cand_k, Q, N, D):
    kc = cand_k or TOPK
    g, cap, qc, chunks = fused_plan(Q, N, kc, DEFAULT_BUDGET)
    assert (g, cap) == ((16, min(ceil_div(4 * kc * 16, 64) * 64, N)) if N == 2725 else (1, min(ceil_div(4 * kc, 64) * 64, max(N, 64))))
    assert chunks == 1
    wi, ws, lengths = reference(Q, N, D, vsf, cand_k, "none", g)
    assert lengths.max() <= cap, "the seed overflows a list under the auto plan: change the seed, not the cap"
    got, (fused, fallbacks, listed), launches = run_exact(ctx, vectors(ctx, Q, N, D), T.problem(Q, N, D)[1], vsf, cand_k)
    assert T.same(got, (wi, ws)) and (fused, fallbacks) == (1, 0)
    assert listed == lengths.sum()   # the lists of the stride the rule yields, and of no other
    assert launches == (1, 1 + (cand_k > 0))


# ---------------- 5. the auto gate ----------------
@pytest.mark.parametrize("N,vsf", [(GATE - 1, VSF.EUCLIDEAN), (GATE - 1, VSF.COSINE), (GATE, VSF.DOT_PRODUCT), (GATE, VSF.COSINE)])
def test_auto_gate(ctx, N, vsf):
    """no option set: the chunked route below 65536 rows, the fused route (stride 16, cap 4 kc 16) from there"""
    Q, D, cand_k = 5, 16, 4 * TOPK
    g, cap, _, chunks = fused_plan(Q, N, cand_k, DEFAULT_BUDGET)
    assert (g, cap, chunks) == (16, 2560, 1) and chunked_plan(Q, N, DEFAULT_BUDGET, False)[2:] == (1, 1)
    wi, ws, longest = T.reference(Q, N, D, vsf, cand_k, None, g)
    assert longest <= cap, "the seed overflows a list: change the seed, not the cap"
    vecs, queries = T.problem(Q, N, D)
    got, (fused, fallbacks, _), launches = run_exact(ctx, J.VectorSet(ctx, vecs), queries, vsf, cand_k, fused=None)
    assert T.same(got, (wi, ws))
    assert (fused, fallbacks) == ((1, 0) if N >= GATE else (0, 0))
    assert launches == ((1, 2) if N >= GATE else (0, 2))


# ---------------- 6. special values ----------------
def same_nan(got, want):
    a, b = np.asarray(got[1]), np.asarray(want[1])
    return np.array_equal(got[0], want[0]) and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def special_problem():
    """real-valued rows; six rows (fewer than TOPK) holding a NaN, +inf, -inf and all zeros, none of them in a tile the stride 4 samples"""
    rng = np.random.default_rng(11)
    vecs, queries = rng.standard_normal((2725, 100)).astype(np.float32), rng.standard_normal((130, 100)).astype(np.float32)
    vecs[130, 7], vecs[700, 99], vecs[2500, 0] = np.nan, np.inf, -np.inf
    vecs[300], vecs[1500, 40:42], vecs[2724, 50] = 0, (np.inf, -np.inf), np.nan
    assert all((n // 128) % 4 != 0 for n in (130, 300, 700, 1500, 2500, 2724))
    return vecs, queries


@pytest.mark.parametrize("special_queries", [False, True])
@pytest.mark.parametrize("vsf", VSFS)
def test_special_values_equal_the_composition(ctx, vsf, special_queries):
    """The fused route, the chunked route under a one-byte budget and J.topk over the dense scan agree bit for bit (NaN == NaN) on rows
    holding NaN, infinities and zeros.  Without special queries the lists are shown to fit on the dense scan's own scores, so the select
    epilogue's !(score < tau) is what lets the NaN rows through.  With an all-zero query and a query holding a NaN, a query whose every
    score is a NaN or a tie lists every row: the header lets that send the whole call to the chunked route."""
    vecs, queries = special_problem()
    if special_queries:
        queries = queries.copy()
        queries[3], queries[129, 17] = 0, np.nan
    g, Q, N = 4, len(queries), len(vecs)
    vs = J.VectorSet(ctx, vecs)
    dense = vs.scan(queries, vsf, dense=True)
    for cand_k in (0, 4 * TOPK):
        kc = cand_k or TOPK
        ci, cs = J.topk(ctx, dense, kc)
        want = J.topk(ctx, vs.scores(queries, vsf, ci), TOPK, ids=ci) if cand_k else (ci, cs)
        _, cap, _, _ = fused_plan(Q, N, kc, DEFAULT_BUDGET, g)
        got, (fused, fallbacks, _), _ = run_exact(ctx, vs, queries, vsf, cand_k, g=g)
        assert same_nan(got, want)
        assert fused + fallbacks == 1
        print(f"{vsf.name} cand_k={cand_k} special_queries={special_queries}: fused={fused} fallbacks={fallbacks}")
        if not special_queries:   # the lists on the composition's own scores: the rows that are not below the sample's kc-th best
            sampled = (np.arange(N) // 128) % g == 0
            tau = -np.sort(-dense[:, sampled], axis=1)[:, kc - 1]
            assert np.isfinite(tau).all()
            assert (~(dense < tau[:, None])).sum(1).max() <= cap, "the seed overflows a list: change the seed, not the cap"
            assert (fused, fallbacks) == (1, 0)
        budget, (_, _, row_chunks, groups) = chunked_budget(Q, N, False, "one byte")
        got, (fused, fallbacks, _), launches = run_exact(ctx, vs, queries, vsf, cand_k, fused=-1, budget=budget)
        assert same_nan(got, want)
        assert (fused, fallbacks) == (0, 0) and launches == (0, row_chunks * groups + (cand_k > 0))
