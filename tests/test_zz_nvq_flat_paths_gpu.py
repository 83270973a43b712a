"""The NVQ flat search's driver (jvector_amd/csrc/nvq_flat.cpp) in the form it takes on large inputs, reached at small shapes through
nvq_flat_score_bytes: the query chunks of the fused route, a list overflow in a chunk that is not the first, the row chunks and query
groups of the chunked route (nvq_select_kernel as a dense scan at tile_offset != 0 and with S below tiles * 128), and the auto gate at
65536 rows.  The references are those of test_zz_nvq_flat_gpu.py: with cand_k = 4 * TOPK the oracle's NVQScorer bits in NodeQueue order
(its gap condition asserted on the oracle alone), with cand_k = 0 the float64 tile formula within ed_body.h's 1e-5 and bit equality
with the same call under the default budget.  The chunking rules and the launch counting are test_zz_exact_flat_paths_gpu.py's: the
two drivers share them."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd.flat_filtered import pack_accept
from oracle import oracle as O

import test_zz_exact_flat_paths_gpu as P
import test_zz_nvq_flat_gpu as T
from test_zz_exact_flat_paths_gpu import DEFAULT_BUDGET, GATE, ceil_div, chunked_plan, fused_budget, fused_plan
from test_zz_nvq_flat_gpu import TOPK, VSFS

STATS = ("nvq_flat_fused_calls", "nvq_flat_fallbacks", "nvq_flat_listed")
A, B, C4, D8 = (100, 3, 300, 3), (64, 1, 257, 130), (768, 2, 400, 4), (256, 8, 1000, 9)   # D, S, N, Q


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


def run_nvq(ctx, nv, queries, vsf, cand_k, fused=1, g=None, cap=None, budget=None, **kw):
    return P.run(ctx, lambda: nv.search_flat(queries, vsf, TOPK, cand_k, **kw), "nvq_flat", STATS,
                 {"fused": fused, "sample_stride": g, "cap": cap, "score_bytes": budget})


@functools.lru_cache(maxsize=None)
def mask(kind, Q, N):
    return T.masks(kind, Q, N, np.random.default_rng(3))


@functools.lru_cache(maxsize=None)
def tile64(shape, vsf):
    return T.tile_scores64(*shape, vsf)


@functools.lru_cache(maxsize=None)
def wanted(shape, vsf, kind):
    return T.want(shape, vsf, mask(kind, shape[3], shape[2])[0])


def with_base(w, id_base):
    return np.where(w[0] >= 0, w[0] + id_base, -1), w[1]


ROWS = {}


def device_rows(ctx, shape):
    if (id(ctx), shape) not in ROWS:
        ROWS[id(ctx), shape] = T.device_rows(ctx, shape)
    return ROWS[id(ctx), shape]


def accept_of(m, q, N):
    return np.ones(N, bool) if m is None else (m if m.ndim == 1 else m[q])


def list_bounds(sc, m, g, kc):
    """per query, (lower, upper) bounds of the select pass's list length from the scorer's scores: the tile scores lie within 1e-5 of
    them (ed_body.h's bound), so a row's score and the threshold together move by at most 2e-5 of the largest score"""
    Q, N = sc.shape
    sampled = (np.arange(N) // 128) % g == 0
    lo, hi = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    for q in range(Q):
        acc = accept_of(m, q, N)
        samp = np.sort(sc[q][acc & sampled].astype(np.float64))[::-1]
        tau, tol = (samp[kc - 1] if len(samp) >= kc else -np.inf), 2e-5 * np.abs(sc[q]).max()
        lo[q], hi[q] = (sc[q][acc] >= tau + tol).sum(), (sc[q][acc] >= tau - tol).sum()
    return lo, hi


def check_float64(shape, vsf, m, got):
    """step 1 alone: the scores against float64 (ed_body.h's bound for the tile form), the ids a top-k under that tolerance"""
    ref, (ids, sc) = tile64(shape, vsf), got
    for q in range(shape[3]):
        acc = accept_of(m, q, shape[2])
        k = min(TOPK, int(acc.sum()))
        i, s = ids[q][:k], sc[q][:k]
        assert (ids[q][k:] == -1).all() and (sc[q][k:] == -np.inf).all()
        assert len(set(i)) == k and i.min() >= 0 and acc[i].all()
        np.testing.assert_allclose(s, ref[q][i], rtol=1e-5, atol=0)
        rest = acc.copy()
        rest[i] = False
        assert not rest.any() or ref[q][rest].max() <= s.min() + 1e-5 * abs(s.min())
        assert (np.diff(s) <= 0).all()


# ---------------- 1. the fused route: query chunks ----------------
# A: a chunk per query and 2 + 1; B: 50 / 50 / 30 and a whole query tile + 2; C4 (N >= 400, many K chunks): a chunk per query and 3 + 1
@pytest.mark.parametrize("shape,qc", [(A, 1), (A, 2), (B, 50), (B, 128), (C4, 1), (C4, 3)])
@pytest.mark.parametrize("kind", ["none", "shared", "junk"])
@pytest.mark.parametrize("vsf", VSFS)
def test_fused_query_chunks(ctx, vsf, kind, shape, qc):
    N, Q = shape[2:]
    m, words, stride = mask(kind, Q, N)
    nv, queries = device_rows(ctx, shape)
    kw = dict(accept=words, accept_stride_words=stride)
    for cand_k in (0, 4 * TOPK):
        kc = cand_k or TOPK
        g, cap, _, _ = fused_plan(Q, N, kc, DEFAULT_BUDGET)
        longest = list_bounds(T.scorer_scores(*shape, vsf), m, g, kc)[1].max()
        assert longest <= cap, "the seed overflows a list: change the seed, not the cap"
        budget = fused_budget(Q, N, kc, qc)
        chunks = fused_plan(Q, N, kc, budget)[3]
        assert chunks == ceil_div(Q, qc) > 1
        whole, (fused, fallbacks, listed0), launches = run_nvq(ctx, nv, queries, vsf, cand_k, **kw)
        assert (fused, fallbacks) == (1, 0) and launches == (1, 1 + (cand_k > 0))
        got, (fused, fallbacks, listed), launches = run_nvq(ctx, nv, queries, vsf, cand_k, budget=budget, **kw)
        assert T.same(got, whole), cand_k
        if cand_k:
            assert T.same(got, wanted(shape, vsf, kind))
        else:
            check_float64(shape, vsf, m, got)
        assert (fused, fallbacks) == (1, 0)
        assert listed == listed0
        assert launches == (chunks, chunks + (cand_k > 0)), cand_k


# ---------------- 2. a list overflow in a chunk that is not the first ----------------
@pytest.mark.parametrize("cand_k", [0, 4 * TOPK])
@pytest.mark.parametrize("vsf", VSFS)
def test_overflow_in_the_last_chunk(ctx, vsf, cand_k):
    """Shape A in chunks of one query under a cap of 64.  Queries 0 and 1 accept 50 rows each: their lists cannot exceed 50.  Query 2
    accepts rows 128 .. 299 only, none of the one sampled tile: its threshold is -inf and all 172 are listed.  The third chunk overflows
    after two chunks have written their results."""
    shape, cap, kc = A, 64, cand_k or TOPK
    N, Q = shape[2:]
    rng = np.random.default_rng(5)
    m = np.zeros((Q, N), bool)
    m[0, rng.permutation(N)[:50]] = m[1, rng.permutation(N)[:50]] = True
    m[2, 128:] = True
    g = fused_plan(Q, N, kc, DEFAULT_BUDGET, cap=cap)[0]
    assert g == 3 and m[:2].sum(1).max() <= cap < m[2].sum() and not m[2, :128].any()   # only the last query overflows, whatever the scores
    budget = fused_budget(Q, N, kc, 1, cap=cap)
    assert fused_plan(Q, N, kc, budget, cap=cap)[2:] == (1, 3)
    _, _, row_chunks, groups = chunked_plan(Q, N, budget, True)
    nv, queries = device_rows(ctx, shape)
    got, (fused, fallbacks, _), launches = run_nvq(ctx, nv, queries, vsf, cand_k, cap=cap, budget=budget, accept=pack_accept(m),
                                                   accept_stride_words=ceil_div(N, 64))
    assert (fused, fallbacks) == (0, 1)
    assert launches == (3, 3 + row_chunks * groups + (cand_k > 0))
    if cand_k:
        assert T.same(got, T.want(shape, vsf, m))   # the queries of the first two chunks included
    else:
        check_float64(shape, vsf, m, got)
        whole, (fused, fallbacks, _), _ = run_nvq(ctx, nv, queries, vsf, 0, fused=-1, accept=pack_accept(m),
                                                  accept_stride_words=ceil_div(N, 64))
        assert T.same(got, whole) and (fused, fallbacks) == (0, 0)


# ---------------- 3. the chunked route: row chunks and query groups ----------------
def chunked_budget(Q, N, masked, plan):
    cell = 8 if masked else 4
    if plan == "one byte":     # C = 128: the dense scan at tile_offset 1, 2, ...; S = the last chunk's rows, below the tile
        budget, expect = 1, (128, min(Q, 128), ceil_div(N, 128), ceil_div(Q, 128))
    elif plan == "C = 256":    # chunks of two tiles: tile_offset 2, 4, 6
        budget, expect = cell * min(Q, 128) * 256, (256, min(Q, 128), ceil_div(N, 256), ceil_div(Q, 128))
    else:                      # "two groups": a whole-N chunk for 128 queries, so each group's one top-k is its result
        budget, expect = cell * N * 128, (N, 128, 1, 2)
    assert chunked_plan(Q, N, budget, masked) == expect
    return budget, expect


# last chunks: A 44 rows; B one row (kk = 1 < kc) in two query groups; C4 16 rows (kk < kc = 40); D8 232 rows of two tiles
@pytest.mark.parametrize("shape,plan", [(A, "one byte"), (B, "one byte"), (C4, "one byte"), (D8, "C = 256"), (B, "two groups")])
@pytest.mark.parametrize("kind", ["none", "shared", "junk", "few"])
@pytest.mark.parametrize("vsf", VSFS)
def test_chunked_row_chunks_and_query_groups(ctx, vsf, kind, shape, plan):
    N, Q = shape[2:]
    budget, (_, _, row_chunks, groups) = chunked_budget(Q, N, kind != "none", plan)
    m, words, stride = mask(kind, Q, N)
    nv, queries = device_rows(ctx, shape)
    kw = dict(fused=-1, accept=words, accept_stride_words=stride)
    for cand_k in (0, 4 * TOPK):
        for id_base in (0, 1000):
            got, (fused, fallbacks, _), launches = run_nvq(ctx, nv, queries, vsf, cand_k, budget=budget, id_base=id_base, **kw)
            assert (fused, fallbacks) == (0, 0)
            assert launches == (0, row_chunks * groups + (cand_k > 0)), (cand_k, id_base)
            if cand_k:
                w = wanted(shape, vsf, kind)
                if kind == "few":
                    assert (w[0][:, 3:] == -1).all() and (w[0][:, :3] >= 0).all()   # the merge holds mostly -1
                assert T.same(got, with_base(w, id_base)), id_base
            else:
                whole, _, launches = run_nvq(ctx, nv, queries, vsf, 0, id_base=id_base, **kw)
                assert launches == (0, 1) and T.same(got, whole), id_base
                if id_base == 0:
                    check_float64(shape, vsf, m, got)


# ---------------- 5. the auto gate ----------------
@functools.lru_cache(maxsize=None)
def gate_problem(N):
    """(oracle with encoded rows, queries): D = 24 in two sub-vectors; no row is de-quantised on the host"""
    D, S, Q = 24, 2, 5
    rng = np.random.default_rng(N)
    X = rng.standard_normal((N, D)).astype(np.float32)
    queries = (X[rng.integers(0, N, Q)] + 0.1 * rng.standard_normal((Q, D))).astype(np.float32)
    o = O.OracleNVQ.compute(X, S)
    o.encode_all(X)
    return o, queries


@pytest.mark.parametrize("N,vsf", [(GATE - 1, VSF.EUCLIDEAN), (GATE - 1, VSF.DOT_PRODUCT), (GATE, VSF.COSINE), (GATE, VSF.EUCLIDEAN)])
def test_auto_gate(ctx, N, vsf):
    """no option set: the chunked route below 65536 rows, the fused route (stride 16, cap 4 kc 16) from there"""
    Q, cand_k = 5, 4 * TOPK
    o, queries = gate_problem(N)
    g, cap, _, chunks = fused_plan(Q, N, cand_k, DEFAULT_BUDGET)
    assert (g, cap, chunks) == (16, 2560, 1) and chunked_plan(Q, N, DEFAULT_BUDGET, False)[2:] == (1, 1)
    sc = o.scores(queries, int(vsf), np.tile(np.arange(N, dtype=np.int32), (Q, 1)))
    assert list_bounds(sc, None, g, cand_k)[1].max() <= cap, "the seed overflows a list: change the seed, not the cap"
    ids, out = [], []
    for q in range(Q):
        top = T.ref_topk(sc[q], np.ones(N, bool), cand_k + 1)[1]
        assert top[TOPK - 1] - top[cand_k] > 1e-4, "the seed leaves no gap: change the seed"
        i, s = T.ref_topk(sc[q], np.ones(N, bool), TOPK)
        ids.append(i)
        out.append(s)
    nv = J.NVQVectors(ctx, J.NVQuantization.create(ctx, o.mean, o.S), o.bytes, o.params)
    got, (fused, fallbacks, _), launches = run_nvq(ctx, nv, queries, vsf, cand_k, fused=None)
    assert T.same(got, (np.stack(ids), np.stack(out)))
    assert (fused, fallbacks) == ((1, 0) if N >= GATE else (0, 0))
    assert launches == ((1, 2) if N >= GATE else (0, 2))
