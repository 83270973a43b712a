"""CPU check of the BQ build-time scoring kernels: the batched robust prune over BQ rows (jvector_amd/csrc/bd_body.h — the body of
bq_retain_kernel) and the node-seeded graph search with self-exclusion (bg_body.h, BgParams::exclude) are compiled unchanged for the
64-lane wave emulator (tests/emu/bd_emu.cpp) and must reproduce the yardsticks of bq_build_yardstick.py with no tolerance:
selections, n_selected and short_edges (NaN equal to NaN) for the prune; ids, BQ similarities, visitedCount and expandedCount for
the search, in the FAST form and in the SAFE form of a retried query.  The GPU twin is tests/test_zz_bq_build_gpu.py."""
import ctypes as C
import os
import platform
import subprocess

import numpy as np
import pytest

from bq_graph_yardstick import Yardstick, build_problem, np_encode
from bq_build_yardstick import candidate_lists, pair_similarity, retain_diverse, same, self_mask

pytestmark = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jvector_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "bd_emu.cpp"), os.path.join(ROOT, "tests", "emu", "bg_emu.cpp"),
       os.path.join(ROOT, "tests", "emu", "hip_emu.h")] + [os.path.join(CSRC, f) for f in (
           "bd_body.h", "bd_params.h", "bg_body.h", "bg_params.h", "gs_body.h", "gs_host.h", "gs_params.h")]
LIB = os.path.join(ROOT, "build", "emu", "libbd_emu.so")
GS_OVERFLOW = 1
N = 600


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               SRC[0], "-o", LIB])
    lib = C.CDLL(LIB)
    lib.bd_emu_retain.restype = C.c_int
    lib.bd_emu_search_nodes.restype = C.c_long
    return lib


_fp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def run_retain(emu, words, D, nodes, scores, max_degree, alpha, cand_count=None, diverse_before=None, wt=None):
    W = words.shape[1]
    P, Cn = nodes.shape
    nodes, scores = np.ascontiguousarray(nodes, np.int32), np.ascontiguousarray(scores, np.float32)
    cc = None if cand_count is None else np.ascontiguousarray(cand_count, np.int32)
    db = None if diverse_before is None else np.ascontiguousarray(diverse_before, np.int32)
    sel = np.full((P, max_degree), -7, np.int32)
    cnt = np.full(P, -7, np.int32)
    se = np.full(P, 123.0, np.float32)
    if wt is None:
        wt = W if W in (1, 2, 12, 16) else 0
    words = np.ascontiguousarray(words)
    rc = emu.bd_emu_retain(_fp(words), C.c_int64(len(words)), D, W, _fp(nodes), _fp(scores), _fp(cc), _fp(db), P, Cn, max_degree,
                           C.c_float(alpha), wt, _fp(sel), _fp(cnt), _fp(se))
    assert rc == 0, rc
    return sel, cnt, se


@pytest.fixture(scope="module")
def data():
    cache = {}

    def get(D, dup=False):
        if (D, dup) not in cache:
            v = np.random.default_rng(40 + D).standard_normal((N, D)).astype(np.float32)
            if dup:
                v[N // 2:] = v[:N - N // 2]
            cache[(D, dup)] = np_encode(v, D)
        return cache[(D, dup)]
    return get


@pytest.mark.parametrize("alpha", [1.0, 1.2, 1.4])
@pytest.mark.parametrize("max_degree", [1, 8, 32, 64])
@pytest.mark.parametrize("D", [64, 100, 300, 768, 1000])
def test_prune_matches_the_yardstick(emu, data, D, max_degree, alpha):
    words = data(D)
    for Cn in (1, 63, 65, 200):
        nodes, scores = candidate_lists(words, D, 6, Cn, 1000 * D + Cn)
        want = retain_diverse(words, D, nodes, scores, max_degree, alpha)
        same(run_retain(emu, words, D, nodes, scores, max_degree, alpha), want)
        if Cn == 65 and words.shape[1] in (1, 2, 12, 16):   # the generic-width form where a compiled width exists
            same(run_retain(emu, words, D, nodes, scores, max_degree, alpha, wt=0), want)


def test_the_prune_cases_are_not_vacuous(data):
    for D in (64, 100, 768):
        words = data(D)
        nodes, scores = candidate_lists(words, D, 40, 65, 7)
        sel, cnt, _ = retain_diverse(words, D, nodes, scores, 32, 1.0)
        not_prefix = sum(1 for p in range(40) if not np.array_equal(sel[p, :cnt[p]], np.arange(cnt[p])))
        assert not_prefix >= 20, (D, not_prefix)
        _, cnt2, _ = retain_diverse(words, D, nodes, scores, 32, 1.2)
        assert (cnt2 > cnt).any(), D


def test_prune_edge_cases(emu, data):
    D, md = 100, 8
    words = data(D)
    nodes, scores = candidate_lists(words, D, 12, 40, 3)
    # the loop never runs: alpha below 1
    want = retain_diverse(words, D, nodes, scores, md, 0.9, diverse_before=np.full(12, 3, np.int32))
    assert np.isnan(want[2]).all() and (want[1] == 3).all()
    same(run_retain(emu, words, D, nodes, scores, md, 0.9, diverse_before=np.full(12, 3, np.int32)), want)
    # ragged counts (0 included) and every kind of diverse_before
    count = np.array([0, 1, 2, 5, 40, 39, 17, 8, 9, 64, -3, 33], np.int32)
    before = np.array([0, 3, md, md + 2, 0, 3, md, md + 2, 1, 2, 0, 50], np.int32)
    for alpha in (1.0, 1.2):
        want = retain_diverse(words, D, nodes, scores, md, alpha, cand_count=count, diverse_before=before)
        same(run_retain(emu, words, D, nodes, scores, md, alpha, cand_count=count, diverse_before=before), want)
    # an id listed twice, -1 and out-of-range ordinals inside a list, arbitrary scores
    rng = np.random.default_rng(5)
    nodes2, scores2 = nodes.copy(), scores.copy()
    for p in range(12):
        a, b = rng.choice(40, 2, replace=False)
        nodes2[p, b] = nodes2[p, a]
        nodes2[p, rng.integers(0, 40)] = -1
        nodes2[p, rng.integers(0, 40)] = N + 5
    for alpha in (1.0, 1.2, 1.4):
        same(run_retain(emu, words, D, nodes2, scores2, md, alpha), retain_diverse(words, D, nodes2, scores2, md, alpha))
    scores3 = rng.standard_normal(scores.shape).astype(np.float32)
    scores3[:, 5] = -np.inf
    scores3[:, 9] = np.nan
    scores3[:, 11] = np.inf
    for alpha in (1.0, 1.4):
        same(run_retain(emu, words, D, nodes2, scores3, 32, alpha), retain_diverse(words, D, nodes2, scores3, 32, alpha))


def test_prune_with_duplicated_vectors_and_the_strict_comparison(emu, data):
    D = 64
    words = data(D, dup=True)
    nodes, scores = candidate_lists(words, D, 10, 65, 9)
    # sim == score * alpha occurs: a candidate whose twin is already selected and whose own score is that similarity
    hits = 0
    for p in range(10):
        for i in range(1, 65):
            hits += int((pair_similarity(words, D, int(nodes[p, i]), nodes[p, :i]) == scores[p, i]).any())
    assert hits > 0
    for md in (8, 32):
        same(run_retain(emu, words, D, nodes, scores, md, 1.0), retain_diverse(words, D, nodes, scores, md, 1.0))
        same(run_retain(emu, words, D, nodes, scores, md, 1.2), retain_diverse(words, D, nodes, scores, md, 1.2))


def test_prune_rounds_end_at_the_largest_alpha(emu, data):
    # lists that can never fill maxDegree (too short, all but one entry unselectable): only the alpha steps end the loop.  64 is the
    # largest alpha the C ABI takes; the body clamps whatever else its parameter block holds to it (an f32 stepped by 0.2f stops
    # moving at 2^22: without the clamp these calls would not return), and NaN means no round
    D, md = 100, 8
    words = data(D)
    nodes, scores = candidate_lists(words, D, 4, 5, 11)
    scores = scores.copy()
    scores[:, 1:] = -np.inf
    nodes[1, 2] = -1
    want = retain_diverse(words, D, nodes, scores, md, 64.0)
    assert (want[1] < md).all()
    for alpha in (64.0, 65.0, 1e6, 1e30, np.inf):
        same(run_retain(emu, words, D, nodes, scores, md, alpha), want)
        same(run_retain(emu, words, D, nodes, scores, md, alpha, wt=0), want)
    count = np.array([0, 1, 5, 3], np.int32)
    same(run_retain(emu, words, D, nodes, scores, md, np.inf, cand_count=count), retain_diverse(words, D, nodes, scores, md, 64.0, cand_count=count))
    sel, cnt, se = run_retain(emu, words, D, nodes, scores, md, np.nan)
    assert np.isnan(se).all() and (cnt == 0).all() and (sel == -1).all()


# ---------------------------------------------------------------- node-seeded search ----------------------------------------------------------------

def run_search_nodes(emu, lv, entry, entry_level, words, D, nodes, k, exclude_self, safe=0, vcap_log2=12, cand_cap=128, spill_cap=4096,
                     workers=2, qmap=None):
    n, W = words.shape
    Q = len(nodes)
    i32p = C.POINTER(C.c_int32)
    L = len(lv)
    keep_ids = [None if ids is None else np.ascontiguousarray(ids, np.int32) for ids, _ in lv]
    lvn = (i32p * L)(*[C.cast(None, i32p) if a is None else a.ctypes.data_as(i32p) for a in keep_ids])
    keep = [np.ascontiguousarray(nb, np.int32) for _, nb in lv]
    nbrs = (i32p * L)(*[a.ctypes.data_as(i32p) for a in keep])
    count = (C.c_int32 * L)(*[a.shape[0] for a in keep])
    degree = (C.c_int32 * L)(*[a.shape[1] for a in keep])
    words = np.ascontiguousarray(words)
    nodes = np.ascontiguousarray(nodes, np.int32)
    out_ids = np.full((Q, k), -7, np.int32)
    out_sc = np.full((Q, k), np.nan, np.float32)
    stats = np.full((Q, 2), -7, np.int64)
    status = np.full(Q, -9, np.int32)
    wt = W if W in (1, 2, 4, 12) else 0
    qm = None if qmap is None else np.ascontiguousarray(qmap, np.int32)
    rc = emu.bd_emu_search_nodes(L, lvn, nbrs, count, degree, entry, entry_level, n, _fp(words), D, W, _fp(nodes), Q, k, int(exclude_self),
                                 safe, vcap_log2, cand_cap, spill_cap, workers, wt, _fp(qm), 0 if qm is None else len(qm),
                                 _fp(out_ids), _fp(out_sc), _fp(stats), _fp(status))
    assert rc >= 0, rc
    return out_ids, out_sc, stats, status


def check_search(got, want, only=None):
    ids, sc, st, status = got
    wi, ws, wst = want
    for qi in (range(ids.shape[0]) if only is None else only):
        assert status[qi] == 0, (qi, status[qi])
        assert np.array_equal(st[qi], wst[qi]), (qi, st[qi], wst[qi])
        order = np.lexsort((np.where(ids[qi] < 0, np.iinfo(np.int32).max, ids[qi]), -sc[qi]))   # the kernel's kept set is unordered
        assert np.array_equal(ids[qi][order], wi[qi]), qi
        assert np.array_equal(sc[qi][order], ws[qi]), qi


@pytest.mark.parametrize("D,degree,levels", [(64, 12, 3), (100, 80, 3), (768, 12, 1)])
def test_node_seeded_search_and_self_exclusion(emu, D, degree, levels):
    v, lv, entry, el, _ = build_problem(300 + D, 500, D, degree, levels, 1)
    ys = Yardstick(v, lv, entry, el, D)
    nodes = np.concatenate([np.random.default_rng(D).choice(500, 7, replace=False), [entry, entry]]).astype(np.int32)
    nodes[3] = nodes[2]   # a repeated ordinal
    for k in (10, 50):
        plain = ys.approx(v[nodes], k, k)
        check_search(run_search_nodes(emu, lv, entry, el, ys.words, D, nodes, k, False), plain)
        assert any(nodes[q] in plain[0][q] for q in range(len(nodes)))   # the exclusion below has something to exclude
        masked = ys.approx(v[nodes], k, k, accept=self_mask(nodes, 500))
        got = run_search_nodes(emu, lv, entry, el, ys.words, D, nodes, k, True)
        check_search(got, masked)
        assert not any(nodes[q] in got[0][q] for q in range(len(nodes)))
        check_search(run_search_nodes(emu, lv, entry, el, ys.words, D, nodes, k, True, safe=1), masked)


def test_self_exclusion_survives_the_retry(emu):
    D = 100
    v, lv, entry, el, _ = build_problem(77, 500, D, 80, 3, 1)
    ys = Yardstick(v, lv, entry, el, D)
    nodes = np.random.default_rng(2).choice(500, 9, replace=False).astype(np.int32)
    k = 200
    masked = ys.approx(v[nodes], k, k, accept=self_mask(nodes, 500))
    ids, sc, st, status = run_search_nodes(emu, lv, entry, el, ys.words, D, nodes, k, True, vcap_log2=8)
    assert (status == GS_OVERFLOW).all() and (ids == -1).all()
    redo = np.flatnonzero(status == GS_OVERFLOW)
    got = run_search_nodes(emu, lv, entry, el, ys.words, D, nodes, k, True, safe=1, qmap=redo)
    check_search(got, masked, only=redo)
    assert not any(nodes[q] in got[0][q] for q in redo)
