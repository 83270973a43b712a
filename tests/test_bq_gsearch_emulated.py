"""CPU check of the BQ graph traversal (jvector_amd/csrc/bg_body.h — the body of bq_graph_search_kernel): the kernel source is
compiled unchanged for the 64-lane wave emulator (tests/emu/bg_emu.cpp) and must reproduce the yardstick of bq_graph_yardstick.py —
the oracle's sequential GraphSearcher driven by a sign quantizer — with no tolerance: the kept results, their BQ similarities,
visitedCount and expandedCount, in the FAST form, and in the SAFE form the host falls back on for queries that outgrow the FAST
form's fixed-size structures.  The GPU twin of this test is tests/test_zz_bq_gsearch_gpu.py."""
import ctypes as C
import os
import platform
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from bq_graph_yardstick import Yardstick, build_problem, np_encode

pytestmark = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jvector_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", "bg_emu.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.h"),
       os.path.join(CSRC, "bg_body.h"), os.path.join(CSRC, "gs_body.h"), os.path.join(CSRC, "gs_host.h"), os.path.join(CSRC, "gs_params.h")]
LIB = os.path.join(ROOT, "build", "emu", "libbg_emu.so")
GS_OVERFLOW = 1


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               SRC[0], "-o", LIB])
    lib = C.CDLL(LIB)
    lib.bg_emu_search.restype = C.c_long
    return lib


def run_emu(emu, lv, entry, entry_level, words, q, D, rerank_k, accept=None, safe=0, vcap_log2=12, cand_cap=128, spill_cap=4096,
            workers=2, wt=None, qmap=None):
    N, W = words.shape
    Q = q.shape[0]
    i32p = C.POINTER(C.c_int32)
    L = len(lv)
    keep_ids = [None if ids is None else np.ascontiguousarray(ids, np.int32) for ids, _ in lv]
    nodes = (i32p * L)(*[C.cast(None, i32p) if a is None else a.ctypes.data_as(i32p) for a in keep_ids])
    keep = [np.ascontiguousarray(nb, np.int32) for _, nb in lv]
    nbrs = (i32p * L)(*[a.ctypes.data_as(i32p) for a in keep])
    count = (C.c_int32 * L)(*[a.shape[0] for a in keep])
    degree = (C.c_int32 * L)(*[a.shape[1] for a in keep])
    qw = np.ascontiguousarray(np_encode(q, D))
    words = np.ascontiguousarray(words)
    mask, stride = None, 0
    if accept is not None:
        mask = O.pack_accept_bits(accept)
        stride = 0 if mask.ndim == 1 else mask.shape[1]
    out_ids = np.full((Q, rerank_k), -7, np.int32)
    out_sc = np.full((Q, rerank_k), np.nan, np.float32)
    stats = np.full((Q, 2), -7, np.int64)
    status = np.full(Q, -9, np.int32)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if wt is None:
        wt = W if W in (1, 2, 4, 12) else 0
    qm = None if qmap is None else np.ascontiguousarray(qmap, np.int32)
    n = emu.bg_emu_search(L, nodes, nbrs, count, degree, entry, entry_level, N, fp(words), fp(qw), D, W, Q, rerank_k, fp(mask),
                          C.c_longlong(stride), safe, vcap_log2, cand_cap, spill_cap, workers, wt, fp(qm), 0 if qm is None else len(qm),
                          fp(out_ids), fp(out_sc), fp(stats), fp(status))
    assert n >= 0, n
    return out_ids, out_sc, stats, status


def check(got, want, only=None):
    ids, sc, st, status = got
    wi, ws, wst = want
    for qi in (range(ids.shape[0]) if only is None else only):
        assert status[qi] == 0, (qi, status[qi])
        assert np.array_equal(st[qi], wst[qi]), (qi, st[qi], wst[qi])
        # the kernel hands over the kept set unordered; the yardstick lists it in NodeQueue order
        order = np.lexsort((np.where(ids[qi] < 0, np.iinfo(np.int32).max, ids[qi]), -sc[qi]))
        assert np.array_equal(ids[qi][order], wi[qi]), qi
        assert np.array_equal(sc[qi][order], ws[qi]), qi


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(D, degree, levels, dup=False):
        key = (D, degree, levels, dup)
        if key not in cache:
            v, lv, entry, el, q = build_problem(1000 + D + degree + levels, 500, D, degree, levels, 9, dup=dup)
            cache[key] = (v, lv, entry, el, q, Yardstick(v, lv, entry, el, D))
        return cache[key]
    return get


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("degree", [12, 80])
@pytest.mark.parametrize("D", [7, 64, 100])
def test_emulated_kernel_matches_the_yardstick(emu, problems, D, degree, levels):
    v, lv, entry, el, q, ys = problems(D, degree, levels)
    for rk in (1, 20, 200):
        want = ys.approx(q, rk, rk)
        check(run_emu(emu, lv, entry, el, ys.words, q, D, rk), want)
        if rk == 20:   # the generic-width form where a compiled width exists, and the SAFE form
            check(run_emu(emu, lv, entry, el, ys.words, q, D, rk, wt=0), want)
            check(run_emu(emu, lv, entry, el, ys.words, q, D, rk, safe=1), want)


@pytest.mark.parametrize("vsf", [O.EUCLIDEAN, O.DOT_PRODUCT, O.COSINE])
def test_yardstick_is_the_same_under_every_similarity_function(problems, vsf):
    v, lv, entry, el, q, ys = problems(100, 12, 3)
    a, b = ys.approx(q, 20, 20, vsf=vsf), ys.approx(q, 20, 20)   # (the 20 nearest of 500: no score near zero)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_wide_rows_in_lds_and_global_visited_table(emu, problems):
    # D = 768: twelve words in scalar registers; a visited table beyond the LDS limit lives in global memory
    v, lv, entry, el, q = build_problem(5, 300, 768, 20, 2, 4)
    ys = Yardstick(v, lv, entry, el, 768)
    want = ys.approx(q, 30, 30)
    check(run_emu(emu, lv, entry, el, ys.words, q, 768, 30), want)
    check(run_emu(emu, lv, entry, el, ys.words, q, 768, 30, vcap_log2=14), want)
    check(run_emu(emu, lv, entry, el, ys.words, q, 768, 30, wt=0), want)


@pytest.mark.parametrize("per_query", [False, True])
def test_accept_masks(emu, problems, per_query):
    v, lv, entry, el, q, ys = problems(64, 12, 3)
    rng = np.random.default_rng(3)
    acc = rng.random((len(q), 500) if per_query else 500) < 0.3
    for rk in (1, 20, 200):
        want = ys.approx(q, rk, rk, accept=acc)
        check(run_emu(emu, lv, entry, el, ys.words, q, 64, rk, accept=acc), want)
        check(run_emu(emu, lv, entry, el, ys.words, q, 64, rk, accept=acc, safe=1), want)
    none = np.zeros(500, bool)
    ids, sc, st, status = run_emu(emu, lv, entry, el, ys.words, q, 64, 20, accept=none)
    assert (ids == -1).all() and np.isneginf(sc).all() and (status == 0).all()
    assert np.array_equal(st, ys.approx(q, 20, 20, accept=none)[2])


def test_ties(emu, problems):
    v, lv, entry, el, q, ys = problems(7, 12, 3, dup=True)
    for rk in (1, 20, 200):
        want = ys.approx(q, rk, rk)
        assert all(len(np.unique(s[np.isfinite(s)])) < np.isfinite(s).sum() for s in want[1]) or rk == 1
        check(run_emu(emu, lv, entry, el, ys.words, q, 7, rk), want)


@pytest.mark.parametrize("D,degree", [(64, 12), (100, 80)])
def test_overflow_is_reported_and_the_safe_form_gives_the_same_answer(emu, problems, D, degree):
    v, lv, entry, el, q, ys = problems(D, degree, 3)
    rk = 200
    want = ys.approx(q, rk, rk)
    # visited table of 256 slots: at most ~128 nodes
    ids, sc, st, status = run_emu(emu, lv, entry, el, ys.words, q, D, rk, vcap_log2=8)
    assert (status == GS_OVERFLOW).all() and (ids == -1).all()
    # roomy table, candidate storage of 128 + 64 keys
    ids, sc, st, status = run_emu(emu, lv, entry, el, ys.words, q, D, rk, vcap_log2=13, cand_cap=128, spill_cap=64)
    assert (status == GS_OVERFLOW).any() and np.isin(status, (0, GS_OVERFLOW)).all()
    redo = np.flatnonzero(status == GS_OVERFLOW)
    check((ids, sc, st, status), want, only=np.flatnonzero(status == 0))
    # the SAFE pass over the overflowed queries only (qmap), the smallest candidate tier: partition, refill, pops from the spill tier
    got = run_emu(emu, lv, entry, el, ys.words, q, D, rk, safe=1, cand_cap=128, qmap=redo)
    check(got, want, only=redo)
    assert (got[3][np.flatnonzero(status == 0)] == -9).all()   # untouched


def test_spill_tier_is_exercised_without_overflow(emu, problems):
    v, lv, entry, el, q, ys = problems(100, 80, 3)
    want = ys.approx(q, 200, 200)
    check(run_emu(emu, lv, entry, el, ys.words, q, 100, 200, cand_cap=128, spill_cap=700, workers=1), want)
