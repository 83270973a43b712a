"""The BQ builder without a GPU: the C ABI of include/jvector_bq_builder.h is mirrored by bq_builder.BQ_BUILDER_SIGNATURES and exported
by the library; the yardstick of tests/bq_builder_yardstick.py is exact (every score the oracle stores under the scaled sign quantizer
is a BQ similarity bit for bit) and its cases are not vacuous; and the entry-point body (jvector_amd/csrc/bm_body.h: the bitwise-majority
row and the member nearest to it) compiled unchanged for the 64-lane wave emulator (tests/emu/bm_emu.cpp) equals its numpy restatement.
The GPU twin is tests/test_zz_bq_builder_gpu.py."""
import ctypes as C
import os
import platform
import re
import subprocess

import numpy as np
import pytest

from bq_builder_yardstick import cluster_data, np_majority, np_nearest_row, oracle_builder, score_bit_mismatches
from bq_graph_yardstick import np_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_symbols(name):
    return re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", header_text(name))


def test_header_symbols_are_mirrored_and_exported():
    import jvector_amd
    from jvector_amd import bq_builder
    names = header_symbols("jvector_bq_builder.h")
    assert sorted(names) == sorted([
        "jv_hip_bq_builder_create", "jv_hip_bq_builder_seed", "jv_hip_bq_builder_insert_batch", "jv_hip_bq_builder_improve_batch",
        "jv_hip_bq_builder_finish", "jv_hip_bq_builder_stats", "jv_hip_bq_builder_working_lists", "jv_hip_bq_builder_neighbors_device",
        "jv_hip_bq_builder_destroy", "jv_hip_bq_build_layered"])
    assert set(names) == set(bq_builder.BQ_BUILDER_SIGNATURES)
    text = header_text("jvector_bq_builder.h")
    for name, (_, args) in bq_builder.BQ_BUILDER_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    if os.path.exists(jvector_amd.LIB_PATH):
        raw = C.CDLL(jvector_amd.LIB_PATH)
        assert [n for n in names if not hasattr(raw, n)] == []
        lb = bq_builder.lib()
        for n in names:
            assert getattr(lb, n).argtypes == bq_builder.BQ_BUILDER_SIGNATURES[n][1], n


def test_package_exports_the_builder():
    import jvector_amd as J
    from jvector_amd import bq_builder
    assert J.BQGraphBuilder is bq_builder.BQGraphBuilder and J.build_bq_layered is bq_builder.build_bq_layered
    for m in ("seed", "insert_batch", "improve_batch", "finish", "working_rows", "row_width", "stats", "close"):
        assert callable(getattr(J.BQGraphBuilder, m))


def test_the_pq_builder_names_no_bq_symbol():
    """tests/mock/build_mock.py compiles builder.cpp without the BQ sources"""
    text = open(os.path.join(ROOT, "jvector_amd", "csrc", "builder.cpp")).read()
    assert "jv_hip_bq_" not in text and "bq_internal.h" not in text and "jv_bq_" not in text


def _build(v, D, max_degree, beam, alpha, overflow, scaled=True, improve=0, count=False):
    ob = oracle_builder(v, D, max_degree, beam, alpha, overflow, scaled=scaled, improve=improve > 0)
    N, words = len(v), np_encode(v, D)
    total = bad = 0
    for i in range(N):
        ob.add(i)
        if count and i in (1, 2, 3, N // 3, N // 2, N - 1):
            t, b = score_bit_mismatches(ob, words, D, range(i + 1))
            total, bad = total + t, bad + b
    for _ in range(improve):
        for i in range(N):
            ob.improve(i)
        if count:
            t, b = score_bit_mismatches(ob, words, D, range(N))
            total, bad = total + t, bad + b
    reprunes = ob.info()["reprunes"]
    ob.cleanup()
    return ob.rows(0, max_degree), total, bad, reprunes


@pytest.mark.parametrize("D,N,max_degree,beam,alpha,overflow", [(64, 400, 8, 30, 1.2, 1.2), (256, 300, 16, 40, 1.2, 2.0), (64, 300, 4, 20, 1.4, 1.5)])
def test_scaled_quantizer_scores_are_bq_similarities_bit_for_bit(D, N, max_degree, beam, alpha, overflow):
    v = cluster_data(N, D, 3, dup=20)
    _, total, bad, reprunes = _build(v, D, max_degree, beam, alpha, overflow, improve=1, count=True)
    assert total > 1000 and bad == 0, (total, bad)
    assert reprunes > 0


def test_the_cases_are_not_vacuous():
    """alpha matters, and at alpha > 1 only the scaled quantizer is the yardstick: the plain one prunes another graph"""
    N, D = 400, 64
    v = cluster_data(N, D, 3, dup=20)
    s10 = _build(v, D, 8, 30, 1.0, 1.5)[0]
    s12 = _build(v, D, 8, 30, 1.2, 1.5)[0]
    p10 = _build(v, D, 8, 30, 1.0, 1.5, scaled=False)[0]
    p12 = _build(v, D, 8, 30, 1.2, 1.5, scaled=False)[0]
    assert np.array_equal(s10, p10)                              # a monotone map of the scores changes nothing at alpha = 1
    assert np.array_equal(_build(v, D, 8, 30, 1.0, 1.5, improve=1)[0], _build(v, D, 8, 30, 1.0, 1.5, scaled=False, improve=1)[0])
    assert int((s10 != s12).any(axis=1).sum()) >= N // 4         # (measured on the issue's data: 287 of 400)
    assert int((s12 != p12).any(axis=1).sum()) >= N // 4         # (234 of 400)


# ---- the entry point's body on the lane emulator ----
CSRC = os.path.join(ROOT, "jvector_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", f) for f in ("bm_emu.cpp", "bg_emu.cpp", "hip_emu.h")] + [os.path.join(CSRC, f) for f in (
    "bm_body.h", "bg_body.h", "bg_params.h", "gs_body.h", "gs_host.h", "gs_params.h")]
LIB = os.path.join(ROOT, "build", "emu", "libbm_emu.so")
needs_emu = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC[0], "-o", LIB])
    lib = C.CDLL(LIB)
    lib.bm_emu_entry.restype = C.c_int
    return lib


def run_entry(emu, words, members, waves):
    words = np.ascontiguousarray(words, np.uint64)
    W = words.shape[1]
    cent = np.full(W, 0xA5A5A5A5A5A5A5A5, np.uint64)
    best = np.full(1, -7, np.int64)
    mem = None if members is None else np.ascontiguousarray(members, np.int32)
    n = len(words) if mem is None else len(mem)
    rc = emu.bm_emu_entry(words.ctypes.data_as(C.c_void_p), C.c_int64(len(words)), W, None if mem is None else mem.ctypes.data_as(C.c_void_p),
                          n, waves, cent.ctypes.data_as(C.c_void_p), best.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return cent, int(best[0]) & 0xFFFFFFFF, int(best[0]) >> 32


def check_entry(emu, words, members, waves):
    ids = np.arange(len(words), dtype=np.int32) if members is None else np.asarray(members, np.int32)
    want_c = np_majority(words[ids])
    want_id, want_h = np_nearest_row(words, ids, want_c)
    cent, got_id, got_h = run_entry(emu, words, members, waves)
    assert np.array_equal(cent, want_c)
    assert (got_id, got_h) == (want_id, want_h)
    return want_c


@needs_emu
@pytest.mark.parametrize("D", [64, 100, 768])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_majority_and_nearest_row_on_the_emulator(emu, D, n):
    rng = np.random.default_rng(100 * D + n)
    N = n + 37
    base = rng.standard_normal(D).astype(np.float32)
    v = (base[None, :] * (rng.random((N, 1)) < 0.5) + 0.8 * rng.standard_normal((N, D))).astype(np.float32)
    words = np_encode(v, D)
    members = np.sort(rng.choice(N, n, replace=False)).astype(np.int32)
    if n % 2 == 0:   # bit 3 of word 0 set in exactly half of the members: an exact half count, which must come out clear
        words[members[:n // 2], 0] |= np.uint64(8)
        words[members[n // 2:], 0] &= ~np.uint64(8)
    for waves in (1, 3):
        check_entry(emu, words, members, waves)
    check_entry(emu, words[:n], None, 2)
    if n % 2 == 0:
        assert not (int(np_majority(words[members])[0]) >> 3) & 1
    assert (np_majority(words[members]).view(np.uint8)[(D + 7) // 8:] == 0).all()   # padding bits stay clear


@needs_emu
def test_ties_go_to_the_smaller_id(emu):
    D = 100
    one = np_encode(np.random.default_rng(5).standard_normal((1, D)).astype(np.float32), D)
    words = np.repeat(one, 130, axis=0)                      # all rows equal: every member at distance 0
    members = np.arange(7, 130, 3, dtype=np.int32)
    c = check_entry(emu, words, members, 2)
    assert np.array_equal(c, one[0]) and run_entry(emu, words, members, 2)[1:] == (7, 0)
    v = np.random.default_rng(6).standard_normal((200, D)).astype(np.float32)
    v[100:] = v[:100]                                        # duplicated rows: the winner has a twin with a larger id
    words = np_encode(v, D)
    check_entry(emu, words, None, 4)
    assert run_entry(emu, words, None, 4)[1] < 100
    members = np.arange(50, 200, dtype=np.int32)             # ... whose first copy is not always a member
    check_entry(emu, words, members, 4)
