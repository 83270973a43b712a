"""The filtered flat PQ search without a GPU: the entry point of include/jvector_flat_filtered.h is declared, mirrored by
flat_filtered.FLAT_FILTERED_SIGNATURES and exported; and the kernel bodies (jvector_amd/csrc/fa_body.h: the three steps of the mask
compaction, the list ADC scan, the position map) compiled unchanged for the lane emulator (tests/emu/fa_emu.cpp) equal np.flatnonzero on
every mask shape the GPU tests use — junk at and beyond N included — and the oracle's ADC scores bit for bit.  The GPU twin is
tests/test_zz_flat_filtered_gpu.py."""
import ctypes as C
import os
import platform
import re
import subprocess

import numpy as np
import pytest

from flat_accept_ref import pack
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["jv_hip_search_flat_filtered"]


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbol_is_declared_mirrored_and_exported():
    import jvector_amd
    from jvector_amd import _lib, flat_filtered
    text = header_text("jvector_flat_filtered.h")
    names = re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)
    assert names == NEW
    assert set(names) == set(flat_filtered.FLAT_FILTERED_SIGNATURES)
    assert '#include "jvector_hip.h"' in text
    for name, (_, args) in flat_filtered.FLAT_FILTERED_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args) == 15, name
    # the engine's own table and header are as they were: the new symbol is in neither
    assert not set(names) & set(_lib.SIGNATURES)
    assert not [n for n in names if n in header_text("jvector_hip.h")]
    assert os.path.exists(jvector_amd.LIB_PATH)
    raw = C.CDLL(jvector_amd.LIB_PATH)
    assert [n for n in names if not hasattr(raw, n)] == []
    lb = flat_filtered.lib()
    for n in names:
        assert getattr(lb, n).argtypes == flat_filtered.FLAT_FILTERED_SIGNATURES[n][1], n


def test_the_searcher_has_the_method_and_pack_accept_packs_little_endian_bits():
    import jvector_amd as J
    from jvector_amd import flat_filtered
    assert callable(J.FlatSearcher.search_filtered) and callable(flat_filtered.search_flat_filtered)
    m = np.zeros(130, bool)
    m[[0, 63, 64, 129]] = True
    w = flat_filtered.pack_accept(m)
    assert w.dtype == np.uint64 and w.tolist() == [1 | 1 << 63, 1, 2]
    w2 = flat_filtered.pack_accept(np.stack([m, ~m]))
    assert w2.shape == (2, 3) and w2[0].tolist() == w.tolist() and w2[1].tolist() == [~(1 | 1 << 63) & (2 ** 64 - 1), 2 ** 64 - 2, 1]
    assert np.array_equal(w, pack(m))


# ---- the bodies on the lane emulator ----
CSRC = os.path.join(ROOT, "jvector_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", f) for f in ("fa_emu.cpp", "bg_emu.cpp", "hip_emu.h")] + [os.path.join(CSRC, f) for f in (
    "fa_body.h", "fa_params.h", "bg_body.h", "bg_params.h", "gs_body.h", "gs_host.h", "gs_params.h")]
LIB = os.path.join(ROOT, "build", "emu", "libfa_emu.so")
needs_emu = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC[0], "-o", LIB])
    lib = C.CDLL(LIB)
    for f in ("fa_emu_scan_rows", "fa_emu_tile", "fa_emu_count", "fa_emu_lists", "fa_emu_adc", "fa_emu_map"):
        getattr(lib, f).restype = C.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check_lists(emu, masks, junk, slack=0, replicate=0):
    """masks: bool [N] (one shared mask) or [Q, N].  The emulated counts and lists against np.flatnonzero; canaries behind every row.
    replicate: the shared mask written into that many list rows (the route of the shapes the multi-query kernel does not take)."""
    masks = np.asarray(masks, bool)
    shared = masks.ndim == 1
    rows = masks[None] if shared else masks
    n = rows.shape[1]
    stride = 0 if shared else (n + 63) // 64 + slack
    bits = pack(masks, junk=junk, stride_words=stride or None).reshape(-1)
    if not shared:
        bits = bits[: stride * (len(rows) - 1) + (n + 63) // 64].copy()   # the last mask ends at its last valid word
    totals = np.full(len(rows), 12345, np.uint32)
    assert emu.fa_emu_count(_p(bits), C.c_int64(stride), C.c_int64(n), len(rows), _p(totals)) == 0
    want = [np.flatnonzero(r).astype(np.int32) for r in rows]
    assert totals.tolist() == [len(w) for w in want]
    L = max(64, (max(len(w) for w in want) + 63) // 64 * 64)
    nrows = replicate if shared and replicate else len(rows)
    flat = np.full(nrows * L + 8, -77, np.int32)
    assert emu.fa_emu_lists(_p(bits), C.c_int64(stride), C.c_int64(n), len(rows), 0, nrows, C.c_int64(L), _p(flat)) == 0
    assert (flat[nrows * L:] == -77).all()
    lists = flat[: nrows * L].reshape(nrows, L)
    for y in range(nrows):
        w = want[0 if shared else y]
        assert np.array_equal(lists[y, :len(w)], w), (y, np.flatnonzero(lists[y, :len(w)] != w)[:5])
        assert (lists[y, len(w):] == -1).all(), y
    return lists


@needs_emu
def test_the_scan_block_is_the_exported_constant(emu):
    from jvector_amd import flat_filtered
    assert emu.fa_emu_scan_rows() == flat_filtered.SCAN_ROWS and flat_filtered.SCAN_ROWS % 4096 == 0
    text = open(os.path.join(CSRC, "fa_params.h")).read()
    assert re.search(r"constexpr\s+int\s+FA_SCAN_ROWS\s*=\s*%d\s*;" % flat_filtered.SCAN_ROWS, text)


@needs_emu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 8193])
@pytest.mark.parametrize("junk", [False, True])
def test_lists_all_set_all_clear_and_the_edges(emu, n, junk):
    check_lists(emu, np.ones(n, bool), junk)
    check_lists(emu, np.zeros(n, bool), junk)
    for at in (0, n - 1):
        one = np.zeros(n, bool)
        one[at] = True
        check_lists(emu, one, junk)
    rng = np.random.default_rng(n)
    for density in (0.01, 0.5):
        check_lists(emu, rng.random(n) < density, junk)


@needs_emu
def test_lists_per_query_masks_with_junk_in_the_slack_words_and_the_tail_bits(emu):
    # the shape of the GPU test D: the last word holds one valid bit, the stride leaves three slack words, all junk is ones
    Q, n = 6, 12801
    rng = np.random.default_rng(4)
    masks = np.zeros((Q, n), bool)
    masks[1] = True
    masks[2, 7777] = True
    for q, density in ((3, 0.01), (4, 0.3), (5, 0.9)):
        masks[q] = rng.random(n) < density
    masks[5, n - 1] = True
    check_lists(emu, masks, junk=True, slack=3)
    check_lists(emu, masks, junk=False, slack=0)


@needs_emu
@pytest.mark.parametrize("junk", [False, True])
def test_lists_at_the_scan_block_boundaries(emu, junk):
    # the shapes of the GPU test E
    S = emu.fa_emu_scan_rows()
    n = 3 * S + 65
    last = np.zeros(n, bool)
    last[3 * S:] = True
    first_rows = np.zeros(n, bool)
    first_rows[0::S] = True
    last_rows = np.zeros(n, bool)
    last_rows[S - 1::S] = True
    last_rows[n - 1] = True
    sides = np.zeros(n, bool)
    for b in (S, 2 * S, 3 * S):
        sides[b - 64: b + 64] = True
    for m in (last, first_rows, last_rows, sides):
        check_lists(emu, m, junk)
    check_lists(emu, np.stack([last, first_rows, last_rows, sides]), junk, slack=2)


@needs_emu
def test_a_shared_mask_replicated_into_several_list_rows(emu):
    m = np.random.default_rng(9).random(5000) < 0.2
    lists = check_lists(emu, m, junk=True, replicate=3)
    assert lists.shape[0] == 3


@needs_emu
def test_the_map_keeps_minus_one(emu):
    lst = np.array([5, 9, 200, 4000, -1, -1], np.int32)
    ids = np.array([3, -1, 0, 2, 1, -1, -1, 3] * 20 + [0, 1, -1], np.int32)
    got = np.concatenate([ids, np.full(8, -77, np.int32)])
    assert emu.fa_emu_map(_p(lst), C.c_int64(4), _p(got), C.c_int64(len(ids))) == 0
    assert np.array_equal(got[:len(ids)], np.where(ids >= 0, lst[np.maximum(ids, 0)], -1)) and (got[len(ids):] == -77).all()
    # a position at or beyond the list's length is no result either
    got = np.array([4, 5, 3], np.int32)
    assert emu.fa_emu_map(_p(lst), C.c_int64(4), _p(got), C.c_int64(3)) == 0 and got.tolist() == [-1, -1, 4000]


def adc_problem(M, N, Q, seed):
    D = 2 * M
    rng = np.random.default_rng(seed)
    vecs = rng.standard_normal((N, D)).astype(np.float32)
    vecs[1::7] = vecs[0:-1:7][: len(vecs[1::7])]
    queries = (vecs[rng.integers(0, N, Q)] + 0.1 * rng.standard_normal((Q, D))).astype(np.float32)
    cb = np.concatenate([vecs[:256, 2 * m: 2 * m + 2].reshape(-1) for m in range(M)])
    opq = O.OraclePQ(D, M, cb)
    return opq, opq.encode_all(vecs), queries


@needs_emu
@pytest.mark.parametrize("M", [16, 32, 96])
@pytest.mark.parametrize("Q", [1, 5])
def test_list_adc_equals_the_oracle_bit_for_bit(emu, M, Q):
    N = 3000
    opq, codes, queries = adc_problem(M, N, Q, 100 + M + Q)
    R = 8 if M == 32 else 4
    tile = emu.fa_emu_tile(R)
    count = tile + 37 if tile + 37 < N else N - 100      # the list crosses a workgroup tile
    assert tile < count <= N
    lst = np.sort(np.random.default_rng(M).choice(N, count, replace=False)).astype(np.int32)
    L = (count + 63) // 64 * 64
    padded = np.concatenate([lst, np.full(L - count, -1, np.int32)])
    for vsf in (O.EUCLIDEAN, O.DOT_PRODUCT, O.COSINE):
        dec = [opq.decoder(queries[q], vsf) for q in range(Q)]
        luts = np.ascontiguousarray(np.stack([d[0] for d in dec]), np.float32)
        bmag = np.array([d[2] for d in dec], np.float32)
        norms = None
        if vsf == O.COSINE:
            norms = np.zeros(N, np.float32)
            for m in range(M):                                  # one f32 chain in ascending m, as the engine's norm table is built
                norms = (norms + dec[0][1][m * 256 + codes[:, m].astype(np.int64)]).astype(np.float32)
        flat = np.full(Q * L + 4, np.float32(7.5))
        assert emu.fa_emu_adc(_p(luts), _p(bmag), _p(codes), _p(norms), _p(padded), C.c_int64(count), C.c_int64(N), C.c_int64(L), Q, M, vsf, R,
                              _p(flat)) == 0
        out = flat[: Q * L].reshape(Q, L)
        assert (flat[Q * L:] == 7.5).all() and (out[:, count:] == 7.5).all()      # nothing beyond the list's length is written
        for q in range(Q):
            want = opq.adc_scores(queries[q], vsf, codes, ordinals=lst)
            assert np.array_equal(out[q, :count].view(np.int32), want.view(np.int32)), (vsf, q)


@needs_emu
def test_list_entries_outside_the_rows_score_minus_infinity(emu):
    M, N, Q = 16, 500, 3
    opq, codes, queries = adc_problem(M, N, Q, 5)
    lst = np.array([3, -1, N, 499, N + 70, 0, -5], np.int32)
    count, L = len(lst), 64
    padded = np.concatenate([lst, np.full(L - count, -1, np.int32)])
    dec = [opq.decoder(queries[q], O.DOT_PRODUCT) for q in range(Q)]
    luts = np.ascontiguousarray(np.stack([d[0] for d in dec]), np.float32)
    out = np.zeros((Q, L), np.float32)
    assert emu.fa_emu_adc(_p(luts), None, _p(codes), None, _p(padded), C.c_int64(count), C.c_int64(N), C.c_int64(L), Q, M, O.DOT_PRODUCT, 4,
                          _p(out)) == 0
    ok = (lst >= 0) & (lst < N)
    for q in range(Q):
        want = opq.adc_scores(queries[q], O.DOT_PRODUCT, codes, ordinals=lst[ok])
        assert np.array_equal(out[q, :count][ok].view(np.int32), want.view(np.int32))
        assert (out[q, :count][~ok] == -np.inf).all()


@needs_emu
def test_the_results_do_not_depend_on_the_lane_schedule(emu):
    m = np.random.default_rng(2).random(9000) < 0.4
    base = check_lists(emu, m, junk=True)
    try:
        for order in ("reverse", "random:5"):
            os.environ["EMU_LANE_ORDER"] = order
            assert np.array_equal(check_lists(emu, m, junk=True), base)
    finally:
        os.environ.pop("EMU_LANE_ORDER", None)
