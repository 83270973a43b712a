"""BQ compaction without a GPU: the two entry points of include/jvector_bq_compact.h are mirrored by bq_compact.BQ_COMPACT_SIGNATURES
and exported; and the kernel bodies (jvector_amd/csrc/bc_body.h: the three steps of the rank, the adjacency gather, the BQ row gather)
compiled unchanged for the 64-lane wave emulator (tests/emu/bc_emu.cpp) equal tests/bq_compact_yardstick.py byte for byte — the maps on
every shape of present mask the scan can get wrong, the rows on random valid working rows, and the counter of stored ids without an
image.  The GPU twin is tests/test_zz_bq_compact_gpu.py."""
import ctypes as C
import os
import platform
import re
import subprocess

import numpy as np
import pytest

from bq_build_yardstick import pair_similarity
from bq_builder_yardstick import cluster_data
from bq_compact_yardstick import compact_lists, renumbering
from bq_graph_yardstick import np_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["jv_hip_bq_builder_renumbering", "jv_hip_bq_builder_compact"]


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_two_symbols_are_declared_mirrored_and_exported():
    import jvector_amd
    from jvector_amd import bq_builder, bq_compact
    text = header_text("jvector_bq_compact.h")
    names = re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)
    assert sorted(names) == sorted(NEW)
    assert set(names) == set(bq_compact.BQ_COMPACT_SIGNATURES)
    assert '#include "jvector_bq_builder.h"' in text
    for name, (_, args) in bq_compact.BQ_COMPACT_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    # the older tables and headers are as they were: the new symbols are in none of them
    assert not set(names) & (set(bq_builder.BQ_BUILDER_SIGNATURES) | set(bq_builder.BQ_DELETE_SIGNATURES))
    for older in ("jvector_bq_builder.h", "jvector_bq_delete.h"):
        assert not [n for n in names if n in header_text(older)]
    assert os.path.exists(jvector_amd.LIB_PATH)
    raw = C.CDLL(jvector_amd.LIB_PATH)
    assert [n for n in names if not hasattr(raw, n)] == []
    lb = bq_compact.lib()
    for n in names:
        assert getattr(lb, n).argtypes == bq_compact.BQ_COMPACT_SIGNATURES[n][1], n


def test_the_builder_class_has_the_compaction_methods():
    import jvector_amd as J
    for m in ("renumbering", "compact"):
        assert callable(getattr(J.BQGraphBuilder, m))


# ---- the bodies on the lane emulator ----
CSRC = os.path.join(ROOT, "jvector_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", f) for f in ("bc_emu.cpp", "bg_emu.cpp", "hip_emu.h")] + [os.path.join(CSRC, f) for f in (
    "bc_body.h", "bc_params.h", "bg_body.h", "bg_params.h", "gs_body.h", "gs_host.h", "gs_params.h")]
LIB = os.path.join(ROOT, "build", "emu", "libbc_emu.so")
needs_emu = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")
SCAN = 16384   # the cap the issue sets for the nodes of one scan block


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC[0], "-o", LIB])
    lib = C.CDLL(LIB)
    lib.bc_emu_rank.restype = C.c_int
    lib.bc_emu_rows.restype = C.c_int
    lib.bc_emu_scan_nodes.restype = C.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack(mask, padding=0):
    """the bitmap of `mask`; padding: the bits at and beyond len(mask) in the last word (0, or ones)"""
    n = len(mask)
    bits = np.pad(np.asarray(mask, bool), (0, (-n) % 64), constant_values=bool(padding))
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()


def emu_rank(emu, present, padding=0, want_new_to_old=True):
    """(old_to_new, new_to_old, counters) of the emulated rank; canaries behind both maps must survive"""
    n, live = len(present), int(np.sum(present))
    o2n = np.full(n + 8, -77, np.int32)
    n2o = np.full(live + 8, -55, np.int32)
    ctr = np.full(3, 12345, np.uint32)
    assert emu.bc_emu_rank(_p(pack(present, padding)), C.c_int64(n), _p(o2n), _p(n2o) if want_new_to_old else None, _p(ctr)) == 0
    assert (o2n[n:] == -77).all() and (n2o[live:] == -55).all()
    if not want_new_to_old:
        assert (n2o == -55).all()
    return o2n[:n], n2o[:live], ctr


def check_rank(emu, present, padding=0):
    present = np.asarray(present, bool)
    want_o2n, want_n2o = renumbering(present)
    o2n, n2o, ctr = emu_rank(emu, present, padding)
    assert np.array_equal(o2n, want_o2n), np.flatnonzero(o2n != want_o2n)[:5]
    assert np.array_equal(n2o, want_n2o)
    assert ctr.tolist() == [int(present.sum()), 0, 0x7fffffff]


@needs_emu
def test_the_scan_block_is_within_the_cap(emu):
    assert 64 <= emu.bc_emu_scan_nodes() <= SCAN and emu.bc_emu_scan_nodes() % 64 == 0
    text = open(os.path.join(CSRC, "bc_params.h")).read()
    assert re.search(r"constexpr\s+int\s+BC_SCAN_NODES\s*=\s*%d\s*;" % emu.bc_emu_scan_nodes(), text)


@needs_emu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_rank_all_set_all_clear_and_the_edges(emu, n):
    check_rank(emu, np.ones(n, bool))
    check_rank(emu, np.zeros(n, bool))
    last = np.zeros(n, bool)
    last[n - 1] = True
    check_rank(emu, last)                       # only the last valid bit
    check_rank(emu, last, padding=1)            # ... with garbage in the padding bits of the last word
    check_rank(emu, np.ones(n, bool), padding=1)
    check_rank(emu, np.zeros(n, bool), padding=1)
    rng = np.random.default_rng(n)
    for density in (0.1, 0.5, 0.9):
        check_rank(emu, rng.random(n) < density, padding=1)


@needs_emu
def test_rank_a_whole_word_clear_in_the_middle(emu):
    n = 2000
    present = np.ones(n, bool)
    present[640:704] = False                    # word 10
    check_rank(emu, present)
    present[64 * 17: 64 * 19] = False           # and two neighbouring ones
    present[5] = present[1999] = False
    check_rank(emu, present, padding=1)


@needs_emu
@pytest.mark.parametrize("seed,density", [(1, 0.5), (2, 0.9), (3, 0.02)])
def test_rank_random_masks_over_three_scan_blocks(emu, seed, density):
    n = 40_000
    assert -(-n // emu.bc_emu_scan_nodes()) >= 3
    rng = np.random.default_rng(seed)
    present = rng.random(n) < density
    present[SCAN - 1: SCAN + 1] = True          # a block boundary with a node on either side
    present[2 * SCAN - 64: 2 * SCAN] = False     # the last word of the second block clear
    check_rank(emu, present, padding=1)


@needs_emu
def test_rank_without_new_to_old(emu):
    present = np.random.default_rng(5).random(300) < 0.7
    o2n, _, _ = emu_rank(emu, present, want_new_to_old=False)
    assert np.array_equal(o2n, renumbering(present)[0])


def random_rows(words, D, R, present, seed):
    """valid working rows: up to R distinct present neighbours, none the node itself, under their BQ similarities, NodeArray order;
    and diverseBefore marks between 0 and the row's length"""
    rng = np.random.default_rng(seed)
    n = len(words)
    ids, sc, db = np.full((n, R), -1, np.int32), np.zeros((n, R), np.float32), np.zeros(n, np.int32)
    pool = np.flatnonzero(present)
    for i in pool:
        others = pool[pool != i]
        deg = int(min(len(others), rng.integers(0, R + 1)))
        if deg == 0:
            continue
        nb = rng.choice(others, deg, replace=False).astype(np.int32)
        s = pair_similarity(words, D, int(i), nb)
        order = np.lexsort((rng.random(deg), -s))   # equal scores in any node order, as a NodeArray may hold them
        ids[i, :deg], sc[i, :deg] = nb[order], s[order]
        db[i] = rng.integers(0, deg + 1)
    return ids, sc, db


def emu_compact(emu, words, ids, sc, db, present, capacity):
    """the whole emulated compaction: (ids, score bits, db) of `capacity` rows — rows at and beyond live as the memset leaves them —
    the new BQ rows [live], and the counters"""
    n, R = ids.shape
    W = words.shape[1]
    o2n, n2o, ctr = emu_rank(emu, present)
    live = len(n2o)
    out_ids = np.full((capacity + 1, R), -1, np.int32)       # blank, as create leaves the rows the kernel does not write; one canary row
    out_sc = np.zeros((capacity + 1, R), np.float32)
    out_db = np.zeros(capacity + 1, np.int32)
    out_ids[:live], out_sc[:live], out_db[:live] = -99, np.nan, -99   # garbage where the kernel must write every cell
    out_ids[capacity], out_db[capacity] = -31, -31
    rows = np.full((live + 1, W), 0x5a5a5a5a5a5a5a5a, np.uint64)
    o2n, n2o = np.ascontiguousarray(o2n), np.ascontiguousarray(n2o if live else np.zeros(1, np.int32))
    assert emu.bc_emu_rows(C.c_int64(n), C.c_int64(live), R, _p(o2n), _p(n2o), _p(ids), _p(sc), _p(db), _p(out_ids), _p(out_sc), _p(out_db), W,
                           _p(words), _p(rows), _p(ctr)) == 0
    assert (out_ids[capacity] == -31).all() and out_db[capacity] == -31 and (rows[live] == 0x5a5a5a5a5a5a5a5a).all()
    return (out_ids[:capacity], out_sc[:capacity].view(np.int32), out_db[:capacity]), rows[:live], ctr, n2o[:live]


@needs_emu
@pytest.mark.parametrize("D", [64, 100])
@pytest.mark.parametrize("N,R", [(1, 2), (65, 9), (300, 19), (300, 64), (2000, 9)])
def test_rows_equal_the_yardstick(emu, N, D, R):
    rng = np.random.default_rng(1000 * N + D + R)
    words = np_encode(cluster_data(N, D, N + D + R, clusters=3, dup=N // 3), D)
    assert words.shape[1] == (D + 63) // 64 == (1 if D == 64 else 2)
    for frac in (0.0, 0.2, 0.9, 1.0):
        present = np.ones(N, bool)
        present[rng.choice(N, int(N * frac), replace=False)] = False
        ids, sc, db = random_rows(words, D, R, present, N + R)
        capacity = int(present.sum()) + 7
        got, rows, ctr, n2o = emu_compact(emu, words, ids, sc, db, present, capacity)
        want = compact_lists(ids, sc, db, present, capacity)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        assert np.array_equal(rows, words[n2o])
        assert ctr.tolist() == [int(present.sum()), 0, 0x7fffffff]
    if N >= 300:
        assert (got[0] >= 0).sum() == 0 and (want[0] == -1).all()      # (everything removed: all blank)


@needs_emu
def test_ids_without_an_image_are_counted(emu):
    N, D, R = 300, 100, 19
    words = np_encode(cluster_data(N, D, 4), D)
    present = np.ones(N, bool)
    present[np.random.default_rng(8).choice(N, 60, replace=False)] = False
    ids, sc, db = random_rows(words, D, R, present, 3)
    gone = np.flatnonzero(~present)
    o2n, n2o = renumbering(present)
    # three rows get ids that name rows not in the graph (one of them twice), and one an id outside the rows
    victims = [int(n2o[200]), int(n2o[17]), int(n2o[90])]
    ids[victims[0], 0] = gone[0]
    ids[victims[1], 0], ids[victims[1], 1] = gone[1], gone[2]
    ids[victims[2], 0] = N + 5
    got, rows, ctr, _ = emu_compact(emu, words, ids, sc, db, present, int(present.sum()))
    assert ctr.tolist() == [int(present.sum()), 4, 17]                  # the count, and the first new row holding one
    masked = ids.copy()
    masked[victims[0], 0] = masked[victims[1], 0] = masked[victims[1], 1] = masked[victims[2], 0] = -1
    want = compact_lists(masked, sc, db, present, int(present.sum()))   # such an id is written as -1, everything else as always
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@needs_emu
def test_the_result_does_not_depend_on_the_lane_schedule(emu):
    N, D, R = 300, 64, 19
    words = np_encode(cluster_data(N, D, 21, clusters=2, dup=60), D)
    present = np.random.default_rng(2).random(N) < 0.6
    ids, sc, db = random_rows(words, D, R, present, 8)
    base = emu_compact(emu, words, ids, sc, db, present, N)
    try:
        for order in ("reverse", "random:5"):
            os.environ["EMU_LANE_ORDER"] = order
            got = emu_compact(emu, words, ids, sc, db, present, N)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], base[0])) and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])
    finally:
        os.environ.pop("EMU_LANE_ORDER", None)
