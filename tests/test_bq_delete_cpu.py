"""BQ deletions without a GPU: the five entry points of include/jvector_bq_delete.h are mirrored by bq_builder.BQ_DELETE_SIGNATURES and
exported; and the kernel bodies (jvector_amd/csrc/bx_body.h: the affected list, and the gather / score / sort / merge of one affected
node) compiled unchanged for the 64-lane wave emulator (tests/emu/bx_emu.cpp) equal the literal restatement of removeDeletedNodes in
tests/bq_delete_yardstick.py: the same affected nodes, and per node the same merged list — ids, order, score bits — the same length
and the same candidate count.  The GPU twin, which also runs the prune and the row rewrite, is tests/test_zz_bq_delete_gpu.py."""
import ctypes as C
import os
import platform
import re
import subprocess

import numpy as np
import pytest

from bq_build_yardstick import pair_similarity
from bq_builder_yardstick import cluster_data, oracle_builder
from bq_delete_yardstick import fallback_draws, merged_lists
from bq_graph_yardstick import np_encode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["jv_hip_bq_builder_mark_deleted", "jv_hip_bq_builder_deleted_count", "jv_hip_bq_builder_live_bits", "jv_hip_bq_builder_remove_deleted",
       "jv_hip_bq_builder_entry"]


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_five_symbols_are_declared_mirrored_and_exported():
    import jvector_amd
    from jvector_amd import bq_builder
    text = header_text("jvector_bq_delete.h")
    names = re.findall(r"JV_API\s+[\w\s\*]+?\b(\w+)\s*\(", text)
    assert sorted(names) == sorted(NEW)
    assert set(names) == set(bq_builder.BQ_DELETE_SIGNATURES)
    assert '#include "jvector_bq_delete.h"' in open(os.path.join(ROOT, "include", "jvector_bq_builder.h")).read()
    for name, (_, args) in bq_builder.BQ_DELETE_SIGNATURES.items():
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    assert os.path.exists(jvector_amd.LIB_PATH)
    raw = C.CDLL(jvector_amd.LIB_PATH)
    assert [n for n in names if not hasattr(raw, n)] == []
    lb = bq_builder.lib()
    for n in names:
        assert getattr(lb, n).argtypes == bq_builder.BQ_DELETE_SIGNATURES[n][1], n


def test_the_builder_class_has_the_deletion_methods():
    import jvector_amd as J
    for m in ("mark_deleted", "remove_deleted", "live_bits", "deleted_counts"):
        assert callable(getattr(J.BQGraphBuilder, m))
    assert isinstance(J.BQGraphBuilder.entry, property)


# ---- the bodies on the lane emulator ----
CSRC = os.path.join(ROOT, "jvector_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "emu", f) for f in ("bx_emu.cpp", "bg_emu.cpp", "hip_emu.h")] + [os.path.join(CSRC, f) for f in (
    "bx_body.h", "bx_params.h", "bg_body.h", "bg_params.h", "gs_body.h", "gs_host.h", "gs_params.h")]
LIB = os.path.join(ROOT, "build", "emu", "libbx_emu.so")
needs_emu = pytest.mark.skipif(platform.machine() != "x86_64", reason="the lane emulator's context switch is x86-64 assembly")


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRC):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", SRC[0], "-o", LIB])
    lib = C.CDLL(LIB)
    lib.bx_emu_affected.restype = C.c_int
    lib.bx_emu_merge.restype = C.c_int
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack(mask):
    n = len(mask)
    return np.packbits(np.pad(np.asarray(mask, bool), (0, (-n) % 64)), bitorder="little").view(np.uint64).copy()


def emu_affected(emu, ids, present, marked):
    n, R = ids.shape
    tasks = np.full(n, -77, np.int32)
    cnt = np.full(1, 12345, np.uint32)
    assert emu.bx_emu_affected(_p(ids), C.c_int64(n), R, _p(pack(present)), _p(pack(marked)), _p(tasks), _p(cnt)) == 0
    return tasks[:int(cnt[0])]


def emu_merge(emu, words, D, ids, sc, marked, tasks, L, wt, given=None, given_n=None):
    """(list [P, L] or None, scores, ln, cn)"""
    n, R = ids.shape
    P = len(tasks)
    tasks = np.ascontiguousarray(tasks, np.int32)
    lst = None if L == 0 else np.full((P, L), -99, np.int32)
    lsc = None if L == 0 else np.full((P, L), np.nan, np.float32)
    ln, cn = np.full(P, -5, np.int32), np.full(P, -5, np.int32)
    G = 0 if given is None else given.shape[1]
    rc = emu.bx_emu_merge(_p(words), C.c_int64(n), D, words.shape[1], _p(ids), _p(sc), R, _p(pack(marked)), _p(tasks), P, _p(given), _p(given_n), G, L,
                          _p(lst), _p(lsc), _p(ln), _p(cn), wt)
    assert rc == 0, rc
    return lst, lsc, ln, cn


def random_rows(words, D, R, present, seed):
    """valid working rows: up to R distinct present neighbours, none the node itself, under their BQ similarities, NodeArray order"""
    rng = np.random.default_rng(seed)
    n = len(words)
    ids, sc = np.full((n, R), -1, np.int32), np.zeros((n, R), np.float32)
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
    return ids, sc


def oracle_rows(v, D, max_degree, beam, alpha, overflow):
    ob = oracle_builder(v, D, max_degree, beam, alpha, overflow)
    n = len(v)
    R = max(max_degree, min(64, int(max_degree * overflow)))
    ids, sc = np.full((n, R), -1, np.int32), np.zeros((n, R), np.float32)
    for i in range(n):
        ob.add(i)
    for i in range(n):
        oi, osc, _ = ob.row(0, i)
        ids[i, :len(oi)], sc[i, :len(oi)] = oi, osc
    return ids, sc


def marked_sets(n, present, seed):
    rng = np.random.default_rng(seed)
    pool = np.flatnonzero(present)
    out = {"none": []}
    if len(pool):
        out["one"] = [int(pool[len(pool) // 2])]
        out["10%"] = rng.choice(pool, max(1, len(pool) // 10), replace=False).tolist()
        out["50%"] = rng.choice(pool, max(1, len(pool) // 2), replace=False).tolist()
        out["all but one"] = pool[pool != pool[len(pool) // 3]].tolist()
        out["all"] = pool.tolist()
    res = {}
    for k, ids in out.items():
        m = np.zeros(n, bool)
        m[ids] = True
        res[k] = m
    return res


def check_case(emu, words, D, ids, sc, present, marked, max_degree, wts, seed=7):
    """every comparison of one (graph, marked set); returns (affected, fallback nodes, longest list)"""
    want = merged_lists(words, D, ids, sc, present, marked, max_degree, seed)
    tasks = emu_affected(emu, ids, present, marked)
    assert np.array_equal(tasks, np.array([m["node"] for m in want], np.int32))
    if not want:
        return 0, 0, 0
    normal = [m for m in want if not m["fallback"]]
    fall = [m for m in want if m["fallback"]]
    n = len(ids)
    for wt in wts:
        # first pass: lengths and candidate counts only (a fallback node shows its survivors and no candidate)
        _, _, ln, cn = emu_merge(emu, words, D, ids, sc, marked, tasks, 0, wt)
        for t, m in enumerate(want):
            if m["fallback"]:
                assert cn[t] == 0 and ln[t] == int(((ids[m["node"]] >= 0) & ~marked[np.maximum(ids[m["node"]], 0)]).sum())
            else:
                assert (ln[t], cn[t]) == (len(m["ids"]), m["candidates"]), (m["node"], ln[t], cn[t])
        if normal:
            L = max(len(m["ids"]) for m in normal) + 3
            lst, lsc, ln, cn = emu_merge(emu, words, D, ids, sc, marked, [m["node"] for m in normal], L, wt)
            for t, m in enumerate(normal):
                k = len(m["ids"])
                assert ln[t] == k and cn[t] == m["candidates"]
                assert np.array_equal(lst[t, :k], m["ids"]), (m["node"], lst[t, :k], m["ids"])
                assert np.array_equal(lsc[t, :k].view(np.int32), m["scores"].view(np.int32)), m["node"]
                assert (lst[t, k:] == -1).all() and (lsc[t, k:] == 0).all()
        if fall:
            given = np.full((len(fall), max_degree), -1, np.int32)
            gn = np.zeros(len(fall), np.int32)
            for t, m in enumerate(fall):
                d = fallback_draws(m["node"], n, max_degree, present, marked, seed)
                given[t, :len(d)], gn[t] = d, len(d)
            L = ids.shape[1] + max_degree
            lst, lsc, ln, cn = emu_merge(emu, words, D, ids, sc, marked, [m["node"] for m in fall], L, wt, given, gn)
            for t, m in enumerate(fall):
                k = len(m["ids"])
                assert ln[t] == k and cn[t] == m["candidates"] == gn[t]
                assert np.array_equal(lst[t, :k], m["ids"]) and np.array_equal(lsc[t, :k].view(np.int32), m["scores"].view(np.int32))
    return len(want), len(fall), max(len(m["ids"]) for m in want)


def widths(D):
    W = (D + 63) // 64
    return (W, 0) if W in (1, 2, 12) else (0,)


@needs_emu
@pytest.mark.parametrize("N,D,R", [(1, 64, 2), (2, 100, 2), (2, 64, 8), (65, 192, 8), (65, 64, 19), (65, 768, 64), (300, 100, 19), (300, 768, 8),
                                   (300, 64, 64), (300, 192, 19)])
def test_random_valid_rows_every_marked_set(emu, N, D, R):
    rng = np.random.default_rng(1000 * N + D + R)
    v = cluster_data(N, D, N + D + R, clusters=3, dup=N // 3)   # a third of the rows twice: many equal scores
    words = np_encode(v, D)
    present = np.ones(N, bool)
    if N >= 65:
        present[rng.choice(N, N // 8, replace=False)] = False    # ids that were never inserted: blank rows, in nobody's list
    ids, sc = random_rows(words, D, R, present, N + R)
    seen = [0, 0, 0]
    for name, marked in marked_sets(N, present, D + R).items():
        got = check_case(emu, words, D, ids, sc, present, marked, max(2, int(R / 1.2)), widths(D))
        seen = [max(a, b) for a, b in zip(seen, got)]
        if name in ("none", "all"):
            assert got[0] == 0
    if N >= 65:
        assert seen[0] > N // 4                   # the cases are not vacuous: many affected nodes ...
    if N >= 300:
        assert seen[2] > R                        # ... and lists longer than a row


@needs_emu
@pytest.mark.parametrize("D,N,max_degree,overflow", [(64, 300, 8, 1.2), (64, 300, 16, 1.25), (64, 65, 4, 1.5)])
def test_graphs_of_the_oracle_builder(emu, D, N, max_degree, overflow):
    v = cluster_data(N, D, 3 + N, dup=N // 10)
    words = np_encode(v, D)
    ids, sc = oracle_rows(v, D, max_degree, 30, 1.2, overflow)
    present = np.ones(N, bool)
    total = 0
    for name, marked in marked_sets(N, present, 5).items():
        total += check_case(emu, words, D, ids, sc, present, marked, max_degree, (1, 0))[0]
    assert total > N // 2   # (affected nodes over the six marked sets: the graphs are not vacuous)


@needs_emu
def test_a_node_whose_only_two_hop_candidate_is_itself(emu):
    N, D, R = 65, 100, 8
    words = np_encode(cluster_data(N, D, 9), D)
    present = np.ones(N, bool)
    ids, sc = random_rows(words, D, R, present, 4)
    i, j = 10, 40
    for row, other in ((i, j), (j, i)):
        ids[row], sc[row] = -1, 0.0
        ids[row, 0], sc[row, 0] = other, pair_similarity(words, D, row, [other])[0]
    marked = np.zeros(N, bool)
    marked[j] = True
    want = {m["node"]: m for m in merged_lists(words, D, ids, sc, present, marked, 6, 3)}
    assert want[i]["fallback"] and 1 <= want[i]["candidates"] <= 6 and i not in want[i]["ids"] and j not in want[i]["ids"]
    affected, fallbacks, _ = check_case(emu, words, D, ids, sc, present, marked, 6, (2, 0), seed=3)
    assert fallbacks >= 1
    # the draws are a function of the seed
    assert fallback_draws(i, N, 6, present, marked, 3) == fallback_draws(i, N, 6, present, marked, 3)
    assert fallback_draws(i, N, 6, present, marked, 3) != fallback_draws(i, N, 6, present, marked, 4)


@needs_emu
def test_the_lists_do_not_depend_on_the_lane_schedule(emu):
    N, D, R = 130, 64, 19
    v = cluster_data(N, D, 21, clusters=2, dup=60)
    words = np_encode(v, D)
    present = np.ones(N, bool)
    ids, sc = random_rows(words, D, R, present, 8)
    marked = marked_sets(N, present, 2)["50%"]
    tasks = emu_affected(emu, ids, present, marked)
    base = emu_merge(emu, words, D, ids, sc, marked, tasks, 400, 1)
    try:
        for order in ("reverse", "random:5"):
            os.environ["EMU_LANE_ORDER"] = order
            assert np.array_equal(emu_affected(emu, ids, present, marked), tasks)
            got = emu_merge(emu, words, D, ids, sc, marked, tasks, 400, 1)
            assert all(np.array_equal(a, b, equal_nan=a.dtype.kind == "f") for a, b in zip(got, base))
    finally:
        os.environ.pop("EMU_LANE_ORDER", None)
