"""Graph construction from binary-quantized vectors alone on the GPU (include/jvector_bq_builder.h): GraphIndexBuilder driven by
BuildScoreProvider.bqBuildScoreProvider — no codebook, no training, no full-resolution vectors.  Thin ctypes calls, as in bq_build.py:
no arithmetic here, no CPU fallback."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib
from ._lib import check
from .bq import BQVectors
from .bq_compact import lib as _compact_lib
from .builder import BuildStats
from .engine import GraphIndex, HipContext, _ptr

_p = C.c_void_p
_i = C.c_int
_f = C.c_float

# name -> (restype, argtypes); mirrors include/jvector_bq_builder.h one to one
BQ_BUILDER_SIGNATURES = {
    "jv_hip_bq_builder_create": (_i, [_p, _p, _i, _i, _f, _f, C.POINTER(_p)]),
    "jv_hip_bq_builder_seed": (_i, [_p, _p, C.c_int32]),
    "jv_hip_bq_builder_insert_batch": (_i, [_p, _p, _p, _i]),
    "jv_hip_bq_builder_improve_batch": (_i, [_p, _p, _p, _i]),
    "jv_hip_bq_builder_finish": (_i, [_p, _p, _p]),
    "jv_hip_bq_builder_stats": (_i, [_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "jv_hip_bq_builder_working_lists": (_i, [_p, _p, _p, _p, _p]),
    "jv_hip_bq_builder_neighbors_device": (_p, [_p, C.POINTER(_i)]),
    "jv_hip_bq_builder_destroy": (_i, [_p]),
    "jv_hip_bq_build_layered": (_i, [_p, _p, _i, _i, _f, _f, _i, _i, C.c_uint64, _i, C.POINTER(_p)]),
}

# the deletion half of the builder's ABI; mirrors include/jvector_bq_delete.h one to one
BQ_DELETE_SIGNATURES = {
    "jv_hip_bq_builder_mark_deleted": (_i, [_p, _p, _p, _i]),
    "jv_hip_bq_builder_deleted_count": (_i, [_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "jv_hip_bq_builder_live_bits": (_i, [_p, _p, _p]),
    "jv_hip_bq_builder_remove_deleted": (_i, [_p, _p, C.c_uint64, C.POINTER(C.c_int64)]),
    "jv_hip_bq_builder_entry": (C.c_int32, [_p]),
}


def lib():
    """the product library with BQ_BUILDER_SIGNATURES and BQ_DELETE_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_bq_builder_bound", False):
        for name, (res, args) in list(BQ_BUILDER_SIGNATURES.items()) + list(BQ_DELETE_SIGNATURES.items()):
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_bq_builder_bound = True
    return lb


class BQGraphBuilder:
    """jv_bq_builder: one graph level over the rows of `bq_vectors`; the mirror of builder.GraphBuilder."""

    def __init__(self, ctx: HipContext, bq_vectors: BQVectors, max_degree=32, beam_width=100, alpha=1.2, overflow=1.25, handle=None):
        """handle: a jv_bq_builder over `bq_vectors` that exists already (compact makes one); its parameters are the handle's"""
        self.ctx, self._lib, self._keep = ctx, lib(), bq_vectors
        self.n, self.max_degree = int(bq_vectors.count()), int(max_degree)
        if handle is None:
            handle = C.c_void_p()
            check(self._lib.jv_hip_bq_builder_create(ctx._h, bq_vectors._h, int(max_degree), int(beam_width), float(alpha), float(overflow),
                                                     C.byref(handle)))
        self._h = handle

    def seed(self, node):
        check(self._lib.jv_hip_bq_builder_seed(self.ctx._h, self._h, int(node)))

    def insert_batch(self, nodes):
        """nodes: int32 ordinals (torch tensor on the device, or a numpy array), none inserted before"""
        p, _k = _ptr(nodes, np.int32)
        check(self._lib.jv_hip_bq_builder_insert_batch(self.ctx._h, self._h, p, int(nodes.shape[0])))

    def improve_batch(self, nodes):
        """improveConnections for nodes that are in the graph: search, merge with the node's neighbours, robust prune, backlink"""
        p, _k = _ptr(nodes, np.int32)
        check(self._lib.jv_hip_bq_builder_improve_batch(self.ctx._h, self._h, p, int(nodes.shape[0])))

    def finish(self, out):
        """enforceDegree; `out` [n, max_degree] int32 (torch / numpy) receives the packed, -1 padded rows"""
        p, _k = _ptr(out, np.int32)
        check(self._lib.jv_hip_bq_builder_finish(self.ctx._h, self._h, p))
        return out

    def row_width(self):
        w = C.c_int()
        self._lib.jv_hip_bq_builder_neighbors_device(self._h, C.byref(w))
        return int(w.value)

    def working_rows(self):
        """the lists as they stand (host arrays): ids [n, row_width], the scores their entries were inserted under, diverseBefore marks"""
        R = self.row_width()
        ids = np.empty((self.n, R), np.int32)
        sc = np.empty((self.n, R), np.float32)
        db = np.empty(self.n, np.int32)
        check(self._lib.jv_hip_bq_builder_working_lists(self.ctx._h, self._h, ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p),
                                                        db.ctypes.data_as(C.c_void_p)))
        return ids, sc, db

    def stats(self):
        s, c = (C.c_double * 3)(), (C.c_int64 * 5)()
        check(self._lib.jv_hip_bq_builder_stats(self._h, s, c))
        return BuildStats(search_s=s[0], prune_s=s[1], backlink_s=s[2], batches=int(c[0]), reprunes=int(c[1]), inserted=int(c[2]),
                          visited=int(c[3]), expanded=int(c[4]))

    def mark_deleted(self, nodes):
        """markNodeDeleted for int32 ordinals that are in the graph (torch tensor on the device, or a numpy array); they stay ordinary
        nodes until remove_deleted, and live_bits() hides them from a search"""
        p, _k = _ptr(nodes, np.int32)
        check(self._lib.jv_hip_bq_builder_mark_deleted(self.ctx._h, self._h, p, int(nodes.shape[0])))

    def remove_deleted(self, seed=0):
        """removeDeletedNodes: the rows of the live nodes with a marked neighbour are repaired, the marked nodes leave the graph.
        Returns dict(removed, rewritten, candidates, fallback)."""
        c = (C.c_int64 * 4)()
        check(self._lib.jv_hip_bq_builder_remove_deleted(self.ctx._h, self._h, int(seed), c))
        return dict(removed=int(c[0]), rewritten=int(c[1]), candidates=int(c[2]), fallback=int(c[3]))

    def live_bits(self):
        """uint64 [ceil(n / 64)] (host): bit i set = node i is in the graph and not marked; BQGraphSearcher's accept_bits"""
        out = np.empty((self.n + 63) // 64, np.uint64)
        check(self._lib.jv_hip_bq_builder_live_bits(self.ctx._h, self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def deleted_counts(self):
        """(nodes marked and not yet removed, nodes removed so far)"""
        m, r = C.c_int64(), C.c_int64()
        check(self._lib.jv_hip_bq_builder_deleted_count(self._h, C.byref(m), C.byref(r)))
        return int(m.value), int(r.value)

    @property
    def entry(self):
        """the node a search of the working graph starts from; -1: the graph is empty"""
        return int(self._lib.jv_hip_bq_builder_entry(self._h))

    def renumbering(self):
        """sequentialRenumbering of the graph: (old_to_new int32 [n], -1 for a row not in the graph; new_to_old int32 [live]), host arrays"""
        o2n = np.empty(self.n, np.int32)
        n2o = np.empty(max(1, self.stats()["inserted"]), np.int32)
        live = C.c_int64()
        check(_compact_lib().jv_hip_bq_builder_renumbering(self.ctx._h, self._h, o2n.ctypes.data_as(C.c_void_p), n2o.ctypes.data_as(C.c_void_p),
                                                           C.byref(live)))
        return o2n, n2o[:int(live.value)]

    def compact(self, dst_bq: BQVectors):
        """a NEW BQGraphBuilder over `dst_bq` (same dimension, at least max(live, 1) rows, not this builder's own vectors) holding this
        graph under the sequential renumbering: rows [0, live) of dst_bq receive the live nodes' BQ rows, its other rows are left alone
        and are free ids of the new builder.  Nothing is marked when this is called.  Returns (builder, old_to_new, new_to_old); this
        builder is not changed."""
        o2n = np.empty(self.n, np.int32)
        n2o = np.empty(max(1, self.stats()["inserted"]), np.int32)
        live, h = C.c_int64(), C.c_void_p()
        check(_compact_lib().jv_hip_bq_builder_compact(self.ctx._h, self._h, dst_bq._h, o2n.ctypes.data_as(C.c_void_p),
                                                       n2o.ctypes.data_as(C.c_void_p), C.byref(live), C.byref(h)))
        return BQGraphBuilder(self.ctx, dst_bq, self.max_degree, handle=h), o2n, n2o[:int(live.value)]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.jv_hip_bq_builder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_bq_layered(ctx: HipContext, bq_vectors: BQVectors, max_degree=32, beam_width=100, alpha=1.2, overflow=1.25, max_batch=131072, improve=0,
                     seed=11, min_top=8, log=None) -> GraphIndex:
    """jv_hip_bq_build_layered: the layered graph of builder.build_hierarchical from BQ rows alone, all inside the library.  Returns a
    GraphIndex (what BQGraphSearcher takes) that also carries `levels` (levels[l] = (None | ascending int32 node ids, int32 neighbour
    rows), host arrays), `entry_node`, `entry_level` and `build_stats`."""
    lb = lib()
    N = int(bq_vectors.count())
    h = C.c_void_p()
    t0 = time.perf_counter()
    check(lb.jv_hip_bq_build_layered(ctx._h, bq_vectors._h, int(max_degree), int(beam_width), float(alpha), float(overflow), int(max_batch),
                                     int(improve), int(seed), int(min_top), C.byref(h)))
    try:
        n_lv, entry, entry_level = C.c_int(), C.c_int32(), C.c_int()
        check(lb.jv_hip_layered_info(h, C.byref(n_lv), C.byref(entry), C.byref(entry_level), None))
        counts = (C.c_int64 * n_lv.value)()
        check(lb.jv_hip_layered_info(h, None, None, None, counts))
        nb0 = np.empty((N, max_degree), np.int32)
        check(lb.jv_hip_layered_level(ctx._h, h, 0, None, nb0.ctypes.data_as(C.c_void_p)))
        levels = [(None, nb0)]
        for l in range(1, n_lv.value):
            ids = np.empty(int(counts[l]), np.int32)
            rows = np.empty((int(counts[l]), max_degree), np.int32)
            check(lb.jv_hip_layered_level(ctx._h, h, l, ids.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p)))
            levels.append((ids, rows))
        sec, cnt = (C.c_double * 4)(), (C.c_int64 * 5)()
        check(lb.jv_hip_layered_stats(h, sec, cnt))
    finally:
        lb.jv_hip_layered_destroy(h)
    stats = BuildStats(search_s=sec[0], prune_s=sec[1], backlink_s=sec[2], batches=int(cnt[0]), reprunes=int(cnt[1]), inserted=int(cnt[2]),
                       visited=int(cnt[3]), expanded=int(cnt[4]), total_s=sec[3], wall_s=time.perf_counter() - t0,
                       levels=[int(c) for c in counts])
    if log:
        log(f"[bq build] layered: {stats['levels']} nodes per level in {stats['total_s']:.1f}s (search {sec[0]:.1f}s prune {sec[1]:.1f}s backlink {sec[2]:.1f}s)")
    g = GraphIndex(ctx, N, levels, int(entry.value), int(entry_level.value))
    g.levels, g.entry_node, g.entry_level, g.build_stats = levels, int(entry.value), int(entry_level.value), stats
    return g
