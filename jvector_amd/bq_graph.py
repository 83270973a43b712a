"""Graph search over binary-quantized vectors on the GPU (include/jvector_bq_graph.h): GraphSearcher.search with
BQVectors.scoreFunctionFor as the approximate score and an exact reranker.  Thin ctypes calls, as in bq.py: no arithmetic here, no
CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .bq import BQVectors
from .engine import GraphIndex, HipContext, VectorSet, _empty, _ptr, pack_accept_bits

_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/jvector_bq_graph.h one to one
BQ_GRAPH_SIGNATURES = {
    "jv_hip_bq_graph_search": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _i64, _p, _p, _p]),
    "jv_hip_bq_graph_max_rerank_k": (_i, [_p, _p, C.POINTER(_i)]),
}


def lib():
    """the product library with BQ_GRAPH_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_bq_graph_bound", False):
        for name, (res, args) in BQ_GRAPH_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_bq_graph_bound = True
    return lb


class BQGraphSearcher:
    """Batched GraphSearcher over a GraphIndex (built any way) scored with BQVectors: one wavefront per query runs the whole search
    loop on the GPU; the approximate results (at most rerank_k) are reranked with the exact scores of `vectors` and the top K come
    back in NodeQueue order.  vectors None: the approximate top K with their BQ similarities.  Results, visitedCount and
    expandedCount equal the reference's sequential search."""

    def __init__(self, ctx: HipContext, graph: GraphIndex, bq_vectors: BQVectors, vectors: VectorSet | None = None):
        self.ctx, self.graph, self.bq, self.vectors = ctx, graph, bq_vectors, vectors
        self._lib = lib()

    def max_rerank_k(self) -> int:
        """largest rerank_k the device kernel takes (a larger one raises UnsupportedError)"""
        out = C.c_int()
        check(self._lib.jv_hip_bq_graph_max_rerank_k(self.ctx._h, self.graph._h, C.byref(out)))
        return out.value

    def search(self, queries, vsf, top_k, rerank_k=None, accept=None, out_ids=None, out_scores=None, return_stats=False, accept_bits=None):
        """queries [Q, D] float32 (numpy in -> numpy out, a device torch tensor in -> device tensors out).  rerank_k None = top_k.
        accept = acceptOrds: None, a bool array [n_nodes] shared by the batch, or [Q, n_nodes] one filter per query; filtered-out
        nodes are traversed but never returned.  accept_bits: instead of `accept`, one mask for the batch already packed — uint64
        [ceil(n_nodes / 64)] host words, bit n of word n // 64 (what BQGraphBuilder.live_bits returns).  return_stats: also int64 [Q, 2] = {visitedCount, expandedCount}."""
        Q = int(queries.shape[0])
        rerank_k = int(top_k) if rerank_k is None else int(rerank_k)
        q_p, qk = _ptr(queries, np.float32)
        if out_ids is None:
            out_ids = _empty((Q, top_k), np.int32, queries)
        if out_scores is None:
            out_scores = _empty((Q, top_k), np.float32, queries)
        oi_p, oik = _ptr(out_ids, np.int32)
        os_p, osk = _ptr(out_scores, np.float32)
        stats = np.zeros((Q, 2), np.int64)
        mask_p, stride, mask = None, 0, None
        if accept_bits is not None:
            if accept is not None:
                raise ValueError("accept and accept_bits are two forms of one argument")
            mask = np.ascontiguousarray(accept_bits, np.uint64)
            if mask.shape != ((self.graph.n_nodes + 63) // 64,):
                raise ValueError(f"accept_bits has shape {mask.shape}, the graph has {self.graph.n_nodes} nodes")
            mask_p = C.c_void_p(mask.ctypes.data)
        elif accept is not None:
            mask = pack_accept_bits(accept, self.graph.n_nodes)
            if mask.ndim == 2:
                if mask.shape[0] != Q:
                    raise ValueError(f"accept has {mask.shape[0]} rows for {Q} queries")
                stride = int(mask.shape[1])
            mask_p = C.c_void_p(mask.ctypes.data)
        check(self._lib.jv_hip_bq_graph_search(
            self.ctx._h, self.graph._h, self.bq._h, self.vectors._h if self.vectors is not None else None, q_p, Q, int(vsf),
            int(top_k), rerank_k, mask_p, stride, oi_p, os_p, C.c_void_p(stats.ctypes.data) if return_stats else None))
        return (out_ids, out_scores, stats) if return_stats else (out_ids, out_scores)
