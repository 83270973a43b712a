"""Graph search scored on NVQ rows alone on the GPU (include/jvector_nvq_graph.h): GraphSearcher.search with
NVQVectors.scoreFunctionFor as the score function — no float rows, no other quantizer, no rerank.  Thin ctypes calls, as in
exact_graph.py: no arithmetic here, no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .engine import GraphIndex, HipContext, NVQVectors, _empty, _ptr, pack_accept_bits

_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/jvector_nvq_graph.h one to one
NVQ_GRAPH_SIGNATURES = {
    "jv_hip_nvq_graph_search": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _i64, _p, _p, _p]),
    "jv_hip_nvq_graph_max_beam_k": (_i, [_p, _p, C.POINTER(_i)]),
}


def lib():
    """the product library with NVQ_GRAPH_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_nvq_graph_bound", False):
        for name, (res, args) in NVQ_GRAPH_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_nvq_graph_bound = True
    return lb


class NVQGraphSearcher:
    """Batched GraphSearcher over a GraphIndex (built any way) scored with the rows of an NVQVectors: one wavefront per query runs the
    whole search loop on the GPU, de-quantising the fresh neighbours of every expansion across the wave; the first top_k of the beam_k
    kept results come back in NodeQueue order with NVQScorer's scores.  Results, visitedCount and expandedCount equal the reference's
    sequential search over the same rows."""

    def __init__(self, ctx: HipContext, graph: GraphIndex, nvq_vectors: NVQVectors):
        self.ctx, self.graph, self.nvq_vectors = ctx, graph, nvq_vectors
        self._lib = lib()

    def max_beam_k(self) -> int:
        """largest beamK the device kernel takes (a larger one raises UnsupportedError)"""
        out = C.c_int()
        check(self._lib.jv_hip_nvq_graph_max_beam_k(self.ctx._h, self.graph._h, C.byref(out)))
        return out.value

    def search(self, queries, vsf, topK, beamK=0, accept=None, return_stats=False, out_ids=None, out_scores=None):
        """queries [Q, D] float32 (numpy in -> numpy out, a device torch tensor in -> device tensors out).  beamK 0 = topK.
        accept = acceptOrds: None, a bool array [n_nodes] shared by the batch, or [Q, n_nodes] one filter per query; filtered-out
        nodes are traversed but never returned.  return_stats: also int64 [Q, 2] = {visitedCount, expandedCount}."""
        Q = int(queries.shape[0])
        q_p, qk = _ptr(queries, np.float32)
        if out_ids is None:
            out_ids = _empty((Q, topK), np.int32, queries)
        if out_scores is None:
            out_scores = _empty((Q, topK), np.float32, queries)
        oi_p, oik = _ptr(out_ids, np.int32)
        os_p, osk = _ptr(out_scores, np.float32)
        stats = np.zeros((Q, 2), np.int64)
        mask_p, stride, mask = None, 0, None
        if accept is not None:
            mask = pack_accept_bits(accept, self.graph.n_nodes)
            if mask.ndim == 2:
                if mask.shape[0] != Q:
                    raise ValueError(f"accept has {mask.shape[0]} rows for {Q} queries")
                stride = int(mask.shape[1])
            mask_p = C.c_void_p(mask.ctypes.data)
        check(self._lib.jv_hip_nvq_graph_search(
            self.ctx._h, self.graph._h, self.nvq_vectors._h, q_p, Q, int(vsf), int(topK), int(beamK), mask_p, stride, oi_p, os_p,
            C.c_void_p(stats.ctypes.data) if return_stats else None))
        return (out_ids, out_scores, stats) if return_stats else (out_ids, out_scores)
