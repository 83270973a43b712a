"""Build-time scoring over binary-quantized vectors on the GPU (include/jvector_bq_build.h): the two calls graph construction makes
per inserted node with BuildScoreProvider.bqBuildScoreProvider — the search whose query is a stored BQ row, and the robust prune
scored row against row — batched.  Thin ctypes calls, as in bq_graph.py: no arithmetic here, no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .bq import BQVectors
from .engine import GraphIndex, HipContext, _empty, _ptr

_p = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes); mirrors include/jvector_bq_build.h one to one
BQ_BUILD_SIGNATURES = {
    "jv_hip_bq_retain_diverse": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, _i, C.c_float, _p, _p, _p]),
    "jv_hip_bq_retain_diverse_max_candidates": (_i, [_p, _p, _i, C.POINTER(_i)]),
    "jv_hip_bq_graph_search_nodes": (_i, [_p, _p, _p, _p, _i, _i, _i, _p, _p, _p]),
}


def lib():
    """the product library with BQ_BUILD_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_bq_build_bound", False):
        for name, (res, args) in BQ_BUILD_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_bq_build_bound = True
    return lb


class BQBuildScorer:
    """bqBuildScoreProvider(BQVectors) for batches of nodes: search_nodes is GraphSearcher.search(searchProviderFor(node), k, k, 0, 0,
    Bits.ALL) over `graph`, retain_diverse is VamanaDiversityProvider.retainDiverse with diversityScoreFunctionFor.  graph may be None
    for a scorer that only prunes."""

    def __init__(self, ctx: HipContext, graph: GraphIndex | None, bq_vectors: BQVectors):
        self.ctx, self.graph, self.bq = ctx, graph, bq_vectors
        self._lib = lib()

    def max_candidates(self, max_degree) -> int:
        """largest candidate list retain_diverse takes for these rows (a longer one raises UnsupportedError)"""
        out = C.c_int()
        check(self._lib.jv_hip_bq_retain_diverse_max_candidates(self.ctx._h, self.bq._h, int(max_degree), C.byref(out)))
        return out.value

    def search_nodes(self, nodes, top_k, exclude_self=False, return_stats=False):
        """nodes [Q] int32 ordinals of BQ rows (numpy in -> numpy out, a device torch tensor in -> device tensors out): the
        approximate top_k of each row's own search, ids [Q, top_k] (-1 padded) and BQ similarities (-inf padded) in NodeQueue order.
        exclude_self: node nodes[q] is traversed but never returned to item q.  return_stats: also int64 [Q, 2] = {visitedCount,
        expandedCount}.  An ordinal outside the rows raises ValueError for host input; in a device tensor it gives an empty row."""
        Q = int(nodes.shape[0])
        n_p, kn = _ptr(nodes, np.int32)
        out_ids = _empty((Q, top_k), np.int32, nodes)
        out_scores = _empty((Q, top_k), np.float32, nodes)
        oi_p, oik = _ptr(out_ids, np.int32)
        os_p, osk = _ptr(out_scores, np.float32)
        stats = np.zeros((Q, 2), np.int64)
        check(self._lib.jv_hip_bq_graph_search_nodes(
            self.ctx._h, self.graph._h if self.graph is not None else None, self.bq._h, n_p, Q, int(top_k), 1 if exclude_self else 0,
            oi_p, os_p, C.c_void_p(stats.ctypes.data) if return_stats else None))
        return (out_ids, out_scores, stats) if return_stats else (out_ids, out_scores)

    def retain_diverse(self, cand_nodes, cand_scores, max_degree, alpha, cand_count=None, diverse_before=None):
        """cand_nodes / cand_scores [P, C]: one NodeArray per row (cand_count [P]: its length, default C; diverse_before [P]: leading
        entries already diverse, default 0).  Returns (selected [P, max_degree] candidate positions ascending, -1 padded;
        n_selected [P]; short_edges [P])."""
        P, Cn = int(cand_nodes.shape[0]), int(cand_nodes.shape[1])
        n_p, kn = _ptr(cand_nodes, np.int32)
        s_p, ks = _ptr(cand_scores, np.float32)
        c_p, kc = _ptr(cand_count, np.int32)
        d_p, kd = _ptr(diverse_before, np.int32)
        sel = _empty((P, max_degree), np.int32, cand_nodes)
        cnt = _empty((P,), np.int32, cand_nodes)
        se = _empty((P,), np.float32, cand_nodes)
        sel_p, k1 = _ptr(sel, np.int32)
        cnt_p, k2 = _ptr(cnt, np.int32)
        se_p, k3 = _ptr(se, np.float32)
        check(self._lib.jv_hip_bq_retain_diverse(self.ctx._h, self.bq._h, P, Cn, n_p, s_p, c_p, d_p, int(max_degree), C.c_float(alpha),
                                                 sel_p, cnt_p, se_p))
        return sel, cnt, se
