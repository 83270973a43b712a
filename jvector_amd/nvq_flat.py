"""The NVQ flat search (include/jvector_nvq_flat.h): the nearest neighbours of a query batch among the NVQ rows an accept filter
admits, in one call — an MFMA tile kernel that de-quantises each chunk of rows once for 128 queries, with the selecting epilogue of
the exact flat search, the NVQScorer rescoring of the candidates and the final top-k.  Context options nvq_flat_fused,
nvq_flat_sample_stride, nvq_flat_cap, nvq_flat_score_bytes; counters nvq_flat_calls, nvq_flat_fused_calls, nvq_flat_fallbacks,
nvq_flat_listed.  The signature table and its binding live here; NVQVectors.search_flat calls search_flat.  Thin ctypes, no
arithmetic on scores, no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .engine import _empty, _ptr
from .flat_filtered import _mask_ptr

_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/jvector_nvq_flat.h one to one
NVQ_FLAT_SIGNATURES = {
    "jv_hip_nvq_search_flat": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _i64, C.c_int32, _p, _p]),
}


def lib():
    """the product library with NVQ_FLAT_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_nvq_flat_bound", False):
        for name, (res, args) in NVQ_FLAT_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_nvq_flat_bound = True
    return lb


def search_flat(ctx, nv, queries, vsf, top_k, cand_k=0, accept=None, accept_stride_words=0, id_base=0, out_ids=None, out_scores=None):
    """jv_hip_nvq_search_flat over an NVQVectors.  accept: None (no filter), bool [N] / [Q, N] (packed by flat_filtered.pack_accept),
    or packed uint64 words (numpy, or a torch int64 tensor in device memory) — flat words take accept_stride_words (0: one mask for
    the batch).  cand_k = 0 returns the top_k of the tile scores; cand_k >= top_k rescores that many candidates with NVQScorer's bits
    first.  Returns (ids, scores)."""
    Q = int(queries.shape[0])
    q_p, qk = _ptr(queries, np.float32)
    if out_ids is None:
        out_ids = _empty((Q, top_k), np.int32, queries)
    if out_scores is None:
        out_scores = _empty((Q, top_k), np.float32, queries)
    oi_p, oik = _ptr(out_ids, np.int32)
    os_p, osk = _ptr(out_scores, np.float32)
    m_p, stride, mk = _mask_ptr(accept, nv.count(), Q, accept_stride_words)
    check(lib().jv_hip_nvq_search_flat(ctx._h, nv._h, q_p, Q, int(vsf), int(top_k), int(cand_k), m_p, stride, int(id_base), oi_p, os_p))
    return out_ids, out_scores
