"""The exact flat search (include/jvector_exact_flat.h): the true nearest neighbours of a query batch among the float rows an accept
filter admits, in one call — the MFMA tile kernel of the dense scan with an epilogue that selects instead of storing, the bit-exact
rescoring of the candidates and the final top-k.  Context options exact_flat_fused, exact_flat_sample_stride, exact_flat_cap,
exact_flat_score_bytes; counters exact_flat_calls, exact_flat_fused_calls, exact_flat_fallbacks, exact_flat_listed.  The signature
table and its binding live here; VectorSet.search_exact calls search_exact.  Thin ctypes, no arithmetic on scores, no CPU fallback."""
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

# name -> (restype, argtypes); mirrors include/jvector_exact_flat.h one to one
EXACT_FLAT_SIGNATURES = {
    "jv_hip_search_exact": (_i, [_p, _p, _p, _i, _i, _i, _i, _p, _i64, C.c_int32, _p, _p]),
}


def lib():
    """the product library with EXACT_FLAT_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_exact_flat_bound", False):
        for name, (res, args) in EXACT_FLAT_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_exact_flat_bound = True
    return lb


def search_exact(ctx, vectors, queries, vsf, top_k, cand_k=0, accept=None, accept_stride_words=0, id_base=0, out_ids=None,
                 out_scores=None):
    """jv_hip_search_exact over a VectorSet.  accept: None (no filter), bool [N] / [Q, N] (packed by flat_filtered.pack_accept), or
    packed uint64 words (numpy, or a torch int64 tensor in device memory) — flat words take accept_stride_words (0: one mask for the
    batch).  cand_k = 0 returns the top_k of the fused-chain scores; cand_k >= top_k rescores that many candidates bit-exactly first.
    Returns (ids, scores)."""
    Q = int(queries.shape[0])
    q_p, qk = _ptr(queries, np.float32)
    if out_ids is None:
        out_ids = _empty((Q, top_k), np.int32, queries)
    if out_scores is None:
        out_scores = _empty((Q, top_k), np.float32, queries)
    oi_p, oik = _ptr(out_ids, np.int32)
    os_p, osk = _ptr(out_scores, np.float32)
    m_p, stride, mk = _mask_ptr(accept, vectors.count, Q, accept_stride_words)
    check(lib().jv_hip_search_exact(ctx._h, vectors._h, q_p, Q, int(vsf), int(top_k), int(cand_k), m_p, stride, int(id_base), oi_p, os_p))
    return out_ids, out_scores
