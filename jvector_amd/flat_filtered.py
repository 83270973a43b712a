"""The flat PQ search under an accept filter (include/jvector_flat_filtered.h): the accept masks are compacted to ordinal lists on the
device and only the accepted rows are scored.  The signature table and its binding live here; FlatSearcher.search_filtered calls
search_flat_filtered.  Thin ctypes, no arithmetic on scores, no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .engine import _empty, _is_torch, _ptr

_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64

# name -> (restype, argtypes); mirrors include/jvector_flat_filtered.h one to one
FLAT_FILTERED_SIGNATURES = {
    "jv_hip_search_flat_filtered": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _i64, C.c_int32, _p, _p, _p]),
}

# rows one scan block of the mask compaction covers (FA_SCAN_ROWS of jvector_amd/csrc/fa_params.h)
SCAN_ROWS = 16384


def lib():
    """the product library with FLAT_FILTERED_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_flat_filtered_bound", False):
        for name, (res, args) in FLAT_FILTERED_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_flat_filtered_bound = True
    return lb


def pack_accept(accept):
    """bool [N] or [Q, N] (numpy or torch) -> uint64 words [ceil(N / 64)] or [Q, ceil(N / 64)], bit n of word n // 64 <-> row n
    (little-endian bit order; the padding bits of the last word are clear)"""
    a = np.asarray(accept.cpu().numpy() if _is_torch(accept) else accept, dtype=bool)
    if a.ndim not in (1, 2):
        raise ValueError(f"accept must be [N] or [Q, N], got shape {a.shape}")
    pad = (-a.shape[-1]) % 64
    a = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, pad)])
    return np.ascontiguousarray(np.packbits(a, axis=-1, bitorder="little").view(np.uint64))


def _mask_ptr(accept, n_rows, Q, accept_stride_words):
    """(pointer, stride in words, keepalive) of an accept argument: None, a bool array, or packed 64-bit words (host or device)"""
    if accept is None:
        return None, 0, None
    words = (n_rows + 63) // 64
    if _is_torch(accept):
        import torch
        if accept.dtype == torch.bool:
            accept = pack_accept(accept)
        elif accept.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
            raise ValueError(f"accept: expected bool or 64-bit words, got {accept.dtype}")
    elif np.asarray(accept).dtype == bool:
        accept = pack_accept(accept)
    if not _is_torch(accept):
        accept = np.ascontiguousarray(accept, dtype=np.uint64)
    elif not accept.is_contiguous():
        raise ValueError("tensor must be contiguous")
    stride = int(accept_stride_words)
    if accept.ndim == 2:
        if int(accept.shape[0]) != Q:
            raise ValueError(f"accept has {accept.shape[0]} rows for {Q} queries")
        stride = stride or int(accept.shape[1])
    cells = int(np.prod(accept.shape))
    if cells < (stride * (Q - 1) + words if stride else words):
        raise ValueError(f"accept holds {cells} words, {stride * (Q - 1) + words if stride else words} are needed")
    return C.c_void_p(accept.data_ptr() if _is_torch(accept) else accept.ctypes.data), stride, accept


def search_flat_filtered(searcher, queries, vsf, top_k, rerank_k, accept, accept_stride_words=0, accepted_out=None, out_ids=None,
                         out_scores=None):
    """jv_hip_search_flat_filtered over a FlatSearcher's code set.  accept: None (no filter), bool [N] / [Q, N], or packed uint64
    words (numpy, or a torch int64 tensor in device memory) — flat words take accept_stride_words (0: one mask for the batch).
    accepted_out: optional int64 [Q] numpy array that receives the accepted rows per query.  Returns (ids, scores)."""
    Q = int(queries.shape[0])
    q_p, qk = _ptr(queries, np.float32)
    if out_ids is None:
        out_ids = _empty((Q, top_k), np.int32, queries)
    if out_scores is None:
        out_scores = _empty((Q, top_k), np.float32, queries)
    oi_p, oik = _ptr(out_ids, np.int32)
    os_p, osk = _ptr(out_scores, np.float32)
    m_p, stride, mk = _mask_ptr(accept, searcher.cv.count(), Q, accept_stride_words)
    a_p = None
    if accepted_out is not None:
        if not (isinstance(accepted_out, np.ndarray) and accepted_out.dtype == np.int64 and accepted_out.flags.c_contiguous
                and accepted_out.size >= Q):
            raise ValueError("accepted_out must be a contiguous int64 numpy array of at least Q entries")
        a_p = C.c_void_p(accepted_out.ctypes.data)
    check(lib().jv_hip_search_flat_filtered(searcher.ctx._h, searcher.luts._h, searcher.cv._h,
                                            searcher.vectors._h if searcher.vectors is not None else None, q_p, Q, int(vsf),
                                            int(top_k), int(rerank_k), m_p, stride, searcher.id_base, oi_p, os_p, a_p))
    return out_ids, out_scores
