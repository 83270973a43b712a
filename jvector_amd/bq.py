"""Binary quantization on the GPU (include/jvector_bq.h): BinaryQuantization (B/quantization/BinaryQuantization.java), BQVectors
(B/quantization/BQVectors.java) and a flat searcher over them.  Thin ctypes calls, as in engine.py: no arithmetic here, no CPU
fallback.  Words are uint64 in the reference's bit order (bit j of word i <-> dimension 64 i + j)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .engine import HipContext, VectorSet, _finalizer, _is_torch, _ptr, pack_accept_bits

_p = C.c_void_p
_i = C.c_int
_i64 = C.c_int64
_sz = C.c_size_t

# name -> (restype, argtypes); mirrors include/jvector_bq.h one to one
BQ_SIGNATURES = {
    "jv_hip_bq_create": (_i, [_p, _i, _i64, C.POINTER(_p)]),
    "jv_hip_bq_upload": (_i, [_p, _p, _i64, _i64, _p]),
    "jv_hip_bq_download": (_i, [_p, _p, _i64, _i64, _p]),
    "jv_hip_bq_count": (_i64, [_p]),
    "jv_hip_bq_dimension": (_i, [_p]),
    "jv_hip_bq_destroy": (_i, [_p]),
    "jv_hip_bq_encode_into": (_i, [_p, _p, _i64, _i64, _p, _i64]),
    "jv_hip_bq_encode": (_i, [_p, _i, _p, _i64, _p]),
    "jv_hip_bq_describe": (_i, [_p, _sz, C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i), C.POINTER(_sz), C.POINTER(_sz)]),
    "jv_hip_bq_load": (_i, [_p, _p, _sz, C.POINTER(_sz), C.POINTER(_p)]),
    "jv_hip_bq_write": (_i, [_p, _p, _p, _sz, C.POINTER(_sz)]),
    "jv_hip_bq_scores": (_i, [_p, _p, _p, _i, _p, _i, _p]),
    "jv_hip_bq_pair_scores": (_i, [_p, _p, _p, _i, _p, _i, _p]),
    "jv_hip_bq_search_flat": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _i64, C.c_int32, _p, _p]),
}


def lib():
    """the product library with BQ_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_bq_bound", False):
        for name, (res, args) in BQ_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_bq_bound = True
    return lb


def words_per_vector(dimension: int) -> int:
    return (int(dimension) + 63) // 64


def describe(data: bytes) -> dict:
    """jv_hip_bq_describe: the fields of a BinaryQuantization + BQVectors block (host only, no device)"""
    buf = (C.c_ubyte * max(1, len(data))).from_buffer_copy(data or b"\0")
    D, cnt, W, off, blen = C.c_int(), C.c_int64(), C.c_int(), C.c_size_t(), C.c_size_t()
    check(lib().jv_hip_bq_describe(C.cast(buf, C.c_void_p), len(data), C.byref(D), C.byref(cnt), C.byref(W), C.byref(off),
                                   C.byref(blen)))
    return {"dimension": D.value, "count": cnt.value, "words": W.value, "data_offset": off.value, "block_len": blen.value}


def _u64(x):
    if x is None:
        return None, None
    if _is_torch(x):
        import torch
        if x.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
            raise ValueError(f"expected a 64-bit integer tensor, got {x.dtype}")
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return C.c_void_p(x.data_ptr()), x
    a = np.ascontiguousarray(x, dtype=np.uint64)
    return C.c_void_p(a.ctypes.data), a


def _empty_u64(shape, like):
    if like is not None and _is_torch(like) and like.is_cuda:
        import torch
        return torch.empty(shape, dtype=torch.int64, device=like.device)   # (torch's int64 holds the same bits)
    return np.empty(shape, np.uint64)


class BinaryQuantization:
    """BinaryQuantization(dimension): no codebook, no training.  encode / encode_all run on the device."""

    def __init__(self, ctx: HipContext, dimension: int):
        if int(dimension) < 1:
            raise ValueError(f"dimension {dimension} < 1")
        self.ctx, self.dimension = ctx, int(dimension)

    def compressed_vector_size(self) -> int:
        return 8 * words_per_vector(self.dimension)

    def encode(self, vectors, out=None):
        """rows (n, D) float32 (numpy or torch, host or device; a single vector is one row) -> (n, W) uint64 words
        (a device torch tensor in -> a device int64 tensor out)"""
        single = len(vectors.shape) == 1
        v = vectors.reshape(1, -1) if single else vectors
        n = int(v.shape[0])
        if int(v.shape[1]) != self.dimension:
            raise ValueError(f"vector dimensions differ: {v.shape[1]}!={self.dimension}")
        v_p, vk = _ptr(v, np.float32)
        if out is None:
            out = _empty_u64((n, words_per_vector(self.dimension)), v)
        o_p, ok = _u64(out)
        check(lib().jv_hip_bq_encode(self.ctx._h, self.dimension, v_p, n, o_p))
        return out[0] if single else out

    def encode_all(self, vectors: VectorSet, first=0, count=None) -> "BQVectors":
        """encodeAll: rows [first, first + count) of a device-resident VectorSet into new BQVectors"""
        count = vectors.count - first if count is None else int(count)
        out = BQVectors(self.ctx, self.dimension, count=count)
        check(lib().jv_hip_bq_encode_into(self.ctx._h, vectors._h, int(first), count, out._h, 0))
        return out


@_finalizer
class BQVectors:
    """BQVectors resident on the device: count x W uint64 words."""

    def __init__(self, ctx: HipContext, dimension: int, words=None, count=None, handle=None):
        self.ctx, self._lib = ctx, lib()
        if handle is None:
            n = int(count if words is None else words.shape[0])
            h = C.c_void_p()
            check(self._lib.jv_hip_bq_create(ctx._h, int(dimension), n, C.byref(h)))
            handle = h
        self._h = handle
        self.dimension = int(self._lib.jv_hip_bq_dimension(self._h))
        self._count = int(self._lib.jv_hip_bq_count(self._h))
        self.words = words_per_vector(self.dimension)
        if words is not None:
            self.upload(0, words)

    @classmethod
    def load(cls, ctx, data: bytes):
        """BQVectors.load: the reference's big-endian block (BinaryQuantization header, count, compressedLength, longs)"""
        buf = (C.c_ubyte * max(1, len(data))).from_buffer_copy(data or b"\0")
        h, consumed = C.c_void_p(), C.c_size_t()
        check(lib().jv_hip_bq_load(ctx._h, C.cast(buf, C.c_void_p), len(data), C.byref(consumed), C.byref(h)))
        self = cls(ctx, 0, handle=h)
        self.bytes_consumed = consumed.value
        return self

    def write(self) -> bytes:
        """BQVectors.write"""
        n = C.c_size_t()
        check(self._lib.jv_hip_bq_write(self.ctx._h, self._h, None, 0, C.byref(n)))
        buf = (C.c_ubyte * n.value)()
        check(self._lib.jv_hip_bq_write(self.ctx._h, self._h, C.cast(buf, C.c_void_p), n.value, C.byref(n)))
        return bytes(buf)

    def count(self):
        return self._count

    def upload(self, first, words):
        n = int(words.shape[0])
        if int(np.prod(words.shape)) != n * self.words:
            raise ValueError(f"BQ rows: expected {n} x {self.words} words")
        p, k = _u64(words)
        check(self._lib.jv_hip_bq_upload(self.ctx._h, self._h, int(first), n, p))

    def get(self, first=0, count=None):
        """rows [first, first + count) as (count, W) uint64 (BQVectors.get(i) for count = 1)"""
        count = self._count - first if count is None else int(count)
        out = np.empty((count, self.words), np.uint64)
        check(self._lib.jv_hip_bq_download(self.ctx._h, self._h, int(first), count, C.c_void_p(out.ctypes.data)))
        return out

    def score_function_for(self, queries, ordinals):
        """scoreFunctionFor(q).similarityTo(node) for ordinals[Q, B]: 1 - hamming(encode(q), row) / D"""
        Q, B = int(ordinals.shape[0]), int(ordinals.shape[1])
        q_p, qk = _ptr(queries, np.float32)
        o_p, ok = _ptr(ordinals, np.int32)
        out = np.empty((Q, B), np.float32) if not (_is_torch(ordinals)) else _like_f32((Q, B), ordinals)
        s_p, sk = _ptr(out, np.float32)
        check(self._lib.jv_hip_bq_scores(self.ctx._h, self._h, q_p, Q, o_p, B, s_p))
        return out

    def diversity_function_for(self, node1, node2):
        """diversityFunctionFor(node1[p]).similarityTo(node2[p, c])"""
        P, Cn = int(node2.shape[0]), int(node2.shape[1])
        a_p, ak = _ptr(node1, np.int32)
        b_p, bk = _ptr(node2, np.int32)
        out = np.empty((P, Cn), np.float32) if not (_is_torch(node2)) else _like_f32((P, Cn), node2)
        s_p, sk = _ptr(out, np.float32)
        check(self._lib.jv_hip_bq_pair_scores(self.ctx._h, self._h, a_p, P, b_p, Cn, s_p))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.jv_hip_bq_destroy(self._h)
            self._h = None


def _like_f32(shape, like):
    import torch
    return torch.empty(shape, dtype=torch.float32, device=like.device)


class BQFlatSearcher:
    """Flat search over BQVectors: the top rerankK rows by Hamming similarity (NodeQueue order, exact ties), reranked with the
    exact scores of `vectors` (jv_hip_search_flat's rerank), top-K.  vectors None or rerank_k 0: the BQ top-K."""

    def __init__(self, ctx, bq_vectors: BQVectors, vectors: VectorSet | None = None, id_base=0):
        self.ctx, self.bq, self.vectors, self.id_base = ctx, bq_vectors, vectors, int(id_base)

    def search(self, queries, vsf, top_k, rerank_k=0, accept=None, out_ids=None, out_scores=None):
        """accept: None, bool [count] shared by the batch, or bool [Q, count] per query — rows never returned"""
        from .engine import _empty
        Q = int(queries.shape[0])
        q_p, qk = _ptr(queries, np.float32)
        if out_ids is None:
            out_ids = _empty((Q, top_k), np.int32, queries)
        if out_scores is None:
            out_scores = _empty((Q, top_k), np.float32, queries)
        oi_p, oik = _ptr(out_ids, np.int32)
        os_p, osk = _ptr(out_scores, np.float32)
        mask_p, stride, mask = None, 0, None
        if accept is not None:
            mask = pack_accept_bits(accept, self.bq.count())
            if mask.ndim == 2:
                if mask.shape[0] != Q:
                    raise ValueError(f"accept has {mask.shape[0]} rows for {Q} queries")
                stride = int(mask.shape[1])
            mask_p = C.c_void_p(mask.ctypes.data)
        check(lib().jv_hip_bq_search_flat(self.ctx._h, self.bq._h, self.vectors._h if self.vectors is not None else None, q_p, Q,
                                          int(vsf), int(top_k), int(rerank_k), mask_p, stride, self.id_base, oi_p, os_p))
        return out_ids, out_scores
