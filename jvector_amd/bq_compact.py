"""Compacting a BQ graph under construction on the GPU (include/jvector_bq_compact.h): the sequential renumbering of the nodes in the
graph and a new builder holding the graph under it.  The signature table and its binding live here; the calls are methods of
bq_builder.BQGraphBuilder (renumbering, compact).  Thin ctypes, no arithmetic, no CPU fallback."""
from __future__ import annotations

import ctypes as C

from . import _lib

_p = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes); mirrors include/jvector_bq_compact.h one to one
BQ_COMPACT_SIGNATURES = {
    "jv_hip_bq_builder_renumbering": (_i, [_p, _p, _p, _p, C.POINTER(C.c_int64)]),
    "jv_hip_bq_builder_compact": (_i, [_p, _p, _p, _p, _p, C.POINTER(C.c_int64), C.POINTER(_p)]),
}


def lib():
    """the product library with BQ_COMPACT_SIGNATURES bound (once per loaded library)"""
    lb = _lib.load()
    if not getattr(lb, "_jv_bq_compact_bound", False):
        for name, (res, args) in BQ_COMPACT_SIGNATURES.items():
            fn = getattr(lb, name)   # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, args
        lb._jv_bq_compact_bound = True
    return lb
