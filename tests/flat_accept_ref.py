"""What jv_hip_search_flat_filtered must return, from the CPU oracle alone: OraclePQ.adc_scores -> mask -> topk -> compare_many -> topk.
Shared by tests/test_flat_filtered_cpu.py and tests/test_zz_flat_filtered_gpu.py.  No device, no product code."""
import numpy as np

from oracle import oracle as O


def problem(seed, N, D, M, Q):
    """the data of tests/test_zz_flat_bq_gpu.py: clustered unit vectors, every seventh vector twice (equal scores at every cut), a
    codebook of 256 of the vectors' own sub-vectors"""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((200, D)).astype(np.float32)
    vecs = (centers[rng.integers(0, 200, N)] + 0.35 * rng.standard_normal((N, D)).astype(np.float32)).astype(np.float32)
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    vecs[1::7] = vecs[0:-1:7][: len(vecs[1::7])]
    queries = (vecs[rng.integers(0, N, Q)] + 0.05 * rng.standard_normal((Q, D))).astype(np.float32)
    sizes, offs = O.subvector_sizes_offsets(D, M)
    pick = rng.choice(N, 256, replace=False)
    cb = np.concatenate([vecs[pick, offs[m]: offs[m] + sizes[m]].reshape(-1) for m in range(M)])
    return vecs, queries, cb


def pack(mask, junk=False, stride_words=None):
    """bool [N] or [Q, N] -> uint64 words; junk: every bit at and beyond N set (the tail of the last word, the slack words of a stride
    above ceil(N / 64))"""
    mask = np.asarray(mask, bool)
    n = mask.shape[-1]
    words = (n + 63) // 64
    width = 64 * (stride_words if stride_words else words)
    bits = np.full(mask.shape[:-1] + (width,), bool(junk))
    bits[..., :n] = mask
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little").view(np.uint64))


class Reference:
    """the oracle's answers over one problem; the approximate scores of a (query, vsf) are computed once and kept"""

    def __init__(self, opq, codes, vecs, queries):
        self.opq, self.codes, self.vecs, self.queries = opq, codes, vecs, queries
        self._approx = {}

    def approx(self, q, vsf):
        key = (q, int(vsf))
        if key not in self._approx:
            a = self.opq.adc_scores(self.queries[q], int(vsf), self.codes)
            a.setflags(write=False)
            self._approx[key] = a
        return self._approx[key]

    def search(self, vsf, top_k, rerank_k, accept, id_base=0, rerank=True, queries=None):
        """accept: bool [N] (shared) or [Q, N].  Returns (ids [Q, top_k], scores [Q, top_k]) with the (-1, -inf) tail."""
        qs = range(len(self.queries)) if queries is None else queries
        accept = np.asarray(accept, bool)
        ids = np.full((len(qs), top_k), -1, np.int32)
        sc = np.full((len(qs), top_k), -np.inf, np.float32)
        for r, q in enumerate(qs):
            rows = np.flatnonzero(accept if accept.ndim == 1 else accept[q]).astype(np.int32)
            if rows.size == 0:
                continue
            k1 = rerank_k if rerank and rerank_k > 0 else top_k
            cand, cs = O.topk(rows, self.approx(q, vsf)[rows], k1)
            if rerank and rerank_k > 0:
                cand, cs = O.topk(cand, O.compare_many(int(vsf), self.queries[q], self.vecs[cand]), top_k)
            ids[r, :len(cand)] = cand + id_base
            sc[r, :len(cand)] = cs
        return ids, sc
