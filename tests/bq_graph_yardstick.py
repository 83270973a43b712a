"""Shared by the BQ graph search tests: problems, and the yardstick — the oracle's own GraphSearcher restatement driven by a "sign"
quantizer so that it walks in BQ order exactly.

For dimension D the quantizer has sub-vectors of 8 dimensions (and one of D % 8), no centring, 256 centroids each; centroid c holds
+1 at position j if bit j of c is set, else -1.  Its codes are the first ceil(D / 8) bytes of a BQ row, and the oracle is given the
query's sign vector.  Every table entry and every ADC sum is then a small exact integer under all three similarity functions, and the
score is strictly decreasing in the Hamming distance — as 1 - (float) h / D is for D <= 16383 — so every comparison, every tie, the
ids, visitedCount and expandedCount coincide with the BQ search."""
import numpy as np

from oracle import oracle as O

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def np_encode(v, D):
    """BinaryQuantization.encodeTo: bit j of word i set iff v[64 i + j] > 0"""
    v = np.asarray(v, np.float32).reshape(-1, D)
    W = (D + 63) // 64
    bits = np.zeros((v.shape[0], W * 64), bool)
    with np.errstate(invalid="ignore"):
        bits[:, :D] = v > 0
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1, W).astype(np.uint64)


def np_hamming(q_words, rows):
    x = np.bitwise_xor(rows, q_words[None, :])
    return _POP8[x.view(np.uint8)].reshape(len(rows), 8 * rows.shape[1]).sum(axis=1)


def np_similarity(h, D):
    """BQVectors.similarityBetween in f32"""
    return np.float32(1) - np.float32(h).astype(np.float32) / np.float32(D)


def sign_pq(D):
    sizes = [8] * (D // 8) + ([D % 8] if D % 8 else [])
    c = np.arange(256)
    cbs = []
    for sz in sizes:
        cb = np.where((c[:, None] >> np.arange(sz)[None, :]) & 1, 1.0, -1.0).astype(np.float32)   # [256][sz], centroid-major
        cbs.append(cb.reshape(-1))
    return O.OraclePQ(D, len(sizes), np.concatenate(cbs), None, 256, sizes=np.array(sizes, np.int32))


def sign_codes(words, D):
    return np.ascontiguousarray(words.view(np.uint8).reshape(len(words), -1)[:, :(D + 7) // 8])


def sign_queries(q):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(q, np.float32) > 0, 1.0, -1.0).astype(np.float32)


def knn_rows(v, ids, degree, rng, random_edges=2, short_every=0):
    """rows of `degree` neighbours among ids (exact kNN by dot product, a few replaced by random members), packed and -1 padded"""
    sub = v[ids]
    n = len(ids)
    k = min(degree, n - 1)
    out = np.full((n, degree), -1, np.int32)
    if k <= 0:
        return out
    sim = sub @ sub.T
    np.fill_diagonal(sim, -np.inf)
    nn = np.argsort(-sim, axis=1, kind="stable")[:, :k]
    for i in range(n):
        row = list(nn[i])
        for _ in range(min(random_edges, k)):
            r = int(rng.integers(0, n))
            if r != i and r not in row:
                row[int(rng.integers(0, k))] = r
        if short_every and i % short_every == 0:
            row = row[:max(1, k // 2)]
        out[i, :len(row)] = ids[np.array(row, np.int64)]
    return out


def build_problem(seed, N, D, degree, levels, nq, dup=False):
    """vectors, levels [(ids | None, rows)], entry node, entry level, queries; upper level l holds ~N / 6^l nodes (nested)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, D)).astype(np.float32)
    if dup:   # duplicated rows: equal BQ words, nearly every comparison a tie
        v[N // 2:] = v[:N - N // 2]
    ids = np.arange(N, dtype=np.int32)
    lv = [(None, knn_rows(v, ids, degree, rng, short_every=7))]
    for l in range(1, levels):
        n = max(2, len(ids) // 6)
        ids = np.sort(rng.choice(ids, n, replace=False)).astype(np.int32)
        lv.append((ids, knn_rows(v, ids, min(degree, 16), rng)))
    entry = int(ids[rng.integers(0, len(ids))])
    q = rng.standard_normal((nq, D)).astype(np.float32)
    return v, lv, entry, levels - 1, q


class Yardstick:
    def __init__(self, v, lv, entry, entry_level, D):
        self.D = D
        self.words = np_encode(v, D)
        self.opq = sign_pq(D)
        self.codes = sign_codes(self.words, D)
        self.og = O.OracleGraph(len(v), lv, entry, entry_level)

    def approx(self, q, top_k, rerank_k, accept=None, vsf=O.EUCLIDEAN):
        """ids [Q, top_k] in NodeQueue order (-1 padded), BQ similarities (-inf padded), stats [Q, 2].  (Euclidean by default: its
        score 1 / (1 + 4 h) is positive like a BQ similarity; the dot-product score (1 + D - 2 h) / 2 turns negative beyond h = D / 2,
        and GraphSearcher keeps a negative score out of the results.)"""
        ids, _, st = self.og.search(self.opq, self.codes, None, sign_queries(q), vsf, top_k, rerank_k, accept=accept)
        qw = np_encode(q, self.D)
        sc = np.full(ids.shape, -np.inf, np.float32)
        for i in range(len(q)):
            m = ids[i] >= 0
            sc[i, m] = np_similarity(np_hamming(qw[i], self.words[ids[i, m]]), self.D)
        return ids, sc, st

    def reranked(self, q, v, vsf, top_k, rerank_k, accept=None):
        """the oracle's walk with top_k = rerank_k, then the exact rerank of its ids under vsf and the top K"""
        cand, _, st = self.approx(q, rerank_k, rerank_k, accept=accept)
        ids = np.full((len(q), top_k), -1, np.int32)
        sc = np.full((len(q), top_k), -np.inf, np.float32)
        for i in range(len(q)):
            c = cand[i][cand[i] >= 0]
            if len(c) == 0:
                continue
            k = min(top_k, len(c))
            wi, ws = O.rerank(q[i:i + 1], v[c][None, :, :], c[None, :], int(vsf), k)
            ids[i, :k], sc[i, :k] = wi[0], ws[0]
        return ids, sc, st
