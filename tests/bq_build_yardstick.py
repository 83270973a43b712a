"""Shared by the BQ build-time scoring tests: the yardstick of the batched robust prune over BQ rows and the generator of its
candidate lists.

The yardstick restates VamanaDiversityProvider.retainDiverse / isDiverse (B/graph/diversity/VamanaDiversityProvider.java:45-96)
with the diversity score of BuildScoreProvider.bqBuildScoreProvider, BQVectors.similarityBetween(row(a), row(b)) =
1 - (float) hamming / D, in numpy: np.float32 arithmetic for the similarity and for score * alpha, currentAlpha an f32 that grows
by += 0.2f, the loop bound currentAlpha <= alpha + 1E-6 in double, the selected set walked in ascending position with the
`node == otherNode -> break` rule, and a strict >.  A pair with an ordinal outside the rows has similarity -inf
(jv_hip_bq_pair_scores).  BQ words come from bq_graph_yardstick.np_encode.

For the node-seeded search the yardstick is bq_graph_yardstick.Yardstick.approx(v[nodes], k, k, accept=...): the sign vector of
v[n] is row n, and exclude_self is a [Q, N] accept mask with bit nodes[q] cleared (self_mask)."""
import numpy as np

from bq_graph_yardstick import np_similarity

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def pair_similarity(words, D, a, b):
    """similarityBetween(row a, rows b) in f32; -inf where an ordinal lies outside the rows"""
    b = np.asarray(b, np.int64)
    out = np.full(len(b), -np.inf, np.float32)
    ok = (b >= 0) & (b < len(words))
    if 0 <= a < len(words) and ok.any():
        x = np.bitwise_xor(words[b[ok]], words[a][None, :])
        h = _POP8[x.view(np.uint8)].reshape(len(x), -1).sum(axis=1)
        out[ok] = np_similarity(h, D)
    return out


def retain_diverse_one(words, D, nodes, scores, max_degree, alpha, diverse_before=0):
    """one NodeArray: (selected bool [n], nSelected, shortEdges f32)"""
    n = len(nodes)
    nodes_a = np.asarray(nodes, np.int64)
    nodes = [int(x) for x in nodes]
    scores = np.asarray(scores, np.float32)
    selected = np.zeros(n, bool)
    diverse_before = max(0, int(diverse_before))
    selected[:min(diverse_before, max_degree, n)] = True
    n_selected = diverse_before
    short_edges = np.float32(np.nan)
    current_alpha = np.float32(1.0)
    sims = {}   # candidate position -> its similarity to every candidate position (alpha-independent)
    while float(current_alpha) <= float(np.float32(alpha)) + 1e-6 and n_selected < max_degree:
        for i in range(diverse_before, n):
            if n_selected >= max_degree:
                break
            if selected[i]:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                thr = np.float32(scores[i]) * current_alpha
            # isDiverse: the selected positions in ascending order up to the first one that holds the candidate's own id (break);
            # any of them more similar to the candidate than score * alpha -> not diverse
            walk = np.flatnonzero(selected)
            own = np.flatnonzero(nodes_a[walk] == nodes[i])
            if len(own):
                walk = walk[:own[0]]
            diverse = True
            if len(walk):
                if i not in sims:
                    sims[i] = pair_similarity(words, D, nodes[i], nodes_a)
                diverse = not bool((sims[i][walk] > thr).any())
            if diverse:
                selected[i] = True
                n_selected += 1
        if current_alpha == np.float32(1.0):
            short_edges = np.float32(n_selected) / np.float32(max_degree)
        current_alpha = np.float32(current_alpha + np.float32(0.2))
    return selected, n_selected, short_edges


def retain_diverse(words, D, cand_nodes, cand_scores, max_degree, alpha, cand_count=None, diverse_before=None):
    """the batch: (selected [P, max_degree] ascending positions, -1 padded; n_selected [P] int32; short_edges [P] float32)"""
    P, C = cand_nodes.shape
    sel = np.full((P, max_degree), -1, np.int32)
    cnt = np.zeros(P, np.int32)
    se = np.full(P, np.nan, np.float32)
    for p in range(P):
        n = C if cand_count is None else min(max(int(cand_count[p]), 0), C)
        db = 0 if diverse_before is None else int(diverse_before[p])
        s, cnt[p], se[p] = retain_diverse_one(words, D, cand_nodes[p, :n], cand_scores[p, :n], max_degree, alpha, db)
        pos = np.flatnonzero(s)[:max_degree]
        sel[p, :len(pos)] = pos
    return sel, cnt, se


def candidate_lists(words, D, P, C, seed):
    """C distinct random ordinals per node, scored against a random base row with the BQ similarity, sorted by score descending
    (ties to the smaller id): cand_nodes [P, C] int32, cand_scores [P, C] float32"""
    rng = np.random.default_rng(seed)
    N = len(words)
    nodes = np.empty((P, C), np.int32)
    scores = np.empty((P, C), np.float32)
    for p in range(P):
        base = int(rng.integers(0, N))
        ids = rng.choice(N, C, replace=False).astype(np.int32)
        sc = pair_similarity(words, D, base, ids)
        order = np.lexsort((ids, -sc))
        nodes[p], scores[p] = ids[order], sc[order]
    return nodes, scores


def self_mask(nodes, n_nodes):
    """[Q, n_nodes] accept mask with bit nodes[q] cleared"""
    acc = np.ones((len(nodes), n_nodes), bool)
    acc[np.arange(len(nodes)), np.asarray(nodes, np.int64)] = False
    return acc


def same(got, want):
    """np.array_equal over tuples, NaN equal to NaN"""
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f")
