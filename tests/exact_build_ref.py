"""The yardstick of the exact build-time scoring tests: VamanaDiversityProvider.retainDiverse / isDiverse
(B/graph/diversity/VamanaDiversityProvider.java:45-96) restated plainly and sequentially over pair scores from the CPU oracle
(jvo_compare's scalar order through oracle.compare_many, never from the engine): np.float32 for score * alpha, currentAlpha an f32
that grows by += 0.2f, the loop bound currentAlpha <= alpha + 1E-6 in double, the selected set walked in ascending position with the
`node == otherNode -> break` rule, and a strict >.  A pair with an ordinal outside the rows scores -inf (jv_hip_exact_pair_scores).
The node-seeded search is exact_graph_ref.search over the score matrix of the nodes' own rows."""
import numpy as np

from oracle import oracle as O


def clustered(seed, n, D, centres=20, spread=0.35):
    """n rows around `centres` cluster centres plus noise: on iid Gaussian rows every candidate is diverse and the prune tests nothing"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, D)).astype(np.float32)
    return (c[rng.integers(0, centres, n)] + spread * rng.standard_normal((n, D))).astype(np.float32)


class Pairs:
    """pair(i, j) = compare(v[nodes[i]], v[nodes[j]]) of one list, the first operand the candidate's; -inf where either ordinal names no
    row.  Entries are computed when first asked for (the oracle scores one pair per call) and kept: the list's prefixes share them."""

    def __init__(self, vsf, v, nodes):
        self.vsf, self.v, self.nodes = int(vsf), v, np.asarray(nodes, np.int64)
        ok = (self.nodes >= 0) & (self.nodes < len(v))
        self.M = np.full((len(self.nodes), len(self.nodes)), -np.inf, np.float32)
        self.known = ~(ok[:, None] & ok[None, :])

    def row(self, i, cols):
        miss = cols[~self.known[i, cols]]
        if len(miss):
            self.M[i, miss] = O.compare_many(self.vsf, self.v[self.nodes[i]], self.v[self.nodes[miss]])
            self.known[i, miss] = True
        return self.M[i, cols]


def top_lists(vsf, v, bases, C):
    """per base node the C other rows the oracle scores highest against it, descending (ties to the smaller id)"""
    nodes, scores = np.empty((len(bases), C), np.int32), np.empty((len(bases), C), np.float32)
    for p, b in enumerate(bases):
        s = np.asarray(O.compare_many(int(vsf), v[b], v), np.float32)
        s[b] = -np.inf
        order = np.lexsort((np.arange(len(v)), -s))[:C]
        nodes[p], scores[p] = order, s[order]
    return nodes, scores


def retain_diverse_one(pairs, nodes, scores, max_degree, alpha, diverse_before=0):
    """one NodeArray: (selected bool [n], nSelected, shortEdges f32, rejected in the first round?, first selected in a later round?)"""
    n = len(nodes)
    nodes = np.asarray(nodes, np.int64)
    scores = np.asarray(scores, np.float32)
    selected = np.zeros(n, bool)
    diverse_before = max(0, int(diverse_before))
    selected[:min(diverse_before, max_degree, n)] = True
    n_selected = diverse_before
    short_edges = np.float32(np.nan)
    current_alpha = np.float32(1.0)
    rejected_first = selected_later = False
    while float(current_alpha) <= float(np.float32(alpha)) + 1e-6 and n_selected < max_degree:
        for i in range(diverse_before, n):
            if n_selected >= max_degree:
                break
            if selected[i]:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                thr = np.float32(scores[i]) * current_alpha
            walk = np.flatnonzero(selected)
            own = np.flatnonzero(nodes[walk] == nodes[i])
            if len(own):
                walk = walk[:own[0]]
            if bool((pairs.row(i, walk) > thr).any()):
                rejected_first |= current_alpha == np.float32(1.0)
            else:
                selected[i] = True
                n_selected += 1
                selected_later |= current_alpha > np.float32(1.0)
        if current_alpha == np.float32(1.0):
            short_edges = np.float32(n_selected) / np.float32(max_degree)
        current_alpha = np.float32(current_alpha + np.float32(0.2))
    return selected, n_selected, short_edges, rejected_first, selected_later


def retain_diverse(pairs, cand_nodes, cand_scores, max_degree, alpha, cand_count=None, diverse_before=None):
    """the batch, pairs[p] = Pairs of node p's list: (selected [P, max_degree] ascending positions, -1 padded; n_selected [P] int32;
    short_edges [P] float32), and whether some node both rejected a candidate at alpha 1.0 and first selected one in a later round"""
    P, C = cand_nodes.shape
    sel = np.full((P, max_degree), -1, np.int32)
    cnt = np.zeros(P, np.int32)
    se = np.full(P, np.nan, np.float32)
    both = False
    for p in range(P):
        n = C if cand_count is None else min(max(int(cand_count[p]), 0), C)
        db = 0 if diverse_before is None else int(diverse_before[p])
        s, cnt[p], se[p], rej, later = retain_diverse_one(pairs[p], cand_nodes[p, :n], cand_scores[p, :n], max_degree, alpha, db)
        both |= rej and later
        pos = np.flatnonzero(s)[:max_degree]
        sel[p, :len(pos)] = pos
    return (sel, cnt, se), both

