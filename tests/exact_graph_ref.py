"""The yardstick of the exact-score graph search tests: GraphSearcher.search with an exact score function, restated plainly and
sequentially.  The Q x N score matrix comes from the CPU oracle (jvo_compare's scalar order, never from the engine); the walk is
searchOneLayer, the layer hand-over and NodeQueue order by table lookup (B/graph/GraphSearcher.java:263-282, 324-369, 406-457, 515-530)."""
import heapq

import numpy as np

from oracle import oracle as O


def score_matrix(vsf, q, v):
    return np.stack([O.compare_many(int(vsf), q[i], v) for i in range(len(q))]).astype(np.float32)


def nodequeue_keys(scores):
    """NodeQueue.encode for nodes 0 .. n - 1: floatToSortableInt(score) << 32 | ~node, a signed 64-bit order"""
    bits = np.ascontiguousarray(scores, np.float32).view(np.int32)
    sortable = (bits ^ ((bits >> 31) & 0x7FFFFFFF)).astype(np.int64)
    return (sortable << 32) | (~np.arange(len(scores), dtype=np.int64) & 0xFFFFFFFF)


def walk(s, levels, entry, entry_level, top_k, beam_k, accept=None):
    """one query: s = its N scores.  Returns ids [top_k], scores [top_k], (visitedCount, expandedCount)"""
    keys = nodequeue_keys(s).tolist()
    rows = [lv[1] if lv[0] is None else {int(n): lv[1][i] for i, n in enumerate(lv[0])} for lv in levels]
    visited, cand, evicted, res = {entry}, [(-keys[entry], entry)], [], []
    n_visited = n_expanded = 0
    for lvl in range(entry_level, -1, -1):
        rk = 1 if lvl > 0 else beam_k
        res = []   # min-heap: res[0] is the worst kept
        while cand:
            top = cand[0][1]
            if len(res) >= rk and s[top] < s[res[0][1]]:   # stopSearch: strict <
                break
            heapq.heappop(cand)
            if (lvl > 0 or accept is None or accept[top]) and s[top] >= np.float32(0):   # threshold 0: a negative score is not kept
                if len(res) < rk:
                    heapq.heappush(res, (keys[top], top))
                elif s[top] > s[res[0][1]]:
                    evicted.append(heapq.heapreplace(res, (keys[top], top))[1])
            n_expanded += 1
            row = rows[lvl][top] if lvl == 0 or top in rows[lvl] else ()
            for nb in row:
                nb = int(nb)
                if nb < 0:
                    break
                if nb not in visited:
                    visited.add(nb)
                    n_visited += 1
                    heapq.heappush(cand, (-keys[nb], nb))
        if lvl > 0:   # setEntryPointsFromPreviousLayer
            for n in [n for _, n in res] + evicted:
                heapq.heappush(cand, (-keys[n], n))
        evicted = []
    best = [n for _, n in sorted(res, reverse=True)[:top_k]]
    ids = np.full(top_k, -1, np.int32)
    sc = np.full(top_k, -np.inf, np.float32)
    ids[:len(best)], sc[:len(best)] = best, s[best]
    return ids, sc, (n_visited, n_expanded)


def search(S, levels, entry, entry_level, top_k, beam_k, accept=None):
    """every query of the score matrix S; accept: None, bool [N] or bool [Q, N].  Returns ids, scores, stats [Q, 2]"""
    out = [walk(S[i], levels, entry, entry_level, top_k, beam_k or top_k,
                None if accept is None else (accept if accept.ndim == 1 else accept[i])) for i in range(len(S))]
    return (np.stack([o[0] for o in out]).reshape(len(S), top_k), np.stack([o[1] for o in out]).reshape(len(S), top_k),
            np.array([o[2] for o in out], np.int64).reshape(len(S), 2))
