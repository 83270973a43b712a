"""Shared by the BQ deletion tests: the yardstick — a literal Python / numpy restatement of GraphIndexBuilder.removeDeletedNodes
(B/graph/GraphIndexBuilder.java:678-799), Neighbors.replaceDeletedNeighbors (B/graph/ConcurrentNeighborMap.java:225-239) and
NodeArray.merge / insertSorted (B/graph/NodeArray.java:63-143, 170-210, 308-317) under the rules of include/jvector_bq_delete.h — over
the arrays BQGraphBuilder.working_rows returns.  The prune is bq_build_yardstick.retain_diverse.

Where the reference leaves a choice open the rule is the header's: candidates are inserted in ascending id (rule 2), the fallback draws
come from splitmix64 seeded with seed + id x 0x9E3779B97F4A7C15 (rule 7), the new entry is the smallest live id (rule 8)."""
import numpy as np

from bq_build_yardstick import pair_similarity, retain_diverse

_MASK = (1 << 64) - 1


def _splitmix(st):
    st = (st + 0x9E3779B97F4A7C15) & _MASK
    z = st
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return st, z ^ (z >> 31)


class NodeArray:
    """nodes / scores in descending score order; the three operations removeDeletedNodes uses"""

    def __init__(self):
        self.nodes, self.scores = [], []

    def size(self):
        return len(self.nodes)

    def add_in_order(self, node, score):
        self.nodes.append(int(node))
        self.scores.append(np.float32(score))

    def insert_sorted(self, node, score):
        score = np.float32(score)
        start, end = 0, len(self.nodes) - 1          # descSortFindRightMostInsertionPoint
        while start <= end:
            mid = (start + end) // 2
            if self.scores[mid] < score:
                end = mid - 1
            else:
                start = mid + 1
        i = start - 1                                # duplicateExistsNear
        while i >= 0 and self.scores[i] == score:
            if self.nodes[i] == node:
                return -1
            i -= 1
        i = start
        while i < len(self.nodes) and self.scores[i] == score:
            if self.nodes[i] == node:
                return -1
            i += 1
        self.nodes.insert(start, int(node))
        self.scores.insert(start, score)
        return start


def merge(a1, a2):
    """NodeArray.merge, line for line"""
    merged = NodeArray()
    i = j = 0
    with_last = set()
    last = np.float32(np.nan)
    while i < a1.size() and j < a2.size():
        if a1.scores[i] < a2.scores[j]:
            if a2.scores[j] != last:
                with_last.clear()
                last = a2.scores[j]
            if a2.nodes[j] not in with_last:
                with_last.add(a2.nodes[j])
                merged.add_in_order(a2.nodes[j], a2.scores[j])
            j += 1
        elif a1.scores[i] > a2.scores[j]:
            if a1.scores[i] != last:
                with_last.clear()
                last = a1.scores[i]
            if a1.nodes[i] not in with_last:
                with_last.add(a1.nodes[i])
                merged.add_in_order(a1.nodes[i], a1.scores[i])
            i += 1
        else:
            if a1.scores[i] != last:
                with_last.clear()
                last = a1.scores[i]
            if a1.nodes[i] not in with_last:
                with_last.add(a1.nodes[i])
                merged.add_in_order(a1.nodes[i], a1.scores[i])
            if a2.nodes[j] not in with_last:
                with_last.add(a2.nodes[j])
                merged.add_in_order(a2.nodes[j], a2.scores[j])
            i += 1
            j += 1
    for a, k in ((a1, i), (a2, j)):
        if k < a.size():
            while k < a.size() and a.scores[k] == last:
                if a.nodes[k] not in with_last:
                    merged.add_in_order(a.nodes[k], a.scores[k])
                k += 1
            while k < a.size():
                merged.add_in_order(a.nodes[k], a.scores[k])
                k += 1
    return merged


def fallback_draws(node, n, max_degree, present, marked, seed):
    """rule 7: the ids the fallback takes for `node`, in draw order"""
    st = (seed + node * 0x9E3779B97F4A7C15) & _MASK
    got = []
    for _ in range(2 * max_degree):
        if len(got) >= max_degree:
            break
        st, z = _splitmix(st)
        r = z % n
        again = 0
        while again < 64 and marked[r]:
            st, z = _splitmix(st)
            r = z % n
            again += 1
        if marked[r] or r == node or not present[r] or r in got:
            continue
        got.append(int(r))
    return got


def merged_lists(words, D, ids, sc, present, marked, max_degree, seed=0):
    """per affected node (ascending): dict(node, list ids, list scores (f32), candidates, fallback) — the list the prune reads"""
    n = len(ids)
    out = []
    for i in range(n):
        if not present[i] or marked[i]:
            continue
        row = [(int(k), s) for k, s in zip(ids[i], sc[i]) if k >= 0]
        if not any(marked[k] for k, _ in row):
            continue
        new_edges = set()
        for j, _ in row:
            if marked[j]:
                for k in ids[j]:
                    if k >= 0 and k != i and not marked[k]:
                        new_edges.add(int(k))
        cand = NodeArray()
        order = sorted(new_edges)
        fallback = len(order) == 0
        if fallback:
            order = sorted(fallback_draws(i, n, max_degree, present, marked, seed))   # "they go through rules 2 - 5": ascending id
        if order:
            s = pair_similarity(words, D, i, np.asarray(order, np.int64))
            for k, x in zip(order, s):
                cand.insert_sorted(k, x)
        live = NodeArray()
        for k, s in row:
            if not marked[k]:
                live.add_in_order(k, s)
        m = merge(live, cand)
        out.append(dict(node=i, ids=np.asarray(m.nodes, np.int32), scores=np.asarray(m.scores, np.float32), candidates=cand.size(),
                        fallback=fallback))
    return out


def remove_deleted(words, D, ids, sc, db, present, marked, max_degree, alpha, seed=0, entry=-1):
    """removeDeletedNodes over copies of the working lists: (ids, sc, db, present, entry, info) with info = dict(counts4, max_len,
    max_node, fallback_nodes, affected)"""
    ids, sc, db, present = ids.copy(), sc.copy(), db.copy(), np.asarray(present, bool).copy()
    marked = np.asarray(marked, bool)
    R = ids.shape[1]
    lists = merged_lists(words, D, ids, sc, present, marked, max_degree, seed)
    for m in lists:
        L = max(1, len(m["ids"]))
        cn = np.full((1, L), -1, np.int32)
        cs = np.zeros((1, L), np.float32)
        cn[0, :len(m["ids"])], cs[0, :len(m["ids"])] = m["ids"], m["scores"]
        sel, _, _ = retain_diverse(words, D, cn, cs, max_degree, alpha, cand_count=np.array([len(m["ids"])], np.int32),
                                   diverse_before=np.zeros(1, np.int32))
        pos = sel[0][sel[0] >= 0]
        i = m["node"]
        ids[i], sc[i] = -1, 0.0
        ids[i, :len(pos)], sc[i, :len(pos)] = cn[0, pos], cs[0, pos]
        db[i] = len(pos)
    ids[marked], sc[marked], db[marked] = -1, 0.0, 0
    present[marked] = False
    if entry >= 0 and marked[entry]:
        live = np.flatnonzero(present)
        entry = int(live[0]) if len(live) else -1
    lens = [len(m["ids"]) for m in lists]
    info = dict(counts4=(int(marked.sum()), len(lists), int(sum(m["candidates"] for m in lists)), int(sum(m["fallback"] for m in lists))),
                max_len=max(lens) if lens else 0, max_node=lists[int(np.argmax(lens))]["node"] if lens else -1,
                fallback_nodes=[m["node"] for m in lists if m["fallback"]], affected=[m["node"] for m in lists])
    assert R >= max_degree
    return ids, sc, db, present, entry, info
