"""Exact build-time scoring on the MI355X (jv_hip_exact_retain_diverse / jv_hip_exact_graph_search_nodes through ExactBuildScorer)
against the plain sequential yardsticks of exact_build_ref.py and exact_graph_ref.py — the CPU oracle's scalar scores, a restatement
of retainDiverse and of GraphSearcher — with no tolerance: positions, n_selected, short_edges (NaN equal to NaN), ids, score bits and
both counters are compared with np.array_equal.  N = 2000 clustered rows, P = 37 nodes, a node's list = the rows the oracle scores
highest against it.  (A node that its own search reaches comes back first under L2 and cosine; under dot product a longer row of the
same direction outscores a row's own copy.  With exclude_self the counters are compared with the yardstick's masked walk.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd import exact_build as XB
from bq_build_yardstick import same
from bq_graph_yardstick import knn_rows
from oracle import oracle as O
import exact_build_ref as R
import exact_graph_ref as G

N, P, CMAX = 2000, 37, 200
ALL_VSF = [VSF.DOT_PRODUCT, VSF.EUCLIDEAN, VSF.COSINE]
EDGE_D = {int(VSF.DOT_PRODUCT): 10, int(VSF.EUCLIDEAN): 13, int(VSF.COSINE): 72}   # rows not 16-byte aligned, and aligned


@pytest.fixture(scope="module")
def ctx():
    c = J.HipContext(0)
    yield c
    c.close()


class Data:
    def __init__(self, ctx, D, dup):
        self.v = R.clustered(500 + D, N, D)
        if dup:   # every row twice: row b + N / 2 is row b
            self.v[N // 2:] = self.v[:N // 2]
        self.vs = J.VectorSet(ctx, self.v)
        self.bases = np.random.default_rng(7).choice(N // 2, P, replace=False).astype(np.int32)
        self._lists, self._graph = {}, None

    def graph(self, ctx):
        if self._graph is None:
            rng, ids = np.random.default_rng(3), np.arange(N, dtype=np.int32)
            lv = [(None, knn_rows(self.v, ids, 16, rng, short_every=7))]
            for _ in range(2):
                ids = np.sort(rng.choice(ids, len(ids) // 6, replace=False)).astype(np.int32)
                lv.append((ids, knn_rows(self.v, ids, 16, rng)))
            entry = int(ids[rng.integers(0, len(ids))])
            nodes = rng.choice(N, 33, replace=False).astype(np.int32)
            nodes[5] = nodes[2]   # (one ordinal twice)
            self._graph = (lv, entry, J.GraphIndex(ctx, N, lv, entry, 2), nodes, {})
        return self._graph

    def lists(self, vsf, C=CMAX):
        if int(vsf) not in self._lists:
            nodes, scores = R.top_lists(vsf, self.v, self.bases, CMAX)
            self._lists[int(vsf)] = (nodes, scores, [R.Pairs(vsf, self.v, nodes[p]) for p in range(P)])
        nodes, scores, pairs = self._lists[int(vsf)]
        return np.ascontiguousarray(nodes[:, :C]), np.ascontiguousarray(scores[:, :C]), pairs


@pytest.fixture(scope="module")
def data(ctx):
    cache = {}

    def get(D, dup=False):
        if (D, dup) not in cache:
            cache[(D, dup)] = Data(ctx, D, dup)
        return cache[(D, dup)]
    return get


@pytest.mark.parametrize("C", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("D", [8, 20, 100, 128, 776])
@pytest.mark.parametrize("vsf", ALL_VSF)
def test_prune_parity(ctx, data, vsf, D, C):
    d = data(D)
    nodes, scores, pairs = d.lists(vsf, C)
    scorer = J.ExactBuildScorer(ctx, None, d.vs, vsf)
    ctx.reset_stats()
    calls = 0
    for md in (1, 8, 32, 64):
        for alpha in (1.0, 1.2, 1.4):
            want, both = R.retain_diverse(pairs, nodes, scores, md, alpha)
            if alpha == 1.4 and C >= 63 and 8 <= md < C:   # the condition on the data: the prune rejects, and later rounds select
                assert both
            same(scorer.retain_diverse(nodes, scores, md, alpha), want)
            calls += 1
    assert ctx.stat("exact_retain_calls") == calls and ctx.stat("exact_retain_nodes") == calls * P


def _own_id(d, vsf, a):
    # positions 2, 40 and 60 name one ordinal; 40 is always diverse (round 1), 2 is rejected by position 0 at alpha 1.0 and may pass later
    for p in range(P):
        x = a["nodes"][p, 40]
        a["nodes"][p, [2, 60]] = x
        a["scores"][p, [2, 60]] = np.float32(O.compare_many(int(vsf), d.v[x], d.v[a["nodes"][p, :1]])[0]) / np.float32(1.1)
        a["scores"][p, 40] = 10.0


def _equal_to_threshold(d, vsf, a):
    # position 0 is the twin of the base row: pair(cand, twin) has the bits of cand's own score, and at alpha 1.0 only > rejects
    a["nodes"][:, 0] = d.bases + N // 2
    a["scores"][:, 0] = [O.compare_many(int(vsf), d.v[b], d.v[b:b + 1])[0] for b in d.bases]


def _non_finite(d, vsf, a):
    a["scores"][:] = np.random.default_rng(3).permuted(a["scores"], axis=1)
    a["scores"][:, 5::11] = np.array([np.inf, -np.inf, np.nan, 0.0, -1.0, np.inf], np.float32)[:a["scores"][:, 5::11].shape[1]]


EDGES = {
    "own_id": (_own_id, False, {}),
    "equal_to_threshold": (_equal_to_threshold, True, {}),
    "diverse_before": (lambda d, vsf, a: None, False, {"diverse_before": np.array([0, 3, 32, 37] * 10, np.int32)[:P]}),
    "cand_count": (lambda d, vsf, a: None, False, {"cand_count": np.array([0, 1, 70] * 13, np.int32)[:P]}),
    "ordinals_outside": (lambda d, vsf, a: a["nodes"].__setitem__((slice(None), [3, 7, 66]), [-1, N, -1]), False, {}),
    "no_round_0.9": (lambda d, vsf, a: None, False, {"alpha": 0.9, "diverse_before": np.full(P, 2, np.int32)}),
    "no_round_nan": (lambda d, vsf, a: None, False, {"alpha": float("nan")}),
    "non_finite_unsorted": (_non_finite, False, {}),
    "on_device": (lambda d, vsf, a: None, False, {"cand_count": np.array([70, 69, 5] * 13, np.int32)[:P], "diverse_before": np.array([1, 0] * 19, np.int32)[:P]}),
}


@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("vsf", ALL_VSF)
def test_prune_edges(ctx, data, vsf, edge):
    edit, dup, kw = EDGES[edge]
    d = data(EDGE_D[int(vsf)], dup)
    nodes, scores, _ = d.lists(vsf, 70)
    kw = dict(kw)
    alpha = kw.pop("alpha", 1.4)
    a = {"nodes": nodes, "scores": scores, **kw}
    host = dict(a)
    edit(d, vsf, a)   # (in place: `host` sees it)
    if edge == "on_device":
        a = {k: __import__("torch").from_numpy(x).cuda() for k, x in a.items()}
    pairs = [R.Pairs(vsf, d.v, host["nodes"][p]) for p in range(P)]
    want, _ = R.retain_diverse(pairs, host["nodes"], host["scores"], 32, alpha, host.get("cand_count"), host.get("diverse_before"))
    got = J.ExactBuildScorer(ctx, None, d.vs, vsf).retain_diverse(a["nodes"], a["scores"], 32, alpha, a.get("cand_count"), a.get("diverse_before"))
    if edge == "on_device":
        assert all(g.is_cuda for g in got)
        got = [g.cpu().numpy() for g in got]
    same(got, want)
    if edge.startswith("no_round"):
        assert np.isnan(want[2]).all()
    if edge == "own_id":   # some node selects position 2 in a later round than position 40, which holds the same ordinal
        first = R.retain_diverse(pairs, host["nodes"], host["scores"], 32, 1.0)[0][0]
        assert any(40 in first[p] and 2 not in first[p] and 2 in want[0][p] for p in range(P))


def test_prune_refusals(ctx, data):
    d = data(128)
    nodes, scores, _ = d.lists(VSF.EUCLIDEAN, 64)
    scorer = J.ExactBuildScorer(ctx, None, d.vs, VSF.EUCLIDEAN)
    cmax, lib, vp = scorer.max_candidates(64), XB.lib(), lambda x: C.c_void_p(x.ctypes.data)
    assert cmax >= 256 and scorer.max_candidates(65) == 0
    sel, cnt, se = np.full((P, 65), 77, np.int32), np.full(P, 77, np.int32), np.full(P, 77, np.float32)
    wide = np.zeros((1, cmax + 1), np.int32)
    nvq = J.NVQuantization.compute(ctx, d.vs, 2).encode_all(d.vs).as_vector_set()

    def call(vh=d.vs._h, n=P, c=64, nd=nodes, sc=scores, md=32, alpha=1.2):
        return lib.jv_hip_exact_retain_diverse(ctx._h, vh, int(VSF.EUCLIDEAN), n, c, vp(nd), vp(sc), None, None, md, alpha, vp(sel), vp(cnt), vp(se))

    INVALID, UNSUPPORTED = J._lib.JV_ERR_INVALID, J._lib.JV_ERR_UNSUPPORTED
    assert call(alpha=65.0) == INVALID and call(md=0) == INVALID and call(c=0) == INVALID and call(n=-1) == INVALID and call(vh=None) == INVALID
    assert call(md=65) == UNSUPPORTED and call(vh=nvq._h) == UNSUPPORTED
    assert call(n=1, c=cmax + 1, nd=wide, sc=wide.astype(np.float32), md=64) == UNSUPPORTED
    assert (sel == 77).all() and (cnt == 77).all() and (se == 77).all()   # a refused call leaves the outputs untouched
    assert call(n=0) == 0 and (sel == 77).all() and call() == 0 and (cnt != 77).all()


@pytest.mark.parametrize("k,beam", [(1, 0), (10, 50)])
@pytest.mark.parametrize("vsf", ALL_VSF)
@pytest.mark.parametrize("D", [20, 128])
def test_search_nodes(ctx, data, D, vsf, k, beam):
    d = data(D)
    lv, entry, graph, nodes, S = d.graph(ctx)
    if int(vsf) not in S:
        S[int(vsf)] = G.score_matrix(vsf, d.v[nodes], d.v)
    scorer = J.ExactBuildScorer(ctx, graph, d.vs, vsf)
    mask = np.ones((len(nodes), N), bool)
    mask[np.arange(len(nodes)), nodes] = False
    ctx.reset_stats()
    plain = scorer.search_nodes(nodes, k, beam, return_stats=True)
    same(plain, G.search(S[int(vsf)], lv, entry, 2, k, beam))
    assert ctx.stat("exact_gs_calls") == 1 and ctx.stat("exact_gs_queries") == len(nodes)
    found = (plain[0] == nodes[:, None]).any(axis=1)   # (a beam of one does not reach every node of an approximate graph)
    assert found.any() and (vsf == VSF.DOT_PRODUCT or np.array_equal(plain[0][found, 0], nodes[found]))
    excl = scorer.search_nodes(nodes, k, beam, exclude_self=True, return_stats=True)
    same(excl, G.search(S[int(vsf)], lv, entry, 2, k, beam, mask))
    assert not (excl[0] == nodes[:, None]).any()
    bad = np.where(np.arange(len(nodes)) == 4, N + 5, nodes).astype(np.int32)   # device ordinals are not looked at: item 4 comes back blank
    ids, sc, st = scorer.search_nodes(__import__("torch").from_numpy(bad).cuda(), k, beam, exclude_self=True, return_stats=True)
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    assert (ids[4] == -1).all() and np.isneginf(sc[4]).all() and (st[4] == 0).all()
    keep = np.arange(len(nodes)) != 4
    same((ids[keep], sc[keep], st[keep]), [x[keep] for x in excl])
    with pytest.raises(ValueError):
        scorer.search_nodes(bad, k, beam)
