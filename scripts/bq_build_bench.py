"""Build-time scoring over binary-quantized vectors on the MI355X (include/jvector_bq_build.h): the node-seeded search
(jv_hip_bq_graph_search_nodes) at Q = 4 096 and 65 536 with topK = 100, and the batched robust prune (jv_hip_bq_retain_diverse) at
P = 65 536, C = 200, maxDegree = 32, alpha = 1.2, timed with the engine's HIP events (regions "gsearch" and "prune"); beside the
prune, for context, jv_hip_retain_diverse with PQ-96 on the same candidate lists.  Data: seeded benchlib.Mixture unit vectors; the
graph is the layered one of jv_hip_build_layered (built with PQ, as today).  The candidate lists are the node-seeded search's own
results (topK = C, the node itself excluded): what a builder would hand to the prune.  One JSON object on stdout.
usage: python scripts/bq_build_bench.py [N=1000000] [D=768] [--no-pq]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import benchlib
import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd.builder import build_hierarchical

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 1_000_000
D = int(args[1]) if len(args) > 1 else 768
NO_PQ = "--no-pq" in sys.argv
Q_SIZES = (4096, 65536)
TOP_K, P, C_LIST, DEGREE, ALPHA, M = 100, 65536, 200, 32, 1.2, 96

T0 = time.perf_counter()
dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
vs = J.VectorSet(ctx, base)
out = {"n": N, "dim": D, "words_per_row": (D + 63) // 64, "degree": DEGREE}


def log(msg):
    print(f"[bq_build_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def event_ms(region, fn, reps):
    """mean engine event time of `region` per call, and the wall time per call"""
    fn()
    ctx.sync()
    ctx.profile(True)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) / reps
    ms, _ = ctx.profile_read(region)
    ctx.profile(False)
    return ms / reps, wall * 1e3, r


cb = benchlib.train_codebooks(base, M, 5)
pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
cv = J.PQVectors.encode_and_build(ctx, pq, vs)
t0 = time.perf_counter()
levels, entry, entry_level, nb0, bstats = build_hierarchical(ctx, pq, cv, base, VSF.DOT_PRODUCT, max_degree=DEGREE, vector_set=vs)
out["build_s"] = time.perf_counter() - t0
log(f"graph built: {bstats['levels']} nodes per level in {out['build_s']:.1f}s")
graph = J.GraphIndex(ctx, N, levels, entry, entry_level)
bv = J.BinaryQuantization(ctx, D).encode_all(vs)
scorer = J.BQBuildScorer(ctx, graph, bv)
rng = np.random.default_rng(7)

search = {}
for Q in Q_SIZES:
    nodes = torch.from_numpy(rng.integers(0, N, Q).astype(np.int32)).to(dev)
    ctx.reset_stats()
    ms, wall, (_, _, st) = event_ms("gsearch", lambda: scorer.search_nodes(nodes, TOP_K, exclude_self=True, return_stats=True), 3)
    search[str(Q)] = {"traversal_event_ms": ms, "call_ms": wall, "nodes_per_s": Q / (wall * 1e-3), "mean_visited": float(st[:, 0].mean()),
                      "mean_expanded": float(st[:, 1].mean()),
                      "queries_retried_share": ctx.stat("bq_gs_queries_retried") / max(1, ctx.stat("bq_gs_queries"))}
    log(f"search_nodes Q {Q}: " + json.dumps(search[str(Q)]))
out["search_nodes_top100"] = search

assert scorer.max_candidates(DEGREE) >= C_LIST
nodes = torch.from_numpy(rng.integers(0, N, P).astype(np.int32)).to(dev)
cand, cand_sc = scorer.search_nodes(nodes, C_LIST, exclude_self=True)
count = (cand >= 0).sum(dim=1).to(torch.int32).contiguous()
ms, wall, (sel, cnt, se) = event_ms("prune", lambda: scorer.retain_diverse(cand, cand_sc, DEGREE, ALPHA, cand_count=count), 3)
out["bq_retain_diverse"] = {"P": P, "C": C_LIST, "max_degree": DEGREE, "alpha": ALPHA, "prune_event_ms": ms, "call_ms": wall,
                            "nodes_per_s": P / (ms * 1e-3), "mean_selected": float(cnt.float().mean()), "mean_candidates": float(count.float().mean())}
log("bq retain_diverse: " + json.dumps(out["bq_retain_diverse"]))

if not NO_PQ:
    prov = J.PQBuildScoreProvider(ctx, cv, VSF.DOT_PRODUCT)
    pq_sc = prov.diversity_scores(nodes, cand)   # the same lists under the PQ score of their node; order kept
    ms, wall, (sel, cnt, se) = event_ms("prune", lambda: prov.retain_diverse(cand, pq_sc, DEGREE, ALPHA, cand_count=count), 3)
    out["pq96_retain_diverse"] = {"prune_event_ms": ms, "call_ms": wall, "nodes_per_s": P / (ms * 1e-3), "mean_selected": float(cnt.float().mean()),
                                  "note": "same candidate lists in BQ order, scored with the PQ diversity score: context, not a like-for-like prune"}
    log("pq retain_diverse: " + json.dumps(out["pq96_retain_diverse"]))

print(json.dumps(out))
