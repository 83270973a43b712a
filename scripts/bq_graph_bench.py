"""Graph search over binary-quantized vectors on the MI355X (jv_hip_bq_graph_search): QPS at several batch sizes, recall@10 and mean
visited / expanded at rerankK 100 and 1000, the traversal kernel's time from the engine's HIP events (region "gsearch") and the
algorithmic bytes per second it stands for (expansions x degree x 8 W) against HBM peak; next to it, on the same data and rerankK,
the BQ flat search (jv_hip_bq_search_flat) and the PQ-96 graph search (jv_hip_graph_search, FusedPQ) for context.  The data are
scripts/bq_bench.py's: seeded benchlib.Mixture unit vectors; the layered graph is built by jv_hip_build_layered (with PQ, as today)
and searched with BQ + exact rerank.  Exact ground truth from jv_hip_exact_scan_dense.  Kernel name for a separate
`rocprofv3 --kernel-trace --stats` run: bq_graph_search_kernel<WT, SAFE>.  One JSON object on stdout.
usage: python scripts/bq_graph_bench.py [N=10000000] [D=768] [--quick] [--no-pq] [--no-flat]"""
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
N = int(args[0]) if len(args) > 0 else 10_000_000
D = int(args[1]) if len(args) > 1 else 768
QUICK, NO_PQ, NO_FLAT = "--quick" in sys.argv, "--no-pq" in sys.argv, "--no-flat" in sys.argv
Q_SIZES = (1, 256, 4096, 131072) if not QUICK else (1, 256, 4096)
Q_GT = 1000 if not QUICK else 200
RERANKS = (100, 1000)
K, DEGREE, M = 10, 32, 96
HBM_PEAK = 8.0e12   # bytes per second

T0 = time.perf_counter()
dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(max(max(Q_SIZES), Q_GT), 3)
vs = J.VectorSet(ctx, base)
W = (D + 63) // 64
out = {"n": N, "dim": D, "words_per_row": W, "degree": DEGREE, "hbm_peak_bytes_per_s": HBM_PEAK}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    ctx.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, r


def log(msg):
    print(f"[bq_graph_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


cb = benchlib.train_codebooks(base, M, 5)
pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
cv = J.PQVectors.encode_and_build(ctx, pq, vs)
t0 = time.perf_counter()
levels, entry, entry_level, nb0, bstats = build_hierarchical(ctx, pq, cv, base, VSF.DOT_PRODUCT, max_degree=DEGREE, vector_set=vs)
out["build_s"] = time.perf_counter() - t0
out["levels"] = bstats["levels"]
log(f"graph built: {out['levels']} nodes per level in {out['build_s']:.1f}s")
graph = J.GraphIndex(ctx, N, levels, entry, entry_level)
bv = J.BinaryQuantization(ctx, D).encode_all(vs)
searcher = J.BQGraphSearcher(ctx, graph, bv, vs)

qg = queries[:Q_GT].contiguous()
gt = benchlib.ground_truth(J, ctx, vs, qg, VSF.DOT_PRODUCT, K, dense=True, q_group=1024).cpu().numpy()

by_rk = {}
for rk in RERANKS:
    ctx.reset_stats()
    wall, (ids, _, st) = timed(lambda: searcher.search(qg, VSF.DOT_PRODUCT, K, rk, return_stats=True), 2)
    entry_rk = {"recall_at_10": benchlib.recall_at_k(host(ids), gt), "qps_at_%d" % Q_GT: Q_GT / wall,
                "mean_visited": float(st[:, 0].mean()), "mean_expanded": float(st[:, 1].mean()),
                "queries_retried_share": ctx.stat("bq_gs_queries_retried") / max(1, ctx.stat("bq_gs_queries")),
                "visited_table_log2": ctx.stat("bq_gs_last_vcap_log2"), "workers": ctx.stat("bq_gs_last_workers")}
    sizes = {}
    for Q in Q_SIZES:
        qs = queries[:Q].contiguous()
        reps = 5 if Q <= 4096 else 2
        timed(lambda: searcher.search(qs, VSF.DOT_PRODUCT, K, rk), 1)
        ctx.profile(True)
        wall, (_, _, st) = timed(lambda: searcher.search(qs, VSF.DOT_PRODUCT, K, rk, return_stats=True), reps)
        gs_ms, gs_n = ctx.profile_read("gsearch")
        ctx.profile(False)
        calls = reps + 1
        kernel_ms = gs_ms / max(1, calls)   # first attempt + (if any) the roomy pass, per call
        algo_bytes = float(st[:, 1].sum()) * DEGREE * 8 * W
        log(f"rerankK {rk} Q {Q}: {Q / wall:.0f} QPS, kernel {kernel_ms:.2f} ms")
        sizes[str(Q)] = {"qps": Q / wall, "call_ms": wall * 1e3, "traversal_kernel_ms": kernel_ms,
                         "algorithmic_bytes_per_s": algo_bytes / max(kernel_ms * 1e-3, 1e-12),
                         "share_of_hbm_peak": algo_bytes / max(kernel_ms * 1e-3, 1e-12) / HBM_PEAK}
    entry_rk["by_batch"] = sizes
    log(f"rerankK {rk}: " + json.dumps(entry_rk))
    by_rk[str(rk)] = entry_rk
out["bq_graph_search"] = {"queries_for_recall": Q_GT, "by_rerank_k": by_rk}

if not NO_FLAT:
    flat = J.BQFlatSearcher(ctx, bv, vs)
    fr = {}
    for rk in RERANKS:
        wall, (ids, _) = timed(lambda: flat.search(qg, VSF.DOT_PRODUCT, K, rk), 2)
        fr[str(rk)] = {"recall_at_10": benchlib.recall_at_k(host(ids), gt), "qps": Q_GT / wall}
    out["bq_search_flat"] = {"queries": Q_GT, "by_rerank_k": fr}
    log("flat: " + json.dumps(fr))

if not NO_PQ:
    fused = J.FusedPQ.build(ctx, cv, nb0)
    gs = J.GraphSearcher(ctx, graph, pq, cv, fused, vs, max_queries=max(Q_GT, 4096))
    pr = {}
    for rk in RERANKS:
        wall, (ids, _, st) = timed(lambda: gs.search(qg, VSF.DOT_PRODUCT, K, rk, return_stats=True), 2)
        q4 = queries[:4096].contiguous()
        wall4, _ = timed(lambda: gs.search(q4, VSF.DOT_PRODUCT, K, rk), 2)
        pr[str(rk)] = {"recall_at_10": benchlib.recall_at_k(host(ids), gt), "qps_at_%d" % Q_GT: Q_GT / wall, "qps_at_4096": 4096 / wall4,
                       "mean_visited": float(st[:, 0].mean()), "mean_expanded": float(st[:, 1].mean())}
    out["pq96_graph_search"] = {"queries": Q_GT, "by_rerank_k": pr}

print(json.dumps(out))
