"""Exact-score graph search on the MI355X (jv_hip_exact_graph_search): QPS, recall@10 against VectorSet.search_exact ground truth and
mean visited / expanded at several beamK, the traversal kernel's time from the engine's HIP events (region "gsearch") and the share of
HBM peak it stands for, taking 4 D bytes per scored row (visited + the entry node); next to it, on the same graph, the PQ + rerank
graph search (jv_hip_graph_search, FusedPQ, M = D / 8) at several rerankK, so that the two can be read at equal recall.  Data: seeded
benchlib.Mixture unit vectors; the layered graph is built by jv_hip_build_layered.  Kernel name for a separate
`rocprofv3 --kernel-trace --stats` run: exact_graph_search_kernel<VSF, TR, SAFE>.  One JSON object on stdout.
usage: python scripts/exact_graph_bench.py [N=1000000] [D=128] [--no-pq]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import benchlib
import jvector_amd as J
from jvector_amd import VectorSimilarityFunction as VSF
from jvector_amd.builder import build_hierarchical

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 1_000_000
D = int(args[1]) if len(args) > 1 else 128
NO_PQ = "--no-pq" in sys.argv
Q, K, DEGREE, M = 4096, 10, 32, D // 8
BEAMS = (10, 50, 100, 200)
HBM_PEAK = 8.0e12   # bytes per second

T0 = time.perf_counter()
dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(Q, 3).contiguous()
vs = J.VectorSet(ctx, base)
out = {"n": N, "dim": D, "degree": DEGREE, "queries": Q, "hbm_peak_bytes_per_s": HBM_PEAK}


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
    print(f"[exact_graph_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


cb = benchlib.train_codebooks(base, M, 5)
pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
cv = J.PQVectors.encode_and_build(ctx, pq, vs)
t0 = time.perf_counter()
levels, entry, entry_level, nb0, bstats = build_hierarchical(ctx, pq, cv, base, VSF.DOT_PRODUCT, max_degree=DEGREE, vector_set=vs)
out["build_s"] = time.perf_counter() - t0
log(f"graph built in {out['build_s']:.1f}s")
graph = J.GraphIndex(ctx, N, levels, entry, entry_level)
gt = vs.search_exact(queries, VSF.DOT_PRODUCT, K, 4 * K)[0].cpu().numpy()

searcher = J.ExactGraphSearcher(ctx, graph, vs)
REPS = 5
by_beam = {}
for beam in BEAMS:
    ctx.reset_stats()
    timed(lambda: searcher.search(queries, VSF.DOT_PRODUCT, K, beam), 1)
    ctx.profile(True)
    wall, (ids, _, st) = timed(lambda: searcher.search(queries, VSF.DOT_PRODUCT, K, beam, return_stats=True), REPS)
    gs_ms, _ = ctx.profile_read("gsearch")
    ctx.profile(False)
    kernel_ms = gs_ms / (REPS + 1)
    row_bytes = float(st[:, 0].sum() + Q) * 4 * D
    by_beam[str(beam)] = {"recall_at_10": benchlib.recall_at_k(ids.cpu().numpy(), gt), "qps": Q / wall, "call_ms": wall * 1e3,
                          "traversal_kernel_ms": kernel_ms, "mean_visited": float(st[:, 0].mean()), "mean_expanded": float(st[:, 1].mean()),
                          "share_of_hbm_peak": row_bytes / max(kernel_ms * 1e-3, 1e-12) / HBM_PEAK,
                          "queries_retried": ctx.stat("exact_gs_queries_retried"), "workers": ctx.stat("exact_gs_last_workers")}
    log(f"beamK {beam}: " + json.dumps(by_beam[str(beam)]))
out["exact_graph_search"] = by_beam

if not NO_PQ:
    fused = J.FusedPQ.build(ctx, cv, nb0)
    gs = J.GraphSearcher(ctx, graph, pq, cv, fused, vs, max_queries=Q)
    pr = {}
    for rk in BEAMS:
        wall, (ids, _, st) = timed(lambda: gs.search(queries, VSF.DOT_PRODUCT, K, rk, return_stats=True), REPS)
        pr[str(rk)] = {"recall_at_10": benchlib.recall_at_k(ids.cpu().numpy(), gt), "qps": Q / wall, "mean_visited": float(st[:, 0].mean())}
        log(f"pq rerankK {rk}: " + json.dumps(pr[str(rk)]))
    out["pq_graph_search"] = pr

print(json.dumps(out))
