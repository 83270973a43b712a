"""NVQ-score graph search on the MI355X (jv_hip_nvq_graph_search) next to the exact-score graph search on the same graph and beams:
recall@10 against VectorSet.search_exact ground truth, QPS, the traversal kernel's time from the engine's HIP events (region
"gsearch"), mean visited / expanded, and the bytes of rows the kernel fetches per second as a share of HBM peak (NVQ: D + 16 S bytes
per scored row, exact: 4 D; scored rows = visited + the entry node).  The two searchers alternate, ROUNDS times per beam after a
warm-up call each; every timing is given as [min, median, max] over the rounds.  Data: seeded benchlib.Mixture unit vectors; the
layered graph is built by jv_hip_build_layered; the rows are encoded by the device encoder.  Kernel names for a separate
`rocprofv3 --kernel-trace --stats` run: nvq_graph_search_kernel<VSF, SAFE>, exact_graph_search_kernel<VSF, TR, SAFE>.
One JSON object on stdout.
usage: python scripts/nvq_graph_bench.py [N=1000000] [D=128] [S=2]"""
import json
import os
import statistics
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
S = int(args[2]) if len(args) > 2 else 2
Q, K, DEGREE, M = 4096, 10, 32, D // 8
BEAMS = (50, 100, 200)
ROUNDS = 5
HBM_PEAK = 8.0e12   # bytes per second

T0 = time.perf_counter()
dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(Q, 3).contiguous()
vs = J.VectorSet(ctx, base)
out = {"n": N, "dim": D, "subvectors": S, "degree": DEGREE, "queries": Q, "rounds": ROUNDS, "hbm_peak_bytes_per_s": HBM_PEAK}


def log(msg):
    print(f"[nvq_graph_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def spread(xs):
    return [min(xs), statistics.median(xs), max(xs)]


cb = benchlib.train_codebooks(base, M, 5)
pq = J.ProductQuantization.from_codebooks(ctx, D, M, cb)
cv = J.PQVectors.encode_and_build(ctx, pq, vs)
t0 = time.perf_counter()
levels, entry, entry_level, nb0, bstats = build_hierarchical(ctx, pq, cv, base, VSF.DOT_PRODUCT, max_degree=DEGREE, vector_set=vs)
out["build_s"] = time.perf_counter() - t0
log(f"graph built in {out['build_s']:.1f}s")
graph = J.GraphIndex(ctx, N, levels, entry, entry_level)
gt = vs.search_exact(queries, VSF.DOT_PRODUCT, K, 4 * K)[0].cpu().numpy()
t0 = time.perf_counter()
nv = J.NVQuantization.compute(ctx, vs, S).encode_all(vs)
ctx.sync()
out["nvq_encode_s"] = time.perf_counter() - t0
log(f"NVQ rows encoded in {out['nvq_encode_s']:.1f}s")

sides = {"nvq_graph_search": (J.NVQGraphSearcher(ctx, graph, nv), "nvq_gs", D + 16 * S),
         "exact_graph_search": (J.ExactGraphSearcher(ctx, graph, vs), "exact_gs", 4 * D)}
for name in sides:
    out[name] = {}
for beam in BEAMS:
    acc = {name: {"call_ms": [], "kernel_ms": []} for name in sides}
    last = {}
    for name, (searcher, _, _) in sides.items():   # warm-up: code objects, workspaces, the NVQ tables
        searcher.search(queries, VSF.DOT_PRODUCT, K, beam)
    ctx.sync()
    for _ in range(ROUNDS):
        for name, (searcher, prefix, _) in sides.items():
            ctx.reset_stats()
            ctx.profile(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids, _, st = searcher.search(queries, VSF.DOT_PRODUCT, K, beam, return_stats=True)
            ctx.sync()
            acc[name]["call_ms"].append((time.perf_counter() - t0) * 1e3)
            acc[name]["kernel_ms"].append(ctx.profile_read("gsearch")[0])
            ctx.profile(False)
            last[name] = (ids, st, ctx.stat(prefix + "_queries_retried"), ctx.stat(prefix + "_last_workers"))
    for name, (_, _, row_bytes) in sides.items():
        ids, st, retried, workers = last[name]
        k_med = statistics.median(acc[name]["kernel_ms"])
        fetched = float(st[:, 0].sum() + Q) * row_bytes
        out[name][str(beam)] = {"recall_at_10": benchlib.recall_at_k(ids.cpu().numpy(), gt),
                                "qps": spread([Q / (ms * 1e-3) for ms in acc[name]["call_ms"]]),
                                "call_ms": spread(acc[name]["call_ms"]), "traversal_kernel_ms": spread(acc[name]["kernel_ms"]),
                                "mean_visited": float(st[:, 0].mean()), "mean_expanded": float(st[:, 1].mean()),
                                "row_bytes_per_query": fetched / Q, "share_of_hbm_peak": fetched / max(k_med * 1e-3, 1e-12) / HBM_PEAK,
                                "queries_retried": retried, "workers": workers}
        log(f"{name} beamK {beam}: " + json.dumps(out[name][str(beam)]))

print(json.dumps(out))
