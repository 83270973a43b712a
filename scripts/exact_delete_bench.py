"""Deleting from an exact-score builder graph next to the only alternative there was, building the survivors' graph again, on the
MI355X: N unit rows (seeded benchlib.Mixture) are built with ExactGraphBuilder under DOT_PRODUCT, a seeded 10 % are marked, and
remove_deleted is timed with the engine's own clock (the growth of seconds3[2] of jv_hip_exact_builder_stats), split into count pass,
write pass and prune + row rewrite by the context's exact_delete_* counters, which also give the two-hop entries gathered against the
distinct ones scored.  Beside it the engine's seconds of a fresh ExactGraphBuilder build of the survivors (one level, same parameters and
batches), and recall@10 of ExactGraphSearcher at beamK 50 / 100 on both graphs over the same queries, ground truth over the survivors
only.  Report only, no bar.  One JSON object on stdout.
usage: python scripts/exact_delete_bench.py [N=1000000] [D=128] [runs=1]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
D = int(sys.argv[2]) if len(sys.argv) > 2 else 128
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 1
K, DEGREE, BEAM, ALPHA, OVERFLOW, BATCH, Q, FRAC = 10, 32, 100, 1.2, 1.25, 131072, 1000, 0.10
BEAMS = (50, 100)
PHASES = ("exact_delete_count_us", "exact_delete_merge_us", "exact_delete_prune_us", "exact_delete_raw_entries", "exact_delete_distinct")
T0 = time.perf_counter()


def log(msg):
    print(f"[exact_delete_bench +{time.perf_counter() - T0:.0f}s] {msg}", file=sys.stderr, flush=True)


def build(ctx, vs, n):
    gb = J.ExactGraphBuilder(ctx, vs, VSF.DOT_PRODUCT, DEGREE, BEAM, ALPHA, OVERFLOW)
    gb.seed(0)
    lo = 1
    while lo < n:
        hi = min(n, lo + min(BATCH, lo))
        gb.insert_batch(torch.arange(lo, hi, dtype=torch.int32, device="cuda:0"))
        lo = hi
    return gb


def seconds(gb):
    st = gb.stats()
    return st["search_s"] + st["prune_s"] + st["backlink_s"]


def recalls(ctx, gb, vs, n, queries, truth, ids_map=None):
    rows = gb.finish(np.empty((n, DEGREE), np.int32))
    g = J.GraphIndex(ctx, n, [(None, rows)], gb.entry, 0)
    searcher = J.ExactGraphSearcher(ctx, g, vs)
    out = {}
    for beam in BEAMS:
        ids = searcher.search(queries, VSF.DOT_PRODUCT, K, beam)[0].cpu().numpy()
        ids = ids if ids_map is None else np.where(ids >= 0, ids_map[np.maximum(ids, 0)], -1)
        out[str(beam)] = float(np.mean([len(set(ids[i].tolist()) & set(truth[i].tolist())) / K for i in range(len(ids))]))
    g.close()
    return out


dev = torch.device("cuda:0")
ctx = J.HipContext(0)
mix = benchlib.Mixture(D, 1, dev)
base = mix.sample(N, 2)
queries = mix.sample(Q, 3).contiguous()
gone = np.sort(np.random.default_rng(10).choice(N, int(N * FRAC), replace=False)).astype(np.int32)
keep = np.setdiff1d(np.arange(N), gone)
vs = J.VectorSet(ctx, base)
vk = J.VectorSet(ctx, base[torch.from_numpy(keep).to(dev)].contiguous())
truth = keep[benchlib.ground_truth(J, ctx, vk, queries, VSF.DOT_PRODUCT, K, dense=True, q_group=1024).cpu().numpy()]
out = {"n": N, "dim": D, "degree": DEGREE, "beam": BEAM, "alpha": ALPHA, "overflow": OVERFLOW, "batch": BATCH, "marked": len(gone), "runs": []}
for run in range(RUNS):
    gb = build(ctx, vs, N)
    case = {"build_all_s": seconds(gb)}
    gb.mark_deleted(gone)
    before, stat0 = gb.stats()["backlink_s"], [ctx.stat(p) for p in PHASES]
    case["counts"] = gb.remove_deleted(0)
    case["remove_deleted_s"] = gb.stats()["backlink_s"] - before
    count_us, merge_us, prune_us, raw, distinct = [ctx.stat(p) - s for p, s in zip(PHASES, stat0)]
    case.update(count_pass_s=count_us / 1e6, write_pass_s=merge_us / 1e6, prune_and_rewrite_s=prune_us / 1e6, two_hop_entries=raw, distinct_scored=distinct)
    case["recall_repaired"] = recalls(ctx, gb, vs, N, queries, truth)
    gb.close()
    gk = build(ctx, vk, len(keep))
    case["rebuild_survivors_s"] = seconds(gk)
    case["recall_rebuilt"] = recalls(ctx, gk, vk, len(keep), queries, truth, keep)
    gk.close()
    log(json.dumps(case))
    out["runs"].append(case)
print(json.dumps(out))
