"""The exact flat search on the MI355X (jv_hip_search_exact, fused route, topK 10, candK 40) against the composition it replaces as
benchlib.ground_truth(dense=True) runs it, on the same inputs, alternated call by call: median wall time per call after a warm-up, and
the peak device memory of each side (torch's allocator for the composition's tensors plus the growth of the engine's own scratch, read
from the driver's free memory).  Prints one JSON object.

usage: python scripts/exact_flat_bench.py [--n 1048576] [--d 768] [--q 2048] [--mask 0.5] [--reps 5] [--vsf 1]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np
import torch

import jvector_amd as J
from benchlib import ground_truth
from jvector_amd.flat_filtered import pack_accept


def used_bytes():
    free, total = torch.cuda.mem_get_info()
    return total - free


def timed(fn, ctx, reps):
    fn()   # warm-up: scratch buffers grow here
    ctx.sync()
    times, peak = [], used_bytes()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        peak = max(peak, used_bytes())
    return out, statistics.median(times), min(times), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--q", type=int, default=2048)
    ap.add_argument("--mask", type=float, default=0.0, help="share of the rows a shared mask accepts; 0: no mask (search_exact only)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vsf", type=int, default=1)
    a = ap.parse_args()
    vsf, k = J.VectorSimilarityFunction(a.vsf), 10
    g = torch.Generator(device="cuda").manual_seed(1)
    vecs = torch.randn(a.n, a.d, device="cuda", generator=g)
    queries = torch.randn(a.q, a.d, device="cuda", generator=g)
    ctx = J.HipContext(0)
    vs = J.VectorSet(ctx, vecs)
    base = used_bytes()
    res = {"n": a.n, "d": a.d, "q": a.q, "vsf": vsf.name, "top_k": k, "cand_k": 4 * k, "mask": a.mask, "reps": a.reps}

    accept = None
    if a.mask > 0:
        m = np.random.default_rng(2).random(a.n) < a.mask
        accept = torch.from_numpy(pack_accept(m).view(np.int64)).cuda()
    gt = None
    if accept is None:   # the composition has no accept filter: it is timed without a mask only, and first
        torch.cuda.reset_peak_memory_stats()
        t_before = torch.cuda.memory_allocated()
        gt, med, best, peak = timed(lambda: ground_truth(J, ctx, vs, queries, vsf, k, dense=True), ctx, a.reps)
        res["composition"] = {"median_ms": med, "min_ms": best, "peak_bytes_over_data": peak - base,
                              "torch_peak_bytes": torch.cuda.max_memory_allocated() - t_before}
        torch.cuda.empty_cache()   # the composition's score buffer goes back to the driver before the other side runs
    ctx.set_option("exact_flat_fused", 1)
    stats = ("exact_flat_fused_calls", "exact_flat_fallbacks", "exact_flat_listed")
    before = [ctx.stat(s) for s in stats]
    base = used_bytes()
    (ids, _), med, best, peak = timed(lambda: vs.search_exact(queries, vsf, k, 4 * k, accept=accept), ctx, a.reps)
    res["search_exact"] = {"median_ms": med, "min_ms": best, "peak_bytes_over_data": peak - base,
                           **{s: (ctx.stat(s) - b) // (a.reps + 1) for s, b in zip(stats, before)}}
    if gt is not None:
        res["same_ids"] = bool(torch.equal(gt.cpu(), ids.cpu()))
        res["time_ratio"] = res["search_exact"]["median_ms"] / res["composition"]["median_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
