#!/usr/bin/env python
"""Robust prune with exact scores on the device (jv_hip_exact_retain_diverse) against what a caller composed before it existed:
jv_hip_exact_pair_scores over the P x C x C block of every list, then a sequential loop on the host.  Only the DEVICE part of that
composition is timed (the pair scores, in chunks of nodes that keep the score block under 256 MB, every buffer on the device): the
host loop over 16384 lists in numpy takes minutes and would make the ratio meaningless.

Rows: N = 2^20 in 4096 clusters of 256 (centre + 0.35 noise), so the prune has something to reject; a node's list is C rows of its own
cluster scored against it with jv_hip_exact_pair_scores and sorted descending.  usage: exact_build_bench.py [D ...] (default 128 768)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jvector_amd as J  # noqa: E402
from jvector_amd import VectorSimilarityFunction as VSF  # noqa: E402

N, P, C, MAX_DEGREE, ALPHA, BLOCK = 1 << 20, 16384, 128, 32, 1.2, 256
WARMUP, ITERS = 2, 5


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ITERS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ctx = J.HipContext(0)
    for D in [int(a) for a in sys.argv[1:]] or [128, 768]:
        g = torch.Generator(device="cuda").manual_seed(1234 + D)
        centres = torch.randn((N // BLOCK, D), generator=g, device="cuda")
        rows = (centres.repeat_interleave(BLOCK, 0) + 0.35 * torch.randn((N, D), generator=g, device="cuda")).contiguous()
        del centres
        vs = J.VectorSet(ctx, rows)
        node = torch.randint(0, N, (P,), generator=g, device="cuda", dtype=torch.int32)
        cand = ((node // BLOCK * BLOCK)[:, None] + torch.rand((P, BLOCK), generator=g, device="cuda").argsort(1)[:, :C]).to(torch.int32).contiguous()
        for vsf in (VSF.EUCLIDEAN, VSF.DOT_PRODUCT, VSF.COSINE):
            sc = vs.pair_scores(vsf, node, cand)
            sc, order = torch.sort(sc, dim=1, descending=True, stable=True)
            nodes = torch.gather(cand, 1, order.to(torch.int64)).contiguous()
            scorer = J.ExactBuildScorer(ctx, None, vs, vsf)
            out = {}

            def prune():
                out["r"] = scorer.retain_diverse(nodes, sc.contiguous(), MAX_DEGREE, ALPHA)

            chunk = max(1, (256 << 20) // (4 * C * C))   # nodes per pair-score call

            def composition():
                for p0 in range(0, P, chunk):
                    sub = nodes[p0:p0 + chunk]
                    vs.pair_scores(vsf, sub.reshape(-1), sub.repeat_interleave(C, 0))

            new_ms, comp_ms = timed(prune), timed(composition)
            n_sel = out["r"][1].float().mean().item()
            print(json.dumps({"N": N, "D": D, "P": P, "C": C, "max_degree": MAX_DEGREE, "alpha": ALPHA, "vsf": vsf.name,
                              "retain_ms_median_min_max": [round(x, 3) for x in new_ms],
                              "pair_scores_device_part_ms_median_min_max": [round(x, 3) for x in comp_ms],
                              "ratio_retain_over_pair_scores": round(new_ms[0] / comp_ms[0], 3), "mean_n_selected": round(n_sel, 2)}), flush=True)
        vs.close()
        del rows
    ctx.close()


if __name__ == "__main__":
    main()
