"""Text-to-video search over LONG videos by stage, on random embeddings (bf16, G = 1152 and 960 regions, W = 99 words, N = 1 000 videos; no
towers: every figure starts from embeddings).  The local stage runs twice on the same queries and shortlists, in one process: on a
``VideoIndex(..., tiled=True)`` (the region-tiled pair kernel) and on the default index of that shape, which takes the parity
route (one multi-kernel ``RWALoss.get_sim`` call per query).  Each figure is the median of event-timed repeats after a warm-up call; the
parity route at 1 000 queries is timed once after a one-query warm-up (it takes seconds).  Prints one JSON line per (G, queries, shortlist):
per-stage milliseconds, the local stage per pair on both routes, queries/s and the largest score difference between the routes.

    python tools/long_search_bench.py [--regions 1152,960] [--videos 1000] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demovlp_amd import ops  # noqa: E402
from demovlp_amd.loss import RWALoss  # noqa: E402
from demovlp_amd.search import VideoIndex  # noqa: E402

DEV = "cuda"
W, K_FINAL = 99, 10


def ms(fn, reps, warm=None):
    (warm or fn)()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(ts))


def unit_rows(n, gen):
    x = torch.randn((n, 256), device=DEV, generator=gen)
    return x / x.norm(dim=1, keepdim=True)


def filled_pair(N, G, gen):
    """the same N videos in a tiled index and in a default (parity-route) one"""
    tiled, parity = VideoIndex(N, G, torch.bfloat16, DEV, tiled=True), VideoIndex(N, G, torch.bfloat16, DEV)
    assert tiled.tiled and not parity.fused and not parity.tiled
    for r0 in range(0, N, 100):
        n = min(100, N - r0)
        block = dict(global_object_embeddings=torch.randn((n, 256), device=DEV, generator=gen).bfloat16(),
                     local_object_embeddings=torch.randn((n, G, 256), device=DEV, generator=gen).bfloat16(),
                     object_mask=torch.zeros((n, G), device=DEV))
        tiled.add(block)
        parity.add(block)
    return tiled, parity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", default="1152,960")
    ap.add_argument("--videos", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = RWALoss(20, "equal")
    N = a.videos
    queries = {nq: (unit_rows(nq, gen), torch.randn((nq, W, 256), device=DEV, generator=gen).bfloat16(), torch.zeros((nq, W), device=DEV)) for nq in (1, 1000)}
    for G in [int(s) for s in a.regions.split(",") if s]:
        tiled, parity = filled_pair(N, G, gen)
        for nq, (qn, lt, tm) in queries.items():
            for S in (50, 200):
                with torch.no_grad():
                    ids, cos = tiled._global_stage(qn, S, 65536)
                    local = tiled._local_stage(loss, lt, tm, ids)
                    t_g = ms(lambda: tiled._global_stage(qn, S, 65536), a.reps)
                    t_l = ms(lambda: tiled._local_stage(loss, lt, tm, ids), a.reps)
                    t_f = ms(lambda: ops.topk_rows(cos + local, K_FINAL), a.reps)

                    def whole():
                        i, c = tiled._global_stage(qn, S, 65536)
                        ops.topk_rows(c + tiled._local_stage(loss, lt, tm, i), K_FINAL)
                    t = ms(whole, a.reps)
                    t_p = ms(lambda: parity._local_stage(loss, lt, tm, ids), a.reps if nq == 1 else 1,
                             warm=lambda: parity._local_stage(loss, lt[:1], tm[:1], ids[:1]))
                    diff = float((parity._local_stage(loss, lt[:8], tm[:8], ids[:8]) - local[:8]).abs().max())
                pairs = nq * S
                print(json.dumps({"section": "long_search", "G": G, "N": N, "queries": nq, "shortlist": S, "k": K_FINAL, "global_ms": round(t_g, 3),
                                  "local_ms": round(t_l, 3), "final_ms": round(t_f, 3), "total_ms": round(t, 3), "qps": round(nq / t * 1e3, 1),
                                  "local_us_per_pair": round(t_l * 1e3 / pairs, 3), "parity_local_ms": round(t_p, 3),
                                  "parity_us_per_pair": round(t_p * 1e3 / pairs, 3), "parity_over_tiled": round(t_p / t_l, 2),
                                  "max_abs_score_diff": diff}), flush=True)
        del tiled, parity
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
