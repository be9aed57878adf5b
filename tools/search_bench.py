"""Text-to-video search throughput by stage, on random embeddings (bf16, G = 240 regions, W = 99 words; no towers: every figure starts from
embeddings, for the search and for the baseline alike).  One process on the card; each figure is the median of event-timed repeats after a
warm-up call.  Prints one JSON line per section:

  topk_scan     dvlp_topk_rows on [M, 2^20] fp32, K = 100, M = 1 and 1000: microseconds and bytes read over the time (GB/s)
  global_stage  cosine product + top-k shortlist over N = 1 000 / 100 000 / 1 000 000 videos, 1 and 1 000 queries, shortlist 50 and 200
  search        the whole query path after the text tower (global stage, local re-rank on the resident index, final k = 10) at N = 1 000 /
                100 000, 1 and 1 000 queries, shortlist 50 and 200: per-stage milliseconds and queries/s
  vs_full_grid  N = 1 000 videos, 1 000 queries: search (shortlist 50) against the only way to answer without it -- the full 1000 x 1000
                local grid (RWALoss.get_sim_by_segment) plus sim_matrix and a host arg-sort

    python tools/search_bench.py [--sizes 1000,100000] [--global-only-sizes 1000000] [--reps 7]
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
from demovlp_amd.model import sim_matrix  # noqa: E402
from demovlp_amd.search import VideoIndex  # noqa: E402

DEV = "cuda"
G, W, K_FINAL = 240, 99, 10


def ms(fn, reps):
    fn()
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


def global_only_index(N, gen):
    ix = VideoIndex(N, G, torch.bfloat16, DEV)
    ix.gn, ix.n = unit_rows(N, gen), N            # the global stage reads nothing else
    return ix


def filled_index(N, gen):
    ix = VideoIndex(N, G, torch.bfloat16, DEV)
    block = dict(global_object_embeddings=torch.randn((1000, 256), device=DEV, generator=gen).bfloat16(),
                 local_object_embeddings=torch.randn((1000, G, 256), device=DEV, generator=gen).bfloat16(),
                 object_mask=torch.zeros((1000, G), device=DEV))
    for r0 in range(0, N, 1000):
        n = min(1000, N - r0)
        ix.add({k: v[:n] for k, v in block.items()})
    ix.gn.copy_(unit_rows(N, gen))                # distinct cosines per video (the local side repeats every 1000 rows: timing only)
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,100000")
    ap.add_argument("--global-only-sizes", default="1000000")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = RWALoss(20, "equal")

    for M in (1, 1000):
        x = torch.randn((M, 1 << 20), device=DEV, generator=gen)
        t = ms(lambda: ops.topk_rows(x, 100), a.reps)
        print(json.dumps({"section": "topk_scan", "M": M, "N": 1 << 20, "K": 100, "us": round(t * 1e3, 1), "GBps": round(x.numel() * 4 / t / 1e6, 1)}))
        del x

    queries = {nq: (unit_rows(nq, gen), torch.randn((nq, W, 256), device=DEV, generator=gen).bfloat16(), torch.zeros((nq, W), device=DEV)) for nq in (1, 1000)}
    for N in [int(s) for s in a.global_only_sizes.split(",") if s]:
        ix = global_only_index(N, gen)
        for nq, (qn, _, _) in queries.items():
            for S in (50, 200):
                t = ms(lambda: ix._global_stage(qn, S, 65536), a.reps)
                print(json.dumps({"section": "global_stage", "N": N, "queries": nq, "shortlist": S, "ms": round(t, 3), "qps": round(nq / t * 1e3, 1)}))
        del ix

    for N in [int(s) for s in a.sizes.split(",") if s]:
        ix = filled_index(N, gen)
        for nq, (qn, lt, tm) in queries.items():
            for S in (50, 200):
                ids, cos = ix._global_stage(qn, S, 65536)
                local = ix._local_stage(loss, lt, tm, ids)
                t_g = ms(lambda: ix._global_stage(qn, S, 65536), a.reps)
                t_l = ms(lambda: ix._local_stage(loss, lt, tm, ids), a.reps)
                t_f = ms(lambda: ops.topk_rows(cos + local, K_FINAL), a.reps)

                def whole():
                    i, c = ix._global_stage(qn, S, 65536)
                    ops.topk_rows(c + ix._local_stage(loss, lt, tm, i), K_FINAL)
                t = ms(whole, a.reps)
                print(json.dumps({"section": "search", "N": N, "queries": nq, "shortlist": S, "k": K_FINAL, "global_ms": round(t_g, 3), "local_ms": round(t_l, 3),
                                  "final_ms": round(t_f, 3), "total_ms": round(t, 3), "qps": round(nq / t * 1e3, 1)}))
        if N == 1000:
            qn, lt, tm = queries[1000]
            lo = torch.randn((N, G, 256), device=DEV, generator=gen).bfloat16()
            go, gt = torch.randn((N, 256), device=DEV, generator=gen).bfloat16(), torch.randn((1000, 256), device=DEV, generator=gen).bfloat16()

            def full_grid():
                local = loss.get_sim_by_segment(lo, lt, ix.om, None, tm, device=DEV)                    # numpy [video, text]
                s = sim_matrix(gt, go).float().cpu().numpy() + local.T
                np.argsort(-s, axis=1, kind="stable")[:, :K_FINAL]

            def two_stage():
                i, c = ix._global_stage(qn, 50, 65536)
                v, p = ops.topk_rows(c + ix._local_stage(loss, lt, tm, i), K_FINAL)
                torch.gather(i, 1, p.long()).cpu(), v.cpu()                                             # results on the host, like the baseline's
            t_full, t_two = ms(full_grid, a.reps), ms(two_stage, a.reps)
            print(json.dumps({"section": "vs_full_grid", "N": N, "queries": 1000, "shortlist": 50, "full_grid_ms": round(t_full, 2), "search_ms": round(t_two, 2),
                              "speedup": round(t_full / t_two, 2)}))
        del ix


if __name__ == "__main__":
    main()
