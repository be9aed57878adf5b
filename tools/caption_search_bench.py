"""Video-to-text search throughput by stage, on random embeddings (bf16, G = 240 regions, W = 99 words; no towers: every figure starts from
embeddings, for the search and for the baseline alike).  One process on the card; each figure is the median of event-timed repeats after a
warm-up call.  Prints one JSON line per section:

  search        the whole query path after the object tower (global stage over the caption index, local re-rank on the resident captions,
                final k = 10) at N = 1 000 / 100 000 captions, 1 and 1 000 query videos, shortlist 50 and 200: per-stage milliseconds and
                videos/s
  vs_full_grid  N = 1 000 captions, 1 000 videos: search (shortlist 50) against the only way to answer without it -- the full 1000 x 1000
                local grid (RWALoss.get_sim_by_segment) plus sim_matrix and a host arg-sort per video

    python tools/caption_search_bench.py [--sizes 1000,100000] [--reps 7] [--no-full-grid]

Each size is a run of its own when asked for alone (``--sizes 100000 --no-full-grid``), so that a job script can give every step its own
time limit.
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
from demovlp_amd.search import CaptionIndex  # noqa: E402

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


def filled_index(N, gen):
    ix = CaptionIndex(N, W, torch.bfloat16, DEV)
    gt = torch.randn((1000, 256), device=DEV, generator=gen).bfloat16()
    lt = torch.randn((1000, W, 256), device=DEV, generator=gen).bfloat16()
    att = torch.ones((1000, W + 1), device=DEV, dtype=torch.long)
    for r0 in range(0, N, 1000):
        n = min(1000, N - r0)
        ix.add(gt[:n], lt[:n], att[:n])
    ix.gn.copy_(unit_rows(N, gen))                # distinct cosines per caption (the local side repeats every 1000 rows: timing only)
    return ix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,100000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-full-grid", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = RWALoss(20, "equal")

    videos = {nv: (unit_rows(nv, gen), torch.randn((nv, G, 256), device=DEV, generator=gen).bfloat16(), torch.zeros((nv, G), device=DEV)) for nv in (1, 1000)}
    for N in [int(s) for s in a.sizes.split(",") if s]:
        ix = filled_index(N, gen)
        for nv, (qn, lo, om) in videos.items():
            for S in (50, 200):
                ids, cos = ix._global_stage(qn, S, 65536)
                local = ix._local_stage(loss, lo, om, ids)
                t_g = ms(lambda: ix._global_stage(qn, S, 65536), a.reps)
                t_l = ms(lambda: ix._local_stage(loss, lo, om, ids), a.reps)
                t_f = ms(lambda: ops.topk_rows(cos + local, K_FINAL), a.reps)

                def whole():
                    i, c = ix._global_stage(qn, S, 65536)
                    ops.topk_rows(c + ix._local_stage(loss, lo, om, i), K_FINAL)
                t = ms(whole, a.reps)
                print(json.dumps({"section": "search", "N": N, "videos": nv, "shortlist": S, "k": K_FINAL, "global_ms": round(t_g, 3), "local_ms": round(t_l, 3),
                                  "final_ms": round(t_f, 3), "total_ms": round(t, 3), "vps": round(nv / t * 1e3, 1),
                                  "index_GB": round(ix.local.numel() / 1e9, 3)}), flush=True)
        if N == 1000 and not a.no_full_grid:
            qn, lo, om = videos[1000]
            lt = torch.randn((N, W, 256), device=DEV, generator=gen).bfloat16()
            gt, go = torch.randn((N, 256), device=DEV, generator=gen).bfloat16(), torch.randn((1000, 256), device=DEV, generator=gen).bfloat16()
            tm = ix.tm[:N]

            def full_grid():
                local = loss.get_sim_by_segment(lo, lt, om, None, tm, device=DEV)                       # numpy [video, text]
                s = sim_matrix(gt, go).float().cpu().numpy().T + local
                np.argsort(-s, axis=1, kind="stable")[:, :K_FINAL]

            def two_stage():
                i, c = ix._global_stage(qn, 50, 65536)
                v, p = ops.topk_rows(c + ix._local_stage(loss, lo, om, i), K_FINAL)
                torch.gather(i, 1, p.long()).cpu(), v.cpu()                                             # results on the host, like the baseline's
            t_full, t_two = ms(full_grid, a.reps), ms(two_stage, a.reps)
            print(json.dumps({"section": "vs_full_grid", "N": N, "videos": 1000, "shortlist": 50, "full_grid_ms": round(t_full, 2), "search_ms": round(t_two, 2),
                              "speedup": round(t_full / t_two, 2)}), flush=True)
        del ix


if __name__ == "__main__":
    main()
