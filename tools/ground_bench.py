"""What grounding costs: the grounding launch (dvlp_xattn_index_pairs_ground) against the score launch (dvlp_xattn_index_pairs_fwd) on the same
pairs, on random bf16 embeddings (G = 240 regions, W = 99 words, an index of 1 000 videos), for Nq x k = 1 000 x 10 and 1 x 10.  Both calls
include the caption-side prep and their output allocations, as a search issues them.  One process on the card; the two calls alternate
inside every repeat, each bracketed by its own event pair, and the figure is the median over the repeats after a warm-up of both.  Prints one
JSON line per size.

    python tools/ground_bench.py [--reps 21] [--videos 1000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demovlp_amd import ops  # noqa: E402

DEV = "cuda"
G, W, K, FRAMES = 240, 99, 10, 8


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--videos", type=int, default=1000)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    N = a.videos
    index = torch.zeros(ops.xattn_index_bytes(N, G), device=DEV, dtype=torch.uint8)
    ops.xattn_index_add(index, N, G, 0, torch.randn((N, G, 256), device=DEV, generator=gen).bfloat16())
    m_img = torch.zeros((N, G), device=DEV)
    for nq in (1000, 1):
        Q = torch.randn((nq, W, 256), device=DEV, generator=gen).bfloat16()
        m_cap = torch.zeros((nq, W), device=DEV)
        cand = torch.randint(0, N, (nq, K), device=DEV, generator=gen, dtype=torch.int32)
        score = lambda: ops.xattn_index_pairs_fwd(index, N, G, m_img, Q, m_cap, cand, 20.0, True)
        ground = lambda: ops.xattn_index_pairs_ground(index, N, G, m_img, Q, m_cap, cand, 20.0, True, frames=FRAMES)
        diff = float((score() - ground()["score"]).abs().max())           # the same pairs: 0 where the two launches round alike
        torch.cuda.synchronize()
        ts, tg = [], []
        for _ in range(a.reps):
            ts.append(timed(score))
            tg.append(timed(ground))
        s, g = float(np.median(ts)), float(np.median(tg))
        print(json.dumps({"section": "ground_vs_score", "videos": N, "G": G, "W": W, "queries": nq, "k": K, "frames": FRAMES, "reps": a.reps,
                          "score_max_abs_diff": diff, "score_ms": round(s, 4), "ground_ms": round(g, 4), "ratio": round(g / s, 3),
                          "score_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "ground_ms_min_max": [round(min(tg), 4), round(max(tg), 4)]}))


if __name__ == "__main__":
    main()
