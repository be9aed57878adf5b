"""Moment search on random embeddings (bf16, G = 1152 regions = 32 frames x 36, W = 99 words; no towers: every figure starts from
embeddings): every window of ``win`` frames at stride 1 of every (query, candidate) pair, two ways in one process.

  in place   ``ops.xattn_long_index_moments_fwd`` on the resident tiled index: one launch per window length;
  rebuild    the only route without it: per window, the candidates' embeddings sliced to the window, a temporary tiled index built from the
             slices (``xattn_long_index_bytes`` / ``_add`` at G' = win x 36) and scored by ``xattn_long_index_pairs_fwd``.  The index builds
             are counted; the score launches alone (``pairs_us``: the whole-video pair kernel at G' = win x 36) are reported beside them.

Each figure is the median of event-timed repeats after a warm-up call.  Prints one JSON line per window length: microseconds per
(pair, window) on both routes, their ratio and the largest score difference between them.

    python tools/moment_bench.py [--videos 32] [--queries 16] [--cands 10] [--reps 7]
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
F, R, W, LAM, GATE = 32, 36, 99, 20.0, True
G = F * R


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=32)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--cands", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    N, Nq, K = a.videos, a.queries, a.cands
    C = torch.randn((N, G, 256), device=DEV, generator=gen).bfloat16()
    Q = torch.randn((Nq, W, 256), device=DEV, generator=gen).bfloat16()
    mi, mc = torch.zeros((N, G), device=DEV), torch.zeros((Nq, W), device=DEV)
    cand = torch.randint(0, N, (Nq, K), device=DEV, generator=gen).to(torch.int32)
    index = torch.zeros(ops.xattn_long_index_bytes(N, G), device=DEV, dtype=torch.uint8)
    ops.xattn_long_index_add(index, N, G, 0, C)
    pairs = Nq * K
    for win in (4, 8, 16):
        M, Gw = F - win + 1, win * R
        miw = torch.zeros((N, Gw), device=DEV)

        def build(m):
            tmp = torch.zeros(ops.xattn_long_index_bytes(N, Gw), device=DEV, dtype=torch.uint8)
            ops.xattn_long_index_add(tmp, N, Gw, 0, C[:, m * R:m * R + Gw].contiguous())
            return tmp

        def rebuild():
            return torch.stack([ops.xattn_long_index_pairs_fwd(build(m), N, Gw, miw, Q, mc, cand, LAM, GATE) for m in range(M)], 2)

        one = build(0)
        with torch.no_grad():
            got = ops.xattn_long_index_moments_fwd(index, N, G, mi, Q, mc, cand, F, win, 1, LAM, GATE)
            diff = float((got - rebuild()).abs().max())
            t_in = ms(lambda: ops.xattn_long_index_moments_fwd(index, N, G, mi, Q, mc, cand, F, win, 1, LAM, GATE), a.reps)
            t_re = ms(rebuild, a.reps)
            t_pairs = ms(lambda: ops.xattn_long_index_pairs_fwd(one, N, Gw, miw, Q, mc, cand, LAM, GATE), a.reps)
        print(json.dumps({"section": "moment_bench", "G": G, "frames": F, "W": W, "videos": N, "pairs": pairs, "win": win, "windows": M,
                          "in_place_ms": round(t_in, 3), "in_place_us_per_pair_window": round(t_in * 1e3 / (pairs * M), 3),
                          "rebuild_ms": round(t_re, 3), "rebuild_us_per_pair_window": round(t_re * 1e3 / (pairs * M), 3),
                          "rebuild_over_in_place": round(t_re / t_in, 2), "pairs_us": round(t_pairs * 1e3 / pairs, 3),
                          "in_place_over_pairs": round(t_in / M / t_pairs, 2), "max_abs_score_diff": diff}), flush=True)


if __name__ == "__main__":
    main()
