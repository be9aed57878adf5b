"""Moment search in the video-to-text direction on random embeddings (bf16, G = 1152 regions = 32 frames x 36, W = 99 words, N = 1 000
resident captions; no towers: every figure starts from embeddings): every window of ``win`` frames at stride 1 of ``videos`` query videos
against ``cands`` captions each, three routes in one process.

  (a) moments   ``ops.xattn_long_caption_index_moments_fwd`` at ``windows_per_group`` = 1 (one window per workgroup: the
                form of 6i), M (one workgroup per pair: the caption staged once) and 0 (what the library's planner picks);
  (b) slices    the only route without it: per window, the query videos' embeddings and masks sliced to the window and scored by
                ``xattn_long_caption_index_pairs_fwd`` at G' = win x 36 (its video-side prep into the workspace is part of that call and
                is counted);
  (c) timeline  ``CaptionIndex.timeline`` end to end from the object-tower outputs (cosine shortlist of ``cands`` captions, the window-major
                launch, one ``dvlp_topk_rows`` over all windows), k = 5.

The routes are timed in turn, round after round (a1, aM, a0, b, c, a1, ...), after one warm-up call of each; every figure is the median of
``--reps`` event-timed calls, printed with the smallest and largest call beside it.  One JSON line per (videos, cands, win): microseconds
per (pair, window) on each route, the ratios against (b) and (a) at one window per workgroup, whether the three chunkings gave equal bytes,
and the largest score difference between (a) and (b).

    python tools/caption_moment_bench.py [--videos 1,8] [--cands 100,1000] [--wins 4,8,16] [--reps 7]
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
from demovlp_amd.search import CaptionIndex  # noqa: E402

DEV = "cuda"
F, R, W, LAM, GATE, N = 32, 36, 99, 20.0, True, 1000
G = F * R


def rounds(fns, reps):
    """every route called once to warm up, then ``reps`` rounds over the routes in turn -> {name: (median, min, max) in ms}"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts[name].append(ev[0].elapsed_time(ev[1]))
    return {name: (float(np.median(t)), float(min(t)), float(max(t))) for name, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", default="1,8")
    ap.add_argument("--cands", default="100,1000")
    ap.add_argument("--wins", default="4,8,16")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",") if x]
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = RWALoss(LAM, "equal")
    lt = torch.randn((N, W, 256), device=DEV, generator=gen).bfloat16()
    cix = CaptionIndex(N, W, torch.bfloat16, DEV, tiled=True)
    for r0 in range(0, N, 100):
        cix.add(torch.randn((100, 256), device=DEV, generator=gen).bfloat16(), lt[r0:r0 + 100], torch.ones((100, W + 1), device=DEV))
    model = torch.nn.Identity()                                # (timeline only asks it for its training flag: the towers are not run)
    for Bi in ints(a.videos):
        go = torch.randn((Bi, 256), device=DEV, generator=gen).bfloat16()
        C = torch.randn((Bi, G, 256), device=DEV, generator=gen).bfloat16()
        mi = torch.zeros((Bi, G), device=DEV)
        cix._video_side = lambda model, block, side=(go, C, mi): side
        data = dict(object=torch.zeros((Bi, F, R, 1), device=DEV), object_mask=torch.ones((Bi, F, R), device=DEV))
        for K in ints(a.cands):
            cand = torch.stack([torch.randperm(N, device=DEV, generator=gen)[:K] for _ in range(Bi)]).to(torch.int32).contiguous()
            for win in ints(a.wins):
                M, Gw = F - win + 1, win * R
                mom = lambda n: ops.xattn_long_caption_index_moments_fwd(cix.local, N, W, cix.tm, C, mi, cand, F, win, 1, LAM, GATE,
                                                                         windows_per_group=n)

                def slices():
                    return torch.stack([ops.xattn_long_caption_index_pairs_fwd(cix.local, N, W, cix.tm, C[:, m * R:m * R + Gw].contiguous(),
                                                                               mi[:, m * R:m * R + Gw].contiguous(), cand, LAM, GATE)
                                        for m in range(M)], 2)

                with torch.no_grad():
                    one = mom(1)
                    same = bool(torch.equal(one.view(torch.int32), mom(M).view(torch.int32)) and
                                torch.equal(one.view(torch.int32), mom(0).view(torch.int32)))
                    diff = float((one - slices()).abs().max())
                    t = rounds({"a1": lambda: mom(1), "aM": lambda: mom(M), "a0": lambda: mom(0), "b": slices,
                                "c": lambda: cix.timeline(model, loss, data, F, win, k=5, shortlist=K)}, a.reps)
                pw = Bi * K * M
                us = lambda name: [round(x * 1e3 / pw, 4) for x in t[name]]
                print(json.dumps({"section": "caption_moment_bench", "G": G, "frames": F, "W": W, "captions": N, "videos": Bi, "cands": K,
                                  "win": win, "windows": M, "pair_windows": pw, "reps": a.reps,
                                  "moments_wpg1_us_per_pair_window_med_min_max": us("a1"),
                                  "moments_wpgM_us_per_pair_window_med_min_max": us("aM"),
                                  "moments_planner_us_per_pair_window_med_min_max": us("a0"),
                                  "slices_us_per_pair_window_med_min_max": us("b"),
                                  "timeline_us_per_pair_window_med_min_max": us("c"),
                                  "moments_wpg1_ms": round(t["a1"][0], 3), "moments_wpgM_ms": round(t["aM"][0], 3),
                                  "moments_planner_ms": round(t["a0"][0], 3), "slices_ms": round(t["b"][0], 3), "timeline_ms": round(t["c"][0], 3),
                                  "wpgM_over_wpg1": round(t["aM"][0] / t["a1"][0], 3), "planner_over_wpg1": round(t["a0"][0] / t["a1"][0], 3),
                                  "slices_over_wpg1": round(t["b"][0] / t["a1"][0], 3), "chunkings_byte_equal": same,
                                  "max_abs_score_diff_slices": diff}), flush=True)
        del cix._video_side


if __name__ == "__main__":
    main()
