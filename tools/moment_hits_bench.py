"""Moment retrieval on random embeddings (bf16, G = 1152 regions = 32 frames x 36, W = 99 words; no towers: every figure starts from
embeddings): windows of 2, 4 and 8 frames at stride 1 (M_total = 31 + 29 + 25 = 85), a shortlist of S = 100 videos, per_video = 3 hits per
video, iou = 0.5.  One process on the card; each figure is the median of event-timed repeats after a warm-up call, with the spread
(min .. max) of the repeats beside it.  Prints one JSON line per section:

  moment_select    ``dvlp_moment_select`` alone on random N(0, 1) window scores [Nq S, M_total] for Nq = 1 and 1000, against the same
                   selection in plain torch in the same process (``torch_select``: per_video rounds of a masked ``max`` over the row, the
                   overlap of every window with the pick, and a mask update -- about a dozen launches per round over [Nq S, M_total]
                   temporaries); ``agree`` says whether both return the same positions (random scores: no ties).
  search_moments   ``VideoIndex.search_moments`` end to end on a random tiled index (text-tower outputs replaced by random embeddings), with
                   the share of its parts: the global stage, the window scores (``dvlp_xattn_long_index_moments_fwd``, one launch per
                   window length over all S candidates) and the selection.

    python tools/moment_hits_bench.py [--videos 200] [--queries 1,16] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demovlp_amd import ops, search  # noqa: E402
from demovlp_amd.loss import RWALoss  # noqa: E402

DEV = "cuda"
F, R, W, LAM = 32, 36, 99, 20.0
G, WINDOWS, STRIDE, S, PER_VIDEO, IOU = F * R, (2, 4, 8), 1, 100, 3, 0.5


def ms(fn, reps):
    """-> (median, min, max) milliseconds of ``reps`` event-timed calls after one warm-up call"""
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def put(row, name, t):
    row[name + "_ms"], row[name + "_spread"] = round(t[0], 3), [round(t[1], 3), round(t[2], 3)]


def torch_select(scores, start, length, T, iou):
    """``dvlp_moment_select`` in plain torch: T rounds of masked max + overlap mask over the whole [P, M] matrix"""
    minus = torch.full((), float("-inf"), device=scores.device)
    x = torch.where(torch.isnan(scores), minus, scores)
    alive = x > minus
    pad = torch.where(torch.isnan(scores).any(1), torch.full((), float("nan"), device=scores.device), minus)
    end = start + length
    vals, poss = [], []
    for _ in range(T):
        v, p = torch.where(alive, x, minus).max(1)
        ok = v > minus
        s, l = start[p][:, None], length[p][:, None]
        inter = (torch.minimum(end[None], s + l) - torch.maximum(start[None], s)).clamp(min=0)
        union = length[None] + l - inter
        alive &= ~(inter.float() > union.float() * iou)
        alive.scatter_(1, p[:, None], False)
        vals.append(torch.where(ok, v, pad))
        poss.append(torch.where(ok, p, torch.full_like(p, -1)))
    return torch.stack(vals, 1), torch.stack(poss, 1).int()


class NoTowers(torch.nn.Module):
    """stands in for the model: ``search_moments`` only flips its training flag once the text side is replaced"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=200)
    ap.add_argument("--queries", default="1,16")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    reps = max(7, a.reps)
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    starts, lengths = search.moment_windows(F, WINDOWS, STRIDE)
    start, length = starts.to(DEV).int(), lengths.to(DEV).int()
    M = int(starts.numel())

    for nq in (1, 1000):
        scores = torch.randn((nq * S, M), device=DEV, generator=gen)
        row = {"section": "moment_select", "queries": nq, "rows": nq * S, "windows": M, "per_video": PER_VIDEO, "iou": IOU}
        kpos = ops.moment_select(scores, start, length, PER_VIDEO, IOU)[1]
        row["agree"] = bool(torch.equal(kpos, torch_select(scores, start, length, PER_VIDEO, IOU)[1]))
        put(row, "kernel", ms(lambda: ops.moment_select(scores, start, length, PER_VIDEO, IOU), reps))
        put(row, "torch", ms(lambda: torch_select(scores, start, length, PER_VIDEO, IOU), reps))
        row["torch_over_kernel"] = round(row["torch_ms"] / row["kernel_ms"], 2)
        print(json.dumps(row), flush=True)

    N = a.videos
    ix = search.VideoIndex(N, G, torch.bfloat16, DEV, tiled=True)
    for r0 in range(0, N, 50):
        n = min(50, N - r0)
        ix.add(dict(global_object_embeddings=torch.randn((n, 256), device=DEV, generator=gen).bfloat16(),
                    local_object_embeddings=torch.randn((n, G, 256), device=DEV, generator=gen).bfloat16(),
                    object_mask=torch.zeros((n, G), device=DEV)))
    loss, model = RWALoss(LAM, "equal"), NoTowers()
    for nq in [int(q) for q in a.queries.split(",") if q]:
        side = (torch.randn((nq, 256), device=DEV, generator=gen).bfloat16(), torch.randn((nq, W, 256), device=DEV, generator=gen).bfloat16(),
                torch.zeros((nq, W), device=DEV))
        ix._text_side = lambda model, text, side=side: side                    # no text tower: the embeddings above
        text = {"input_ids": torch.zeros((nq, W + 1), device=DEV, dtype=torch.long)}
        qn = ops.rownorm_fwd(side[0].contiguous())[0]
        ids, _ = ix._global_stage(qn, S, 65536)
        with torch.no_grad():
            scores = ix._window_scores(loss, side, ids, F, list(WINDOWS), STRIDE)
            row = {"section": "search_moments", "videos": N, "queries": nq, "shortlist": S, "windows": M, "per_video": PER_VIDEO, "iou": IOU, "k": 10}
            put(row, "end_to_end", ms(lambda: ix.search_moments(model, loss, text, k=10, frames=F, windows=WINDOWS, stride=STRIDE, per_video=PER_VIDEO,
                                                                iou=IOU, shortlist=S), reps))
            put(row, "global_stage", ms(lambda: ix._global_stage(qn, S, 65536), reps))
            put(row, "window_scores", ms(lambda: ix._window_scores(loss, side, ids, F, list(WINDOWS), STRIDE), reps))
            put(row, "moment_select", ms(lambda: ops.moment_select(scores, start, length, PER_VIDEO, IOU), reps))
        row["window_scores_us_per_pair_window"] = round(row["window_scores_ms"] * 1e3 / (nq * S * M), 3)
        print(json.dumps(row), flush=True)
        del ix._text_side


if __name__ == "__main__":
    main()
