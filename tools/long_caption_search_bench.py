"""Video-to-text search with LONG query videos by stage, on random embeddings (bf16, W = 99 words, G = 960 and 1152 regions, N = 1 000
captions in a ``CaptionIndex(..., tiled=True)``; no towers: every figure starts from embeddings).  The local stage
(``dvlp_xattn_long_caption_index_pairs_fwd``, the region-tiled pair kernel on the video-major grid) is timed beside two other
routes to the same pairs, in the same process:

  get_sim      one bf16 ``RWALoss.get_sim`` call on a [1, S] grid per query video (the multi-kernel route; what a default index of this
               shape would have to do);
  query-major  ``ops.xattn_long_index_pairs_fwd`` over the transposed pair list: the query videos in a resident video index, one row per
               caption that occurs, its videos as candidates, -1 where a caption has fewer than the longest row.  Its scores are compared
               with the video-major launch's bit for bit.

Each figure is the median of event-timed repeats after a warm-up call; the get_sim loop at 1 000 videos is timed once after a one-video
warm-up (it takes seconds).  Prints one JSON line per (G, videos, shortlist).

    python tools/long_caption_search_bench.py [--regions 960,1152] [--captions 1000] [--reps 7]
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
W, K_FINAL = 99, 10
LAM, GATE = 20.0, True


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


def transposed(ids):
    """The pairs (video i, caption ids[i, k]) caption-major: (captions that occur [Bj], cand int32 [Bj, Kmax] of video rows with -1 fillers,
    and for pair i S + k its (row, column) there)."""
    nv, S = ids.shape
    j = ids.flatten().long()
    i = torch.arange(nv, device=DEV).repeat_interleave(S)
    j_sorted, order = torch.sort(j, stable=True)
    uniq, counts = torch.unique_consecutive(j_sorted, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    group = torch.repeat_interleave(torch.arange(uniq.numel(), device=DEV), counts)
    pos = torch.arange(j.numel(), device=DEV) - start[group]
    cand = torch.full((uniq.numel(), int(counts.max())), -1, device=DEV, dtype=torch.int32)
    cand[group, pos] = i[order].int()
    row, col = torch.empty_like(group), torch.empty_like(pos)
    row[order], col[order] = group, pos
    return uniq, cand, row, col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", default="960,1152")
    ap.add_argument("--captions", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = RWALoss(LAM, "equal")
    N = a.captions
    lt = torch.randn((N, W, 256), device=DEV, generator=gen).bfloat16()
    cix = CaptionIndex(N, W, torch.bfloat16, DEV, tiled=True)
    for r0 in range(0, N, 100):
        n = min(100, N - r0)
        cix.add(torch.randn((n, 256), device=DEV, generator=gen).bfloat16(), lt[r0:r0 + n], torch.ones((n, W + 1), device=DEV))
    assert cix.tiled and len(cix) == N
    for G in [int(s) for s in a.regions.split(",") if s]:
        for nv in (1, 1000):
            qn = unit_rows(nv, gen)
            lo = torch.randn((nv, G, 256), device=DEV, generator=gen).bfloat16()
            om = torch.zeros((nv, G), device=DEV)
            vidx = torch.zeros(ops.xattn_long_index_bytes(nv, G), device=DEV, dtype=torch.uint8)      # the query-major route's resident side
            ops.xattn_long_index_add(vidx, nv, G, 0, lo)
            for S in (50, 200):
                with torch.no_grad():
                    ids, cos = cix._global_stage(qn, S, 65536)
                    local = cix._local_stage(loss, lo, om, ids)
                    t_g = ms(lambda: cix._global_stage(qn, S, 65536), a.reps)
                    t_l = ms(lambda: cix._local_stage(loss, lo, om, ids), a.reps)
                    t_f = ms(lambda: ops.topk_rows(cos + local, K_FINAL), a.reps)

                    def whole():
                        i, c = cix._global_stage(qn, S, 65536)
                        ops.topk_rows(c + cix._local_stage(loss, lo, om, i), K_FINAL)
                    t = ms(whole, a.reps)

                    def get_sim_loop(n=nv):
                        out = torch.empty((n, S), device=DEV)
                        for v in range(n):
                            rows = ids[v].long()
                            out[v] = loss.get_sim(lo[v:v + 1], lt[rows], om[v:v + 1], None, cix.tm[rows])[0]
                        return out
                    t_p = ms(get_sim_loop, a.reps if nv == 1 else 1, warm=lambda: get_sim_loop(1))
                    diff = float((get_sim_loop(min(nv, 8)) - local[:8]).abs().max())

                    uniq, cand, row, col = transposed(ids)
                    Q, qm = lt[uniq].contiguous(), cix.tm[uniq].contiguous()
                    qmajor = lambda: ops.xattn_long_index_pairs_fwd(vidx, nv, G, om, Q, qm, cand, LAM, GATE)
                    back = qmajor()[row, col].view(nv, S)
                    same = bool(torch.equal(back.view(torch.int32), local.view(torch.int32)))
                    t_q = ms(qmajor, a.reps)
                pairs = nv * S
                print(json.dumps({"section": "long_caption_search", "G": G, "N": N, "videos": nv, "shortlist": S, "k": K_FINAL,
                                  "global_ms": round(t_g, 3), "local_ms": round(t_l, 3), "final_ms": round(t_f, 3), "total_ms": round(t, 3),
                                  "videos_per_s": round(nv / t * 1e3, 1), "local_us_per_pair": round(t_l * 1e3 / pairs, 3),
                                  "get_sim_local_ms": round(t_p, 3), "get_sim_us_per_pair": round(t_p * 1e3 / pairs, 3),
                                  "get_sim_over_tiled": round(t_p / t_l, 2), "max_abs_score_diff_get_sim": diff,
                                  "query_major_ms": round(t_q, 3), "query_major_us_per_pair": round(t_q * 1e3 / pairs, 3),
                                  "video_major_over_query_major": round(t_l / t_q, 3), "query_major_rows": int(cand.shape[0]),
                                  "query_major_row_length": int(cand.shape[1]), "query_major_fillers": int((cand < 0).sum()),
                                  "bit_equal_to_query_major": same}), flush=True)
            del lo, vidx
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
