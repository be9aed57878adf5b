"""What a filter costs the global stage of search, on random embeddings (no towers, no local stage: the mask lives in the global stage
alone).  One process on the card; each figure is the median of event-timed repeats after a warm-up call, with the spread (min .. max) of
the repeats beside it.  The sizes are those of tools/search_bench.py.  Prints one JSON line per (N, queries, shortlist):

  none_ms        (a) ``_global_stage`` without a mask: ``dvlp_gemm`` + ``dvlp_topk_rows`` per chunk -- the figure tools/search_bench.py
                 calls ``global_stage`` / ``global_ms``
  shared50_ms    (b) one 50 % mask for all queries (``dvlp_topk_rows_masked``, allow_ld = 0)
  perq50_ms      (c) one 50 % mask per query
  perq1_ms       (c) one 1 % mask per query
  where_ms       (d) the form the masked kernel replaces: ``torch.where(mask, sims, -inf)`` + ``dvlp_topk_rows`` per chunk (per-query 50 %
                 bool mask; its result still lists -inf rows with real ids when fewer than S are allowed)

    python tools/filtered_search_bench.py [--sizes 1000,100000,1000000] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demovlp_amd import ops  # noqa: E402
from demovlp_amd.search import VideoIndex  # noqa: E402

DEV = "cuda"
G, CHUNK = 240, 65536


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


def unit_rows(n, gen):
    x = torch.randn((n, 256), device=DEV, generator=gen)
    return x / x.norm(dim=1, keepdim=True)


def global_only_index(N, gen):
    ix = VideoIndex(N, G, torch.bfloat16, DEV)
    ix.gn, ix.n = unit_rows(N, gen), N            # the global stage reads nothing else
    return ix


def where_stage(ix, qn, S, allow):
    """the post-hoc form: -inf written into the cosine matrix of every chunk, then the unmasked top-k"""
    Nq = qn.shape[0]
    out = (torch.empty((Nq, S), device=DEV, dtype=torch.float32), torch.empty((Nq, S), device=DEV, dtype=torch.int32))
    minus = torch.full((), float("-inf"), device=DEV)
    for c0 in range(0, ix.n, CHUNK):
        cn = min(CHUNK, ix.n - c0)
        sims = ops.gemm(qn, ix.gn[c0:], Nq, cn, 256, dtype=ops.F32)
        ops.topk_rows(torch.where(allow[:, c0:c0 + cn], sims, minus), S, index_base=c0, out=out, merge=c0 > 0)
    ids, order = torch.sort(out[1], dim=1)
    return ids.contiguous(), torch.gather(out[0], 1, order).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    queries = {nq: unit_rows(nq, gen) for nq in (1, 1000)}
    for N in [int(s) for s in a.sizes.split(",") if s]:
        ix = global_only_index(N, gen)
        for nq, qn in queries.items():
            u = torch.rand((nq, N), device=DEV, generator=gen)
            half, one = u < 0.5, u < 0.01
            masks = dict(shared50=ops.pack_allow_bits(half[0]), perq50=ops.pack_allow_bits(half), perq1=ops.pack_allow_bits(one))
            del u, one
            for S in (50, 200):
                row = {"section": "filtered_global_stage", "N": N, "queries": nq, "shortlist": S}
                forms = [("none", lambda: ix._global_stage(qn, S, CHUNK))]
                forms += [(name, lambda m=m: ix._global_stage(qn, S, CHUNK, m)) for name, m in masks.items()]
                forms += [("where", lambda: where_stage(ix, qn, S, half))]
                for name, fn in forms:
                    med, lo, hi = ms(fn, a.reps)
                    row[name + "_ms"], row[name + "_spread"] = round(med, 3), [round(lo, 3), round(hi, 3)]
                print(json.dumps(row), flush=True)
            del half, masks
        del ix


if __name__ == "__main__":
    main()
