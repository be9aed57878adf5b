"""Multiple-choice evaluation throughput on an MSRVTT-MC-sized pass (2990 questions, K = 5 options, F = 8, R = 30, W = 99, bf16,
synthetic retrieval weights).  Prints ONE JSON line:

  eval_mc_q64_qps      trainer.evaluate_mc with 64 questions per batch (object tower once per clip, pair-list local kernel)
  ref_loop_qps         the reference's loop shape (trainer/trainer_dist.py:796-829): one question per batch, the clip expanded to K copies
                       through the object tower, a K x K get_sim, row 0 read
  pairs_us / grid_us   the local term alone for 64 questions: the pair-list kernel (Q K pairs) against one full-grid fused launch over the
                       same Q K captions (Q x Q K pairs), microseconds per call

    python tools/mc_eval_bench.py [--questions 2990] [--ref-questions 300]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demovlp_amd import ops, synthetic as syn  # noqa: E402
from demovlp_amd.loss import GlobalLocalLoss  # noqa: E402
from demovlp_amd.model import ObjectMCRelation, sim_matrix  # noqa: E402
from demovlp_amd.trainer import evaluate_mc  # noqa: E402

DEV = "cuda"
F, R, K = 8, 30, 5


def batches(mc, n_total, Q):
    """n_total questions in batches of Q, cycling through the generated set (the inputs only need realistic shapes)."""
    n = mc["options"].shape[0]
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in mc.items() if k != "mc_ids"}
    out = []
    for q0 in range(0, n_total, Q):
        q1 = min(n_total, q0 + Q)
        idx = torch.arange(q0, q1, device=DEV) % n
        rows = (idx[:, None] * K + torch.arange(K, device=DEV)).reshape(-1)
        out.append({"text": {"input_ids": dev["input_ids"][rows], "attention_mask": dev["attention_mask"][rows]},
                    "object": dev["object"][idx].contiguous(), "object_mask": dev["object_mask"][idx].contiguous(),
                    "mc_id": list(range(q0, q1))})
    return out


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=2990)
    ap.add_argument("--ref-questions", type=int, default=300)
    ap.add_argument("--q", type=int, default=64)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    sd = syn.retrieval_state_dict(F, R)
    model = ObjectMCRelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None},
                             {"model": "", "pretrained": True, "input": "text", "two_outputs": True}, pretrained_init=False,
                             compute_dtype="bfloat16")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model.set_text_dropout(0.0)
    model.to(DEV).eval()
    loss = GlobalLocalLoss(use_local=True, use_global=True, coef=1.0, focal_type="equal")
    mc = syn.mc_questions(sd, F, R, 0, 64, K)
    gt = {q: int(mc["answers"][q % 64]) for q in range(a.questions)}

    bq = batches(mc, a.questions, a.q)
    evaluate_mc(model, loss, bq[:2], gt)                                   # warm-up (allocator, first launches)
    t_eval = timed(lambda: evaluate_mc(model, loss, bq, gt))

    b1 = batches(mc, a.ref_questions, 1)

    def ref_loop():
        with torch.no_grad():
            for d in b1:
                att = d["text"]["attention_mask"]
                text_length = torch.sum(att, dim=1)
                text_mask = (att[:, 1:] - 1.0) * 100.0
                e = {"text": d["text"], "object": d["object"].expand(K, -1, -1, -1), "object_mask": d["object_mask"].expand(K, -1, -1)}
                o = model(e, return_embeds=True)
                s = sim_matrix(o["global_text_embeddings"], o["global_object_embeddings"]) + \
                    loss.local_loss.get_sim(o["local_object_embeddings"], o["local_text_embeddings"], o["object_mask"], text_length, text_mask)
                int(s[0].argmax())
    with torch.no_grad():
        ref_loop()                                                           # warm-up
    t_ref = timed(ref_loop)

    # the local term alone, 64 questions: pair list vs full grid over the same captions
    d = bq[0]
    with torch.no_grad():
        o = model(d, return_embeds=True)
    C, Qe = o["local_object_embeddings"].contiguous(), o["local_text_embeddings"].contiguous()
    mi = o["object_mask"].float().contiguous()
    mcap = ((d["text"]["attention_mask"][:, 1:] - 1.0) * 100.0).float().contiguous()
    pairs = lambda: ops.xattn_pairs_fwd(C, Qe, mi, mcap, None, K, 20.0, True)
    grid = lambda: ops.xattn_fwd(C, Qe, mi, mcap, 20.0, True, False)
    for f in (pairs, grid):
        f()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def us(f, n=50):
        ts = []
        for _ in range(n):
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
        return float(np.median(ts))

    print(json.dumps({"questions": a.questions, "K": K, "F": F, "R": R, "W": int(mcap.shape[1]), "dtype": "bf16",
                      "eval_mc_q64_qps": round(a.questions / t_eval, 1), "ref_loop_qps": round(a.ref_questions / t_ref, 1),
                      "ref_loop_questions_timed": a.ref_questions, "pairs_us": round(us(pairs), 1), "grid_us": round(us(grid), 1),
                      "local_Q": int(C.shape[0])}))


if __name__ == "__main__":
    main()
