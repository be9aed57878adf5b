"""QA answer head: stock PyTorch-ROCm kernels against the HIP head (csrc/qahead.hip), one JSON line.

    python tools/qa_head_bench.py                       # head + loss forward+backward alone, and one whole train_step_qa, each with both heads
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/qa_head_bench.py --launch-loop hip --iters 10
                                                        # a bare loop of head forward+backward for counting launches: run it with two values
                                                        # of --iters and divide the difference of the kernel counts by the difference of iters

Shapes: B = 64, F = 8, R = 30 (G = 240), num_label = 1500, bf16 towers (configs/ft/msrvtt_qa-select.json).  Timing: warm-up, then hip events
around each of ``--reps`` iterations, median reported (with min and max).  The head alone is fed detached bf16 embeddings of the model's own
towers, in train mode (dropout 0.2 on), gradients to the embeddings and to the head's parameters.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from demovlp_amd import functional as Fn, synthetic as syn  # noqa: E402
from demovlp_amd.loss import CrossEntropy  # noqa: E402
from demovlp_amd.model import ObjectQARelation  # noqa: E402
from demovlp_amd.trainer import FusedAdamW, ParamArena, train_step_qa  # noqa: E402

DEV = "cuda"
B, F, R, NL = 64, 8, 30, 1500


def build(impl):
    m = ObjectQARelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None, "num_label": NL},
                         {"model": "pretrained/distilbert-base-uncased", "pretrained": True, "input": "text", "two_outputs": True},
                         pretrained_init=False, compute_dtype="bfloat16", head_impl=impl)
    sd = syn.fill_state_dict(F, R, None, NL)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to(DEV).train()


def batch():
    obj, mask = syn.fast_region_batch(B, F, R)
    ids, att = syn.caption_batch(B)
    t = lambda a: torch.from_numpy(a).to(DEV)
    label = torch.from_numpy(np.random.default_rng(0).integers(0, NL, B)).to(DEV)
    return {"text": {"input_ids": t(ids), "attention_mask": t(att)}, "object": t(obj), "object_mask": t(mask), "label": label}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)))


def head_loop(m, impl, data):
    """fn() = head + loss forward and backward on fixed embeddings of the model's own towers."""
    with torch.no_grad():
        h, hr = m.text_model(input_ids=data["text"]["input_ids"], attention_mask=data["text"]["attention_mask"], want_relu=True)
        lin = m.txt_proj[1]
        te = Fn.LinearFn.apply(hr, lin.weight, lin.bias, h)
        oe, _ = m.object_model(data["object"], data["object_mask"])
    te, oe = te.detach().requires_grad_(True), oe.detach().requires_grad_(True)
    loss_fn = CrossEntropy(impl=impl)
    params = list(m.head.parameters())

    def fn():
        te.grad = oe.grad = None
        for p in params:
            p.grad = None
        logits = m.compute_fusion(te, oe, data["text"]["attention_mask"], data["object_mask"])
        loss_fn(logits, data["label"]).backward()
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--launch-loop", choices=["stock", "hip"], default=None)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    data = batch()
    if args.launch_loop:
        fn = head_loop(build(args.launch_loop), args.launch_loop, data)
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(dict(launch_loop=args.launch_loop, iters=args.iters)))
        return
    out = dict(config=dict(B=B, F=F, R=R, G=F * R, num_label=NL, dtype="bfloat16", warmup=args.warmup, reps=args.reps))
    for impl in ("stock", "hip"):
        m = build(impl)
        out[f"head_fwd_bwd_{impl}"] = timed(head_loop(m, impl, data), args.warmup, args.reps)
        arena = ParamArena(m, bf16_shadow=True)
        opt = FusedAdamW(arena, lr=1e-4)
        loss_fn = CrossEntropy(impl=impl)
        out[f"train_step_qa_{impl}"] = timed(lambda: train_step_qa(m, loss_fn, opt, data), args.warmup, args.reps)
        del m, arena, opt
    out["hip_not_slower"] = bool(out["head_fwd_bwd_hip"]["median_ms"] <= out["head_fwd_bwd_stock"]["median_ms"]
                                 and out["train_step_qa_hip"]["median_ms"] <= out["train_step_qa_stock"]["median_ms"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
