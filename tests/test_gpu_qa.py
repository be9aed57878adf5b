"""Video-QA answer head on the device: the kernels of csrc/qahead.hip one by one against float64 restatements
on the host (tests/qa_ref.py), ``BUTDQAHead(impl="hip")`` against golden G10 and against the float64 head, ``trainer.train_step_qa`` /
``trainer.evaluate_qa`` against the reference's own QA loop (golden G16).

Bars.  fp32: 1e-4 of each tensor's max (the project's fp32 gradient bar, README round 6), G10's own bars for the G10 comparison, 1e-3 abs
for the loss curve (README round 5).  bf16 kernels fed the SAME bf16-rounded inputs as the float64 restatement: W_v is rounded to bf16 (unit
round-off 2^-9 per element) and dv / dH are stored in bf16 (2^-9 again); the attention logits are O(1) sums, so an absolute logit error e
becomes a relative softmax error e.  Eight round-offs, 8 x 2^-9 = 1.6e-2, rounded to 2e-2 of each tensor's max."""
import numpy as np
import pytest
import torch

import qa_ref
from demovlp_amd import DemoVLPHipError, functional as Fn, metric, ops, synthetic as syn
from demovlp_amd.loss import CrossEntropy
from demovlp_amd.model import ObjectQARelation
from demovlp_amd.trainer import FusedAdamW, ParamArena, evaluate_qa, train_step_qa
from demovlp_amd.video_qa_model import BUTDQAHead
from helpers import golden_batch, load_golden, rel_err
from oracle import restatement as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP32_BAR, BF16_BAR = 1e-4, 2e-2


def close(got, want, bar, what=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))
    print(f"{what}: rel-to-max err {err:.3e} (bar {bar:.0e})")
    assert got.shape == want.shape and err < bar, (what, err)


def head_weights(seed, num_label=50):
    """head.* tensors as float64 leaves (values of synthetic.fill_state_dict, perturbed per seed so that g != |V|)."""
    sd = {k: v for k, v in syn.fill_state_dict(8, 30, None, num_label).items() if k.startswith("head.")}
    rng = np.random.default_rng(seed)
    p = {}
    for k, v in sd.items():
        a = np.asarray(v, np.float64) * (1.0 + 0.1 * rng.standard_normal(np.shape(v)))
        p[k] = torch.tensor(a.astype(np.float32).astype(np.float64), requires_grad=True)
    return p


def stable_relu_gates(p, v):
    """ReLU'(0) is a jump: an element of H = v W_v^T + b_v closer to zero than the rounding error of H (fp32 ~1e-6 of max|H|, with a bf16
    W_v ~1e-2) takes either gate, in ANY finite-precision implementation, and each flip moves dH by a whole element -- with 3.9 M elements at
    B = 64, G = 240 a float64 comparison at 1e-4 would be decided by that, not by the kernel.  So the kernel-level comparison keeps H away from
    the kink: b_v = +-8 sigma (sigma = std of v W_v^T in float64, sign drawn per channel), half the channels open and half shut.  The gates that
    depend on the data are covered by TestHeadEndToEnd.test_head_gradients_elementwise_vs_float64 (the head's own biases)."""
    n = qa_ref.WN[0]
    with torch.no_grad():
        sigma = float((v.double() @ qa_ref.fold(p[n + ".weight_v"], p[n + ".weight_g"]).t()).std())
        sign = torch.from_numpy(np.random.default_rng(17).integers(0, 2, 256) * 2.0 - 1.0)
        p[n + ".bias"].copy_((8.0 * sigma * sign).float().double())


def attend_inputs(B, G, seed, dtype, zero_mask_sample=True):
    rng = np.random.default_rng(seed)
    v = torch.from_numpy(rng.standard_normal((B, G, 256)).astype(np.float32)).to(dtype).float()
    q = torch.from_numpy(rng.standard_normal((B, 256)).astype(np.float32))
    mask = torch.from_numpy((rng.random((B, G)) > 0.2).astype(np.float32))
    if zero_mask_sample:
        mask[B - 1] = 0.0                                      # a sample whose every region is padding: uniform attention
    return v, mask, q


class TestWeightNormFold:
    def test_forward_and_backward_of_five_tensors_in_one_launch(self):
        rng = np.random.default_rng(0)
        shapes = [(256, 256), (256, 256), (1, 256), (256, 256), (256, 256)]
        vs = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in shapes]
        gs = [torch.tensor(float(rng.random() + 0.5)) for _ in shapes]
        dW = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in shapes]
        leaves = [t.to(DEV).requires_grad_(True) for pair in zip(vs, gs) for t in pair]
        out = Fn.WeightNormFoldFn.apply((0,), *leaves)
        assert len(out) == 6 and out[5].dtype == torch.bfloat16
        torch.autograd.backward(out[:5], [d.to(DEV) for d in dW])
        for i, (v, g, d) in enumerate(zip(vs, gs, dW)):
            v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
            w = qa_ref.fold(v64, g64)
            w.backward(d.double())
            close(out[i], w, 1e-6, f"W{i}")
            close(leaves[2 * i].grad, v64.grad, FP32_BAR, f"dV{i}")
            close(leaves[2 * i + 1].grad, g64.grad, FP32_BAR, f"dg{i}")
        assert torch.equal(out[5], out[0].to(torch.bfloat16))
        again = Fn.WeightNormFoldFn.apply((0,), *leaves)
        assert all(torch.equal(a, b) for a, b in zip(out, again))


class TestTokenMax:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_forward_backward_with_ties(self, dtype):
        rng = np.random.default_rng(1)
        x = torch.from_numpy(rng.standard_normal((5, 100, 256)).astype(np.float32)).to(dtype)
        x[0, 7, :] = 9.0
        x[0, 93, :] = 9.0                                      # a tie: the first index wins, as torch.max on the CPU gives
        x[1, :, 3] = -2.0                                      # a whole column tied
        xg = x.to(DEV).requires_grad_(True)
        out = Fn.TokenMaxFn.apply(xg)
        dout = torch.from_numpy(rng.standard_normal((5, 256)).astype(np.float32))
        out.backward(dout.to(DEV))
        ref = x.float().max(dim=1)[0]
        assert out.dtype == torch.float32 and torch.equal(out.cpu(), ref)
        first = (x.float() == ref[:, None]).float().argmax(dim=1)                    # first maximal token
        want = torch.zeros(5, 100, 256)
        want.scatter_(1, first[:, None], dout[:, None])
        assert xg.grad.dtype == dtype and torch.equal(xg.grad.float().cpu(), want.to(dtype).float())
        assert float(xg.grad[0, 7].float().abs().sum()) > 0 and float(xg.grad[0, 93].float().abs().sum()) == 0


def run_attend(v, mask, q, p, dtype, drop=None):
    """QAAttendFn on the device with the folded weights of ``p`` -> (pooled, att, grads dict)."""
    W = {n: qa_ref.fold(p[n + ".weight_v"], p[n + ".weight_g"]).detach().float().to(DEV).requires_grad_(True) for n in qa_ref.WN[:3]}
    b = {n: p[n + ".bias"].detach().float().to(DEV).requires_grad_(True) for n in qa_ref.WN[:3]}
    vg = v.to(dtype).to(DEV).requires_grad_(True)
    qg = q.to(DEV).requires_grad_(True)
    Wv_b = W[qa_ref.WN[0]].detach().to(torch.bfloat16) if dtype == torch.bfloat16 else None
    pooled, att = Fn.QAAttendFn.apply(vg, mask.to(DEV), qg, W[qa_ref.WN[1]], b[qa_ref.WN[1]], W[qa_ref.WN[0]], Wv_b, b[qa_ref.WN[0]],
                                      W[qa_ref.WN[2]], b[qa_ref.WN[2]], drop)
    return pooled, att, dict(v=vg, q=qg, Wq=W[qa_ref.WN[1]], bq=b[qa_ref.WN[1]], Wv=W[qa_ref.WN[0]], bv=b[qa_ref.WN[0]], wl=W[qa_ref.WN[2]],
                             bl=b[qa_ref.WN[2]])


def ref_attend(v, mask, q, p, ks=None):
    t = {n: qa_ref.fold(p[n + ".weight_v"], p[n + ".weight_g"]).detach().float().double().requires_grad_(True) for n in qa_ref.WN[:3]}
    b = {n: p[n + ".bias"].detach().clone().requires_grad_(True) for n in qa_ref.WN[:3]}
    v64, q64 = v.double().requires_grad_(True), q.double().requires_grad_(True)
    pooled, att = qa_ref.attend(v64, mask.double(), q64, t[qa_ref.WN[1]], b[qa_ref.WN[1]], t[qa_ref.WN[0]], b[qa_ref.WN[0]], t[qa_ref.WN[2]],
                                b[qa_ref.WN[2]], ks)
    return pooled, att, dict(v=v64, q=q64, Wq=t[qa_ref.WN[1]], bq=b[qa_ref.WN[1]], Wv=t[qa_ref.WN[0]], bv=b[qa_ref.WN[0]], wl=t[qa_ref.WN[2]],
                             bl=b[qa_ref.WN[2]])


class TestAttend:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("B,G", [(64, 240), (5, 288), (1, 1152), (5, 1), (5, 37), (1, 240)])
    @pytest.mark.parametrize("train", [False, True])
    def test_forward_backward_vs_float64(self, B, G, dtype, train):
        """eval and train mode (keep mask pinned against orc.dropout_keep_flat at ops.QA_HEAD_DROPOUT_SITE), both dtypes, the fused route
        (bf16, G <= 288) and the general one, one sample with an all-zero mask."""
        p = head_weights(3)
        v, mask, q = attend_inputs(B, G, 100 + B + G, dtype)
        v = v * 0.25                                           # logits of order 1
        stable_relu_gates(p, v)
        drop, ks = None, None
        if train:
            seed, prob = 1234567891011, 0.2
            state = ops.dropout_state(torch.device(DEV), seed)
            ops.dropout_advance(state)
            ops.dropout_advance(state)                         # offset 2
            drop = (prob, state, ops.QA_HEAD_DROPOUT_SITE)
            ks = qa_ref.keep_scale(B, G, prob, seed, 2, ops.QA_HEAD_DROPOUT_SITE)
        pooled, att, g = run_attend(v, mask, q, p, dtype, drop)
        if train:
            ops.dropout_advance(state)                         # the backward must use the forward's snapshot, not the live state
        rng = np.random.default_rng(G)
        dp = torch.from_numpy(rng.standard_normal((B, 256)).astype(np.float32))
        pooled.backward(dp.to(DEV))
        rp, ratt, r = ref_attend(v, mask, q, p, ks)
        rp.backward(dp.double())
        bar = FP32_BAR if dtype == torch.float32 else BF16_BAR
        close(att, ratt, bar, "att")
        close(pooled, rp, bar, "pooled")
        assert abs(float(att[B - 1].sum()) - 1.0) < 1e-5 and float((att[B - 1] - 1.0 / G).abs().max()) < 1e-6      # all-zero mask: uniform
        for k in g:
            close(g[k].grad, r[k].grad, bar, "d" + k)
        assert g["v"].grad.dtype == dtype

    def test_strided_view_equals_contiguous_copy_bit_for_bit_and_runs_are_reproducible(self):
        """QAAttendFn on ``full[:, 1:]`` against the same call on a contiguous copy: everything whose arithmetic does not depend on the row layout
        -- pooled, att, dv, dq, dWq, dbq, dbv, dwl, dbl -- bit for bit.  dWv = dH^T v is a dvlp_gemm reduction over the storage rows,
        (B - 1)(G + 1) + G of them for the view (B - 1 zero rows in between) and B G for the copy: the K extent differs, so the product's split of
        K may differ and the sums are only compared at the fp32 / bf16 bar (the measured difference is printed)."""
        p = head_weights(4)
        B, G = 6, 240
        for dtype in (torch.bfloat16, torch.float32):
            rng = np.random.default_rng(8)
            full = torch.from_numpy(rng.standard_normal((B, G + 1, 256)).astype(np.float32)).to(dtype).to(DEV)
            _, mask, q = attend_inputs(B, G, 9, dtype)
            outs = []
            for v in (full[:, 1:], full[:, 1:].contiguous(), full[:, 1:]):
                assert v.shape == (B, G, 256)
                pooled, att, g = run_attend(v, mask, q, p, dtype)
                pooled.sum().backward()
                outs.append(dict(pooled=pooled, att=att, **{"d" + k: t.grad for k, t in g.items()}))
            assert not full[:, 1:].is_contiguous()
            for k in outs[0]:
                assert torch.equal(outs[0][k], outs[2][k]), k                      # two runs of the same call: every output bit-equal
                if k != "dWv":
                    assert torch.equal(outs[0][k], outs[1][k]), k                  # the view against the copy
            same = torch.equal(outs[0]["dWv"], outs[1]["dWv"])
            print(f"{dtype}: dWv of the strided view bit-equal to the contiguous copy's: {same}")
            close(outs[0]["dWv"], outs[1]["dWv"], FP32_BAR if dtype == torch.float32 else BF16_BAR, "dWv view vs copy")

    @pytest.mark.parametrize("train", [False, True])
    def test_bf16_fused_route_with_data_dependent_gates(self, train):
        """The fused MFMA route (forward and recompute backward) with the head's OWN biases, so every ReLU gate depends on the data.  An element
        of H whose float64 value is smaller than the bf16 rounding of H may take either gate (stable_relu_gates explains); the rounding bound is
        2^-8 sum_k |v_k| |W_nk| (2^-9 per rounded weight, doubled for the accumulation).  dH is compared element-wise on all other elements,
        and they must be nearly all of them; att / pooled are compared as usual."""
        B, G, dtype = 64, 240, torch.bfloat16
        p = head_weights(6)
        v, mask, q = attend_inputs(B, G, 31, dtype, zero_mask_sample=False)
        v = v * 0.25
        n = qa_ref.WN
        W = {k: qa_ref.fold(p[k + ".weight_v"], p[k + ".weight_g"]).detach().float() for k in n[:3]}
        bias = {k: p[k + ".bias"].detach().float() for k in n[:3]}
        d = lambda t: t.to(DEV).contiguous()
        drop, ks, prob = None, None, 0.0
        if train:
            seed, prob = 77, 0.2
            state = ops.dropout_state(torch.device(DEV), seed)
            ops.dropout_advance(state)
            drop = (prob, state, ops.QA_HEAD_DROPOUT_SITE)
            ks = qa_ref.keep_scale(B, G, prob, seed, 1, ops.QA_HEAD_DROPOUT_SITE)
        vd, md, qd = d(v.to(dtype)), d(mask), d(q)
        Wv_b = d(W[n[0]]).to(dtype)
        assert ops.qa_attend_fused(dtype, G)
        qp, att, pooled, snap = ops.qa_attend_fwd(vd, G, md, qd, d(W[n[1]]), d(bias[n[1]]), Wv_b, d(bias[n[0]]), d(W[n[2]]), d(bias[n[2]]), None, drop)
        dp = torch.from_numpy(np.random.default_rng(5).standard_normal((B, 256)).astype(np.float32))
        _, dH, *_ = ops.qa_attend_bwd(vd, G, md, qd, d(W[n[1]]), Wv_b, d(bias[n[0]]), d(W[n[2]]), None, prob, snap, ops.QA_HEAD_DROPOUT_SITE if train else 0,
                                      qp, att, d(dp))
        v64 = v.double()
        Wv64 = W[n[0]].double()
        H64 = (v64 @ Wv64.t() + bias[n[0]].double()).requires_grad_(True)
        qp64 = torch.relu(q.double() @ W[n[1]].double().t() + bias[n[1]].double())
        z = torch.relu(H64) * qp64[:, None]
        if ks is not None:
            z = z * ks
        logit = (z @ W[n[2]].double().reshape(-1) + bias[n[2]].double().reshape(())) * mask.double()
        a64 = torch.softmax(logit, 1)
        p64 = (a64[..., None] * v64).sum(1)
        p64.backward(dp.double())
        close(att, a64, BF16_BAR, "att")
        close(pooled, p64, BF16_BAR, "pooled")
        tol = 2.0 ** -8 * (v64.abs() @ Wv64.abs().t())
        sure = H64.detach().abs() > tol
        frac = float(sure.double().mean())
        open_frac = float((H64.detach() > 0).double().mean())
        got, want = dH.view(B, G, 256).double().cpu(), H64.grad
        err = float(((got - want).abs() * sure).max() / want.abs().max())
        print(f"gates open {open_frac:.3f}; compared {frac:.4f} of the elements; dH rel-to-max err {err:.3e} (bar {BF16_BAR:.0e})")
        assert 0.2 < open_frac < 0.8 and frac > 0.95 and err < BF16_BAR


class TestSoftmaxXent:
    @pytest.mark.parametrize("C", [2, 50, 1500, 1541])
    def test_loss_gradient_and_prediction(self, C):
        rng = np.random.default_rng(C)
        B = 7
        x = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32) * 3)
        x[2, C // 2] = 3.0e4                                   # one huge logit
        x[3, 1] = x[3, 0] = 50.0                               # a tie for the arg-max: first index
        y = torch.from_numpy(rng.integers(0, C, B))
        y[2] = 0
        xg = x.to(DEV).requires_grad_(True)
        crit = CrossEntropy(impl="hip")
        loss = crit(xg, y.to(DEV))
        (loss * 2.0).backward()
        x64 = x.double().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(x64, y)
        (ref * 2.0).backward()
        assert abs(loss.item() - ref.item()) < 1e-5 * max(1.0, abs(ref.item()))
        close(xg.grad, x64.grad, FP32_BAR, "dlogits")
        assert torch.equal(crit.last_pred.cpu().long(), x.max(dim=-1)[1]) and int(crit.last_pred[3]) == 0
        assert bool(torch.isfinite(xg.grad).all())

    def test_bad_labels_raise(self):
        x = torch.zeros(4, 10, device=DEV)
        with pytest.raises(DemoVLPHipError):
            CrossEntropy(impl="hip")(x, torch.zeros(4, device=DEV))                  # float labels
        with pytest.raises(DemoVLPHipError):
            CrossEntropy(impl="hip")(x, torch.zeros(3, dtype=torch.int64, device=DEV))


def qa_model(F, R, NL, sd, impl, dtype="float32"):
    m = ObjectQARelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None, "num_label": NL},
                         {"model": "pretrained/distilbert-base-uncased", "pretrained": True, "input": "text", "two_outputs": True},
                         pretrained_init=False, compute_dtype=dtype, head_impl=impl)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV)


def to_data(obj, mask, ids, att):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return {"text": {"input_ids": t(ids), "attention_mask": t(att)}, "object": t(obj), "object_mask": t(mask)}


class TestHeadEndToEnd:
    def test_hip_head_vs_reference_golden_g10(self):
        """The bars of tests/test_gpu_round2.py::test_qa_model_vs_reference_golden, with head_impl='hip' and CrossEntropy(impl='hip')."""
        g = load_golden("g10_qa.npz")
        F, R, B, NL = int(g["F"]), int(g["R"]), int(g["B"]), int(g["num_label"])
        m = qa_model(F, R, NL, syn.fill_state_dict(F, R, None, NL), "hip").eval()
        logits = m(to_data(*golden_batch(F, R, B)))["logits"]
        assert logits.shape == (B, NL) and rel_err(logits.detach().cpu().numpy(), g["logits"]) < 1e-4
        loss = CrossEntropy(impl="hip")(logits, torch.from_numpy(g["label"]).to(DEV))
        assert abs(loss.item() - g["loss"][0]) < 1e-4
        loss.backward()
        named = dict(m.named_parameters())
        bad = [(k, float(named[k].grad.double().norm()), n) for k, n in zip(g["grad_names"], g["grad_norms"])
               if abs(float(named[k].grad.double().norm()) - n) > 2e-3 * max(n, 1e-6)]
        assert not bad, bad[:5]
        for k in g.files:
            if k.startswith("grad/"):
                close(named[k[5:]].grad.reshape(g[k].shape), torch.from_numpy(g[k]), 2e-3, k)

    @pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
    def test_model_head_reads_the_strided_view_like_a_contiguous_copy(self, dtype):
        """BUTDQAHead(impl='hip') as ObjectQARelation calls it: ``object_embeddings[:, 1:]`` (strided) against a contiguous copy of it -- logits and
        the gradient handed back to the embeddings bit for bit; two runs of the strided call are bit-equal in every gradient."""
        torch.manual_seed(0)
        head = BUTDQAHead(256, 256, 256, 50, impl="hip").to(DEV).eval()
        cd = torch.bfloat16 if dtype == "bfloat16" else torch.float32
        rng = np.random.default_rng(12)
        B, G = 5, 240
        emb = torch.from_numpy(rng.standard_normal((B, G + 1, 256)).astype(np.float32) * 0.25).to(cd).to(DEV)
        q = torch.from_numpy(rng.standard_normal((B, 256)).astype(np.float32)).to(DEV)
        mask = torch.from_numpy((rng.random((B, G)) > 0.2).astype(np.float32)).to(DEV)
        y = torch.from_numpy(rng.integers(0, 50, B)).to(DEV)
        runs = []
        for make in (lambda e: e[:, 1:], lambda e: e[:, 1:].contiguous(), lambda e: e[:, 1:]):
            e = emb.clone().requires_grad_(True)
            head.zero_grad()
            logits = head(q, make(e), mask)
            CrossEntropy(impl="hip")(logits, y).backward()
            runs.append((logits.detach(), e.grad, {k: t.grad.clone() for k, t in head.named_parameters()}))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        assert torch.equal(runs[0][0], runs[2][0]) and torch.equal(runs[0][1], runs[2][1])
        assert all(torch.equal(runs[0][2][k], runs[2][2][k]) for k in runs[0][2])

    @pytest.mark.parametrize("train", [False, True])
    def test_head_gradients_elementwise_vs_float64(self, train):
        p = head_weights(5)
        B, G = 5, 240
        v, mask, q = attend_inputs(B, G, 77, torch.float32, zero_mask_sample=False)
        v = v * 0.25
        head = BUTDQAHead(256, 256, 256, 50, impl="hip")
        head.load_state_dict({k[5:]: t.detach().float() for k, t in p.items()})
        head.to(DEV).train(train)
        ks = None
        if train:
            head.seed_dropout(99)
            ks = qa_ref.keep_scale(B, G, 0.2, 99, 1, ops.QA_HEAD_DROPOUT_SITE)            # the first train-mode forward runs at offset 1
        y = torch.from_numpy(np.random.default_rng(2).integers(0, 50, B))
        vg, qg = v.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
        logits = head(qg, vg, mask.to(DEV))
        CrossEntropy(impl="hip")(logits, y.to(DEV)).backward()
        v64, q64 = v.double().requires_grad_(True), q.double().requires_grad_(True)
        ref = qa_ref.head_logits(p, q64, v64, mask.double(), ks)
        torch.nn.functional.cross_entropy(ref, y).backward()
        assert rel_err(logits.detach().cpu().numpy(), ref.detach().numpy()) < 1e-4
        close(vg.grad, v64.grad, FP32_BAR, "dv")
        close(qg.grad, q64.grad, FP32_BAR, "dq")
        for k, t in head.named_parameters():
            close(t.grad, p["head." + k].grad, FP32_BAR, k)

    def test_bf16_model_vs_float64_and_vs_stock_head(self):
        """compute_dtype='bfloat16': logits and head gradients of the whole model against the float64 restatement (orc.qa_logits) fed the
        same weights; the stock head on the same bf16 towers is the yardstick -- the HIP head must not be more than 2x farther from float64.
        Measured on the MI355X: logits 3.084e-3 of max|logit|, worst head gradient 2.387e-1 of its tensor's max (stock head:
        3.075e-3, 2.387e-1); bars 6.2e-3 and 4.8e-1 = 2 x measured (BF16_MODEL_MEASURED / BF16_MODEL_BAR below).  The worst tensor, with either
        head, is head.classifier.main.0.bias (main.0.weight next, 2.1e-1): a sum over B = 4 samples behind 512 ReLU gates, some of which the bf16
        towers' error flips; every other head tensor is within 1e-1.  The gradient half therefore guards the hip <= 2 x stock relation; the fused
        bf16 route itself is pinned by TestAttend.test_bf16_fused_route_with_data_dependent_gates."""
        F, R, B, NL = 8, 30, 4, 50
        sd = syn.fill_state_dict(F, R, None, NL)
        obj, mask, ids, att = golden_batch(F, R, B)
        y = torch.tensor([3, 17, 0, 42])
        p = orc.params_from_numpy(sd, requires_grad=True)
        ref = orc.qa_logits(p, torch.from_numpy(ids), torch.from_numpy(att), torch.from_numpy(obj), torch.from_numpy(mask))
        torch.nn.functional.cross_entropy(ref, y).backward()
        dev = {}
        for impl in ("stock", "hip"):
            m = qa_model(F, R, NL, sd, impl, "bfloat16").eval()
            logits = m(to_data(obj, mask, ids, att))["logits"]
            CrossEntropy(impl=impl)(logits.float(), y.to(DEV)).backward()
            named = dict(m.named_parameters())
            e_logit = float((logits.detach().double().cpu() - ref.detach()).abs().max() / ref.detach().abs().max())
            per = {k: float((named[k].grad.double().cpu() - p[k].grad).abs().max() / p[k].grad.abs().max()) for k in named if k.startswith("head.")}
            worst = max(per, key=per.get)
            e_grad = per[worst]
            print(f"bf16 {impl}: worst head tensor {worst} (max |grad| {float(p[worst].grad.abs().max()):.3e}); " +
                  ", ".join(f"{k[5:]} {e:.2e}" for k, e in sorted(per.items())))
            dev[impl] = (e_logit, e_grad)
            print(f"bf16 {impl}: logits rel-to-max {e_logit:.3e}, worst head gradient rel-to-max {e_grad:.3e}")
        assert dev["hip"][0] <= 2 * dev["stock"][0] and dev["hip"][1] <= 2 * dev["stock"][1], dev
        assert dev["hip"][0] < BF16_MODEL_BAR[0] and dev["hip"][1] < BF16_MODEL_BAR[1], dev


# measured deviation of the bf16 model with the HIP head from float64 (logits, worst head gradient; relative to each tensor's max), and the bar
# = 2 x measured.  Filled in from the MI355X run recorded in DESIGN.md.
BF16_MODEL_MEASURED = (3.084e-3, 2.387e-1)       # (the stock head on the same bf16 towers: 3.075e-3, 2.387e-1 -- the towers' bf16 dominates both)
BF16_MODEL_BAR = (6.2e-3, 4.8e-1)


def g16_setup(impl):
    g = load_golden("g16_qa_finetune.npz")
    F, R, NL = int(g["F"]), int(g["R"]), int(g["num_label"])
    sd = syn.retrieval_state_dict(F, R)
    sd.update({k: v for k, v in syn.fill_state_dict(F, R, None, NL).items() if k.startswith("head.")})
    m = qa_model(F, R, NL, sd, impl)
    return g, m, syn.retrieval_state_dict(F, R), (F, R, NL)


class TestTrainAndEvaluateVsG16:
    @pytest.mark.parametrize("impl", ["hip", "stock"])
    def test_train_step_qa_follows_the_reference_curve_then_evaluate_qa_matches(self, impl):
        """fp32, dropout off (eval mode while gradients flow, as the fixture): loss curve within 1e-3 abs, correct counts on steps where every
        recorded margin clears the threshold; then the 64 validation questions: logits rel_err < 1e-4, predictions equal wherever the recorded
        top-2 margin exceeds 10 x 1e-4 x max|logit| (at most 3 of 64 may fall below), metric dict over the compared questions equal."""
        g, m, rsd, (F, R, NL) = g16_setup(impl)
        m.eval()
        arena = ParamArena(m)
        opt = FusedAdamW(arena, lr=float(g["lr"]))
        loss_fn = CrossEntropy(impl=impl)
        K, B = int(g["steps"]), int(g["B"])
        train = syn.qa_questions(rsd, F, R, 0, K * B, NL)
        assert np.array_equal(train["label"], g["train_label"])
        before = {k: t.detach().clone() for k, t in m.named_parameters()}
        thr_of = lambda logits_max: 10 * 1e-4 * logits_max
        thr = thr_of(float(np.abs(g["val_logits"]).max()))
        for s, data in enumerate(syn.qa_batches(train, B, DEV)):
            loss, n_correct = train_step_qa(m, loss_fn, opt, data)
            print(f"step {s}: loss {loss.item():.6f} (G16 {g['losses'][s]:.6f}), correct {int(n_correct)} (G16 {int(g['correct'][s])})")
            assert abs(loss.item() - g["losses"][s]) < 1e-3
            if g["train_margin"][s].min() > thr:
                assert int(n_correct) == int(g["correct"][s])
        moved = [k for k, t in m.named_parameters() if not torch.equal(t.detach(), before[k])]
        assert any(k.startswith("head.") for k in moved) and any(k.startswith("object_model.") for k in moved) and any(k.startswith("text_model.") for k in moved)
        assert all(k in moved for k in before if k.startswith("head."))
        val = syn.qa_questions(rsd, F, R, int(g["val_first"]), int(g["val_n"]), NL)
        m.train()
        r = evaluate_qa(m, syn.qa_batches(val, int(g["val_b"]), DEV), val["label2ans"], val["qid2data"])
        assert m.training                                     # the previous mode is restored
        assert np.array_equal(r["question_ids"], val["question_id"])
        err = rel_err(r["logits"], g["val_logits"])
        print(f"evaluate_qa logits rel_err {err:.3e}")
        assert err < 1e-4
        sure = g["val_margin"] > thr
        assert (~sure).sum() <= 3
        assert np.array_equal(r["preds"][sure], g["val_preds"][sure])
        mk = lambda preds: metric.evaluate_qa([dict(question_id=int(q), answer=int(a)) for q, a, s_ in zip(val["question_id"], preds, sure) if s_],
                                              val["label2ans"], val["qid2data"])
        assert mk(r["preds"]) == mk(g["val_preds"])
        if sure.all():
            res = r["nested_val_metrics"]["evaluate_qa"]
            assert res["overall_acc"] == float(g["overall_acc"])
            assert [res[f"{t}_acc"] for t in metric.QA_ANSWER_TYPES] == list(g["type_acc"])

    def test_exception_in_forward_leaves_the_optimizer_usable(self):
        g, m, rsd, (F, R, NL) = g16_setup("hip")
        arena = ParamArena(m)
        opt = FusedAdamW(arena, lr=1e-4)
        loss_fn = CrossEntropy(impl="hip")
        data = next(syn.qa_batches(syn.qa_questions(rsd, F, R, 0, 4, NL), 4, DEV))
        bad = dict(data, label=data["label"].float())
        with pytest.raises(DemoVLPHipError):
            train_step_qa(m, loss_fn, opt, bad)
        loss, n = train_step_qa(m, loss_fn, opt, data)
        assert np.isfinite(loss.item()) and 0 <= int(n) <= 4
