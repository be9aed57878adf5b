"""Multiple-choice evaluation on the device (b): the pair-list local similarity
(``dvlp_xattn_pairs_fwd`` through ``RWALoss.get_sim_pairs``) against the full-grid fused kernel (bf16, bit for bit) and the fp64 oracle
(fp32), and ``trainer.evaluate_mc`` against the reference's multiple-choice loop (golden G15)."""
import os

import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, metric, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from demovlp_amd.model import ObjectMCRelation
from demovlp_amd.trainer import evaluate_mc
from oracle import restatement as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G15 = os.path.join(ROOT, "tests", "golden", "g15_mc.npz")

# bf16 evaluate_mc vs G15, measured on the MI355X ("Multiple-choice evaluation"): max |score - reference| 3.2e-3, no prediction
# changed, accuracy equal.  A prediction can only flip where the reference's top-1 gap is below twice the score deviation:
BF16_MC_GAP = 6.5e-3          # every question whose reference top-1 gap exceeds this keeps its prediction (2 x 3.2e-3)
BF16_MC_ACC_POINTS = 1.25     # accuracy within one question of 80 (measured: equal)


def _inputs(Bi, Bj, G, W, seed, dtype):
    rng = np.random.default_rng(seed)
    im = rng.standard_normal((Bi, G, 256), dtype=np.float32)
    cap = rng.standard_normal((Bj, W, 256), dtype=np.float32)
    n = min(G, W)
    for b in range(min(Bi, Bj)):
        cap[b, :n, :64] += 0.5 * im[b, :n, :64]
    m_img = np.zeros((Bi, G), np.float32)
    if G > 4:
        m_img[-1, G - 4:] = -100.0                                    # padded regions
    m_cap = np.full((Bj, W), -100.0, np.float32)                      # padded words
    for b in range(Bj):
        m_cap[b, : max(1, min(W, 3 + 5 * b))] = 0.0
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(im).to(dtype), t(cap).to(dtype), t(m_img), t(m_cap)


def _cand(Bi, Bj, K, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, Bj, (Bi, K))
    if K > 1:
        c[0, -1] = c[0, 0]                                            # a repeat
        c[-1] = np.sort(c[-1])[::-1]                                  # out of order
    return c.astype(np.int64)


class TestPairsBf16BitEqualToFullGrid:
    @pytest.mark.parametrize("Bi,Bj,G,W,K", [(4, 9, 240, 99, 5), (3, 7, 288, 112, 4), (3, 5, 1, 99, 3), (3, 6, 240, 1, 5), (4, 6, 288, 99, 1),
                                             (1, 8, 240, 99, 6), (1, 1, 30, 99, 1)])
    @pytest.mark.parametrize("focal", ["equal", "prob"])
    def test_equals_get_sim_entries(self, Bi, Bj, G, W, K, focal):
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 11 + G + W, torch.bfloat16)
        loss = RWALoss(20, focal)
        cand = _cand(Bi, Bj, K, G + K)
        with torch.no_grad():
            full = loss.get_sim(C, Q, mi, None, mc)
            pairs = loss.get_sim_pairs(C, Q, mi, None, mc, cand=cand)
            pairs_dev = loss.get_sim_pairs(C, Q, mi, None, mc, cand=torch.from_numpy(cand).to(DEV))
        want = full[torch.arange(Bi, device=DEV)[:, None], torch.from_numpy(cand).to(DEV)]
        assert pairs.shape == (Bi, K) and pairs.dtype == torch.float32
        assert torch.isfinite(pairs).all()
        assert torch.equal(pairs, want), float((pairs - want).abs().max())
        assert torch.equal(pairs_dev, want)

    def test_multiple_choice_layout_without_cand(self):
        Bi, K, G, W = 6, 5, 240, 99
        C, Q, mi, mc = _inputs(Bi, Bi * K, G, W, 5, torch.bfloat16)
        loss = RWALoss(20, "equal")
        with torch.no_grad():
            full = loss.get_sim(C, Q, mi, None, mc)
            pairs = loss.get_sim_pairs(C, Q, mi, None, mc)
        want = full[torch.arange(Bi, device=DEV)[:, None], torch.arange(Bi * K, device=DEV).view(Bi, K)]
        assert torch.equal(pairs, want)

    def test_forward_only(self):
        C, Q, mi, mc = _inputs(2, 4, 30, 20, 1, torch.bfloat16)
        with pytest.raises(DemoVLPHipError):
            RWALoss(20, "equal").get_sim_pairs(C.requires_grad_(True), Q, mi, None, mc, cand=np.zeros((2, 2), np.int64))
        with pytest.raises(ValueError):
            RWALoss(20, "equal").get_sim_pairs(C.detach(), Q, mi, None, mc, cand=np.full((2, 2), 4, np.int64))


class TestPairsFp32VsOracle:
    @pytest.mark.parametrize("Bi,Bj,G,W,K", [(3, 7, 240, 99, 4), (2, 4, 1152, 99, 3), (2, 5, 30, 99, 2), (2, 3, 3, 7, 3)])
    def test_within_1e5_of_fp64(self, Bi, Bj, G, W, K):
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 3 + G, torch.float32)
        cand = _cand(Bi, Bj, K, 7 + G)
        with torch.no_grad():
            got = RWALoss(20, "equal").get_sim_pairs(C, Q, mi, None, mc, cand=cand).cpu().double()
        Cd, Qd, mid, mcd = C.cpu().double(), Q.cpu().double(), mi.cpu().double(), mc.cpu().double()
        ref = torch.tensor([[float(orc.xattn_pair(Cd[i], Qd[int(cand[i, k])], mid[i], mcd[int(cand[i, k])], 20.0, True)) for k in range(K)]
                            for i in range(Bi)], dtype=torch.float64)
        err = float((got - ref).abs().max())
        print("\npairs fp32 Bi=%d Bj=%d G=%d W=%d K=%d: max |score - fp64 oracle| %.2e" % (Bi, Bj, G, W, K, err))
        assert err < 1e-5, err

    def test_bf16_beyond_the_fused_range_matches_the_full_grid(self):
        Bi, Bj, G, W, K = 2, 4, 1152, 99, 3                            # F = 32, R = 36: the gathered multi-kernel path
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 9, torch.bfloat16)
        cand = _cand(Bi, Bj, K, 2)
        loss = RWALoss(20, "equal")
        with torch.no_grad():
            full = loss.get_sim(C, Q, mi, None, mc)
            pairs = loss.get_sim_pairs(C, Q, mi, None, mc, cand=cand)
        want = full[torch.arange(Bi, device=DEV)[:, None], torch.from_numpy(cand).to(DEV)]
        err = float((pairs - want).abs().max())
        print("\npairs bf16 G=1152: max |pairs - full grid| %.2e" % err)
        assert err < 2e-3, err


def _mc_model(dtype, F, R):
    m = ObjectMCRelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None},
                         {"model": "pretrained/distilbert-base-uncased", "pretrained": True, "input": "text", "two_outputs": True},
                         pretrained_init=False, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.retrieval_state_dict(F, R).items()}, strict=True)
    m.set_text_dropout(0.0)
    return m.to(DEV)


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(G15))


@pytest.fixture(scope="module")
def mc_set(g15):
    F, R = int(g15["F"]), int(g15["R"])
    return syn.mc_questions(syn.retrieval_state_dict(F, R), F, R, int(g15["first"]), int(g15["n"]), int(g15["K"]))


def _gt(g15):
    return {int(i): int(a) for i, a in zip(g15["mc_ids"], g15["answers"])}


def _loss():
    return GlobalLocalLoss(use_local=True, use_global=True, coef=1.0, focal_type="equal")


class TestEvaluateMcVsReference:
    def test_fp32_vs_g15(self, g15, mc_set):
        model = _mc_model("float32", int(g15["F"]), int(g15["R"]))
        res = evaluate_mc(model, _loss(), syn.mc_batches(mc_set, 16, DEV), _gt(g15))
        dev = np.abs(res["scores"] - g15["scores"]).max()
        pred = np.array([res["pred_id2answer"][int(i)] for i in g15["mc_ids"]])
        clear = g15["top_gap"] > 1e-4
        print("\nmc fp32: max |score - reference| %.2e; %d of %d predictions differ (%d decided by < 1e-4); accuracy %s vs %s"
              % (dev, (pred != g15["preds"]).sum(), len(pred), (~clear).sum(), res["nested_val_metrics"]["evaluate_mc"]["mc_accuracy"],
                 g15["mc_accuracy"]))
        assert dev < 1e-4, dev
        assert (pred[clear] == g15["preds"][clear]).all()
        assert res["nested_val_metrics"] == {"evaluate_mc": {"mc_accuracy": str(g15["mc_accuracy"])}}

    def test_bf16_vs_g15(self, g15, mc_set):
        model = _mc_model("bfloat16", int(g15["F"]), int(g15["R"]))
        res = evaluate_mc(model, _loss(), syn.mc_batches(mc_set, 32, DEV), _gt(g15))
        dev = np.abs(res["scores"] - g15["scores"]).max()
        pred = np.array([res["pred_id2answer"][int(i)] for i in g15["mc_ids"]])
        clear = g15["top_gap"] > BF16_MC_GAP
        acc = float(res["nested_val_metrics"]["evaluate_mc"]["mc_accuracy"])
        print("\nmc bf16: max |score - reference| %.2e; %d of %d predictions differ (%d decided by < %.1e); accuracy %.2f vs %s"
              % (dev, (pred != g15["preds"]).sum(), len(pred), (~clear).sum(), BF16_MC_GAP, acc, g15["mc_accuracy"]))
        assert (pred[clear] == g15["preds"][clear]).all()
        assert abs(acc - float(str(g15["mc_accuracy"]))) <= BF16_MC_ACC_POINTS


class TestEvaluateMcBehaviour:
    def test_batching_q1_equals_q32(self, g15, mc_set):
        model = _mc_model("bfloat16", int(g15["F"]), int(g15["R"]))
        sub = {k: (v[:40] if k not in ("input_ids", "attention_mask") else v[:40 * int(g15["K"])]) for k, v in mc_set.items()}
        r1 = evaluate_mc(model, _loss(), syn.mc_batches(sub, 1, DEV), _gt(g15))
        r32 = evaluate_mc(model, _loss(), syn.mc_batches(sub, 32, DEV), _gt(g15))
        assert r1["pred_id2answer"] == r32["pred_id2answer"]
        assert list(r1["pred_id2answer"]) == [int(i) for i in sub["mc_ids"]]
        print("\nmc bf16 Q=1 vs Q=32: max |score diff| %.2e" % np.abs(r1["scores"] - r32["scores"]).max())

    def test_per_option_global_term(self, g15, mc_set):
        from demovlp_amd.model import sim_matrix
        model = _mc_model("float32", int(g15["F"]), int(g15["R"]))
        K = int(g15["K"])
        sub = {k: (v[:8] if k not in ("input_ids", "attention_mask") else v[:8 * K]) for k, v in mc_set.items()}
        ref = evaluate_mc(model, _loss(), syn.mc_batches(sub, 8, DEV), _gt(g15))
        per = evaluate_mc(model, _loss(), syn.mc_batches(sub, 8, DEV), _gt(g15), global_term="per_option")
        b = next(syn.mc_batches(sub, 8, DEV))
        with torch.no_grad():
            out = model(b, return_embeds=True)
            g = sim_matrix(out["global_text_embeddings"], out["global_object_embeddings"]).view(8, K, 8)
            g = g[torch.arange(8), :, torch.arange(8)].float().cpu().numpy()        # cos(t_{q,k}, v_q)
        # reference: every option carries cos(t_{q,0}, v_q); per_option: option k carries cos(t_{q,k}, v_q); the local term is the same
        assert np.allclose(per["scores"] - ref["scores"], g - g[:, :1], atol=1e-6, rtol=0)
        assert np.abs(g - g[:, :1]).max() > 1e-4                                     # the two modes do differ here
        with pytest.raises(ValueError):
            evaluate_mc(model, _loss(), syn.mc_batches(sub, 8, DEV), _gt(g15), global_term="other")

    def test_train_mode_is_restored(self, g15, mc_set):
        model = _mc_model("bfloat16", int(g15["F"]), int(g15["R"]))
        K = int(g15["K"])
        sub = {k: (v[:4] if k not in ("input_ids", "attention_mask") else v[:4 * K]) for k, v in mc_set.items()}
        model.train()
        res = evaluate_mc(model, _loss(), syn.mc_batches(sub, 4, DEV), _gt(g15), metrics=[metric.evaluate_mc])
        assert model.training and all(m.training for m in model.modules())
        model.eval()
        evaluate_mc(model, _loss(), syn.mc_batches(sub, 4, DEV), _gt(g15))
        assert not model.training
        assert set(res["pred_id2answer"]) == {int(i) for i in sub["mc_ids"]} and res["scores"].shape == (4, K)
