"""Grounding of search results on a real MI355X (product library): ``dvlp_xattn_index_pairs_ground`` against the score kernel (bit for bit),
against the fp64 reference of ``tests/test_ground.py`` on the same bf16-rounded inputs, and ``VideoIndex.search(ground=True)`` /
``VideoIndex.ground`` on the retrieval set with signal (golden G11's inputs).

Measured on the MI355X over the six shapes x both gates below (bars = twice the measured value, as the figures are printed by the tests):

  per-term deviation of word_scores / region_scores from the fp64 reference      measured 4.89e-3 (G = 240, W = 99, gate on)  -> bar 9.8e-3
  shortfall of the kernel's argmax in the reference's logits (lam = 20)           measured 2.64e-2 (G = 48, W = 37; 1.3e-2 at the large
                                                                                  shapes); doubled that is 5.3e-2, above the 0.05 the
                                                                                  issue allows for delta -> the test holds to 0.05
  deviation of word_region_weight from the reference's P[w, g*]                   measured 3.0e-2 (G = 30, gate on)  -> bar 6.0e-2
  share of words / regions whose argmax equals the reference's                    0.992 - 0.998 on the four shapes with G, W > 1 (asserted
                                                                                  >= 0.90 over all shapes together; per shape printed)

With W = 1 (G = 1) every region's (word's) normalised similarity is +-1, so a column (row) of logits is all ties up to the last bit and the
reference's argmax is decided by rounding: the agreement share of those two shapes is noise (0.0 and 0.6 measured) and is why the share is
asserted over all shapes together; the shortfall rule covers them (2e-6 measured).

Two places where the recipe could not be taken literally, both mended without asking less:
  * G = 1 (or W = 1) with the 'equal' gate: the gate keeps entries with P L > sum P, which the single entry of a length-1 softmax never
    is, so the reference's renormalisation is 0 / 0 and its cosines on that side are NaN.  The kernels give a finite number there (the
    score kernel always has: its full-grid test asserts finite scores at G = 1): the gate is a threshold on rounded fp32 values and either
    drops the entry (0) or keeps it.  Where the reference is NaN the test asserts a finite value; every finite entry is compared.
  * frames = 8 does not divide G = 30: the frame test uses the largest divisor of G that is at most 8 (8, 8, 1, 8, 6, 8 for the six shapes)."""
import numpy as np
import pytest
import torch

from demovlp_amd import ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from demovlp_amd.model import ObjectRelation
from helpers import load_golden
from test_ground import ground_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(4, 9, 240, 99, 5), (3, 7, 288, 112, 4), (3, 5, 1, 99, 3), (3, 6, 240, 1, 5), (1, 1, 30, 99, 1), (3, 5, 48, 37, 2)]
FOCAL = ["equal", "prob"]
LAM = 20.0

SUM_BAR = 5e-5                     # at most 400 fp32 additions of terms below 1: 400 x 2^-24 = 2.4e-5, doubled
SCORE_DEV_MEASURED, SCORE_DEV_BAR = 4.89e-3, 9.8e-3     # twice the measured maximum (below the project's bf16 score bar of 2e-2)
DELTA_MEASURED, DELTA = 2.642e-2, 0.05                   # twice the measured maximum is 5.3e-2, ABOVE the 0.05 it had to stay under: held to 0.05
WEIGHT_DEV_MEASURED, WEIGHT_DEV_BAR = 3.0e-2, 6.0e-2    # twice the measured maximum
AGREE_MIN = 0.90
FLOAT_ROWS = ("word_scores", "region_scores", "word_region_weight", "frame_scores")
INT_ROWS = ("word_region", "region_word")


# ---- the _inputs / _cand / _filled recipe of tests/test_gpu_search.py, restated
def _inputs(Bi, Bj, G, W, seed, dtype):
    rng = np.random.default_rng(seed)
    im = rng.standard_normal((Bi, G, 256), dtype=np.float32)
    cap = rng.standard_normal((Bj, W, 256), dtype=np.float32)
    n = min(G, W)
    for b in range(min(Bi, Bj)):
        cap[b, :n, :64] += 0.5 * im[b, :n, :64]
    m_img = np.zeros((Bi, G), np.float32)
    if G > 4:
        m_img[-1, G - 4:] = -100.0                 # a masked video tail
    m_cap = np.full((Bj, W), -100.0, np.float32)
    for b in range(Bj):
        m_cap[b, : max(1, min(W, 3 + 5 * b))] = 0.0      # ragged caption lengths
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(im).to(dtype), t(cap).to(dtype), t(m_img), t(m_cap)


def _cand(Bj, Bi, K, seed):
    """video rows per caption [Bj, K], with a repeat and an unordered row"""
    c = np.random.default_rng(seed).integers(0, Bi, (Bj, K))
    if K > 1:
        c[0, -1] = c[0, 0]
        c[-1] = np.sort(c[-1])[::-1]
    return c.astype(np.int32)


def _filled(C, capacity, splits):
    G = C.shape[1]
    index = torch.zeros(ops.xattn_index_bytes(capacity, G), device=DEV, dtype=torch.uint8)
    r0 = 0
    for n in splits:
        ops.xattn_index_add(index, capacity, G, r0, C[r0:r0 + n].contiguous())
        r0 += n
    return index


def _frames(G):
    return max(f for f in range(1, 9) if G % f == 0)


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for name in a:
        x, y = a[name], b[name]
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), name


class Run:
    """One shape and gate: the kernel's outputs on the host and the fp64 reference of every distinct (video, caption) pair of the call."""

    def __init__(self, shape, focal):
        Bi, Bj, G, W, K = shape
        self.shape, self.focal, self.frames = shape, focal, _frames(G)
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 11 + G + W, torch.bfloat16)
        self.cand = _cand(Bj, Bi, K, G + K)
        self.args = (_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, torch.from_numpy(self.cand).to(DEV), LAM, focal == "equal")
        self.inputs = (C, Q, mi, mc)
        self.dev = ops.xattn_index_pairs_ground(*self.args, frames=self.frames)
        self.out = {k: v.cpu().numpy() for k, v in self.dev.items()}
        self.m_img = mi.cpu().numpy()
        c64, q64, mi64, mc64 = C.cpu().double(), Q.cpu().double(), mi.cpu().double(), mc.cpu().double()       # the bf16-rounded inputs
        self.ref = {}
        for j in range(Bj):
            for i in set(int(v) for v in self.cand[j]):
                self.ref[(i, j)] = {k: v.numpy() for k, v in ground_reference(c64[i], q64[j], mi64[i], mc64[j], LAM, focal == "equal").items()}

    def pairs(self):
        Bj, K = self.cand.shape
        for j in range(Bj):
            for k in range(K):
                yield j, k, self.ref[(int(self.cand[j, k]), j)]

    def tag(self):
        return "%s %s" % (self.shape, self.focal)


@pytest.fixture(scope="module")
def runs():
    return [Run(s, f) for s in SHAPES for f in FOCAL]


def _dev_where_defined(got, ref, tag):
    """max |got - ref| over the reference's finite entries; where the reference is 0 / 0 (module docstring) the kernel's value is finite"""
    nan = np.isnan(ref)
    assert np.isfinite(got).all(), tag
    return float(np.abs(got[~nan] - ref[~nan]).max()) if (~nan).any() else 0.0


class TestGroundKernelAgainstTheScoreKernel:
    @pytest.mark.parametrize("shape", SHAPES)
    @pytest.mark.parametrize("focal", FOCAL)
    def test_score_is_bit_equal_to_the_score_kernel_and_the_full_grid(self, shape, focal):
        """1: the grounding launch, the score launch and the full-grid launch share the per-pair code and must give one bit pattern."""
        Bi, Bj, G, W, K = shape
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 11 + G + W, torch.bfloat16)
        cand = torch.from_numpy(_cand(Bj, Bi, K, G + K)).to(DEV)
        index = _filled(C, Bi, [Bi])
        with torch.no_grad():
            full = RWALoss(20, focal).get_sim(C, Q, mi, None, mc)                       # [Bi, Bj]
        fwd = ops.xattn_index_pairs_fwd(index, Bi, G, mi, Q, mc, cand, LAM, focal == "equal")
        out = ops.xattn_index_pairs_ground(index, Bi, G, mi, Q, mc, cand, LAM, focal == "equal", frames=_frames(G))
        want = full[cand.long(), torch.arange(Bj, device=DEV)[:, None]]
        assert fwd.shape == (Bj, K) and torch.isfinite(fwd).all()
        assert torch.equal(fwd, want), float((fwd - want).abs().max())
        assert out["score"].dtype == torch.float32 and torch.equal(out["score"], fwd), float((out["score"] - fwd).abs().max())
        assert out["word_scores"].shape == (Bj, K, W) and out["region_scores"].shape == (Bj, K, G) and out["frame_scores"].shape == (Bj, K, _frames(G))
        assert out["word_region"].dtype == torch.int32 and out["region_word"].dtype == torch.int32 and out["word_region_weight"].shape == (Bj, K, W)
        none = ops.xattn_index_pairs_ground(index, Bi, G, mi, Q, mc, cand, LAM, focal == "equal")
        assert "frame_scores" not in none
        _same_bytes(none, {k: v for k, v in out.items() if k != "frame_scores"})

    def test_means_of_the_rows_add_up_to_the_score(self, runs):
        """2: |mean(word_scores) + mean(region_scores) - score| <= 5e-5."""
        worst = 0.0
        for r in runs:
            o = r.out
            d = np.abs(o["word_scores"].astype(np.float64).mean(-1) + o["region_scores"].astype(np.float64).mean(-1) - o["score"]).max()
            print("\n%-36s max |mean(word) + mean(region) - score| %.2e" % (r.tag(), d))
            worst = max(worst, d)
        assert worst <= SUM_BAR, worst

    def test_word_and_region_scores_against_the_fp64_reference(self, runs):
        """3: per-term deviation from the fp64 reference on the same bf16-rounded inputs; bar = twice the measured maximum (module docstring)."""
        worst = 0.0
        for r in runs:
            d = 0.0
            for j, k, ref in r.pairs():
                d = max(d, _dev_where_defined(r.out["word_scores"][j, k], ref["word_scores"], r.tag()),
                        _dev_where_defined(r.out["region_scores"][j, k], ref["region_scores"], r.tag()))
            print("\n%-36s max |word / region score - fp64| %.3e" % (r.tag(), d))
            worst = max(worst, d)
        print("\nper-term deviation over all shapes: %.3e (bar %.3e)" % (worst, SCORE_DEV_BAR))
        assert worst <= SCORE_DEV_BAR, worst

    def test_argmaxes_against_the_fp64_reference(self, runs):
        """4: no exclusions.  The kernel's pick is right when the reference's logit there is within DELTA of the reference's best logit of that
        word (region); where the reference decides by more than DELTA that is exact agreement.  The share of exact agreement is printed per
        run and kind and must be at least 0.90 over all shapes together (module docstring)."""
        worst, pooled = 0.0, {"word_region": [], "region_word": []}
        for r in runs:
            short = {"word_region": 0.0, "region_word": 0.0}
            same = {"word_region": [], "region_word": []}
            for j, k, ref in r.pairs():
                for name, logit in (("word_region", ref["logit_wr"]), ("region_word", ref["logit_rw"])):
                    pick = r.out[name][j, k].astype(np.int64)
                    assert pick.min() >= 0 and pick.max() < logit.shape[1], (r.tag(), name)
                    at = np.take_along_axis(logit, pick[:, None], 1)[:, 0]
                    short[name] = max(short[name], float((logit.max(1) - at).max()))
                    same[name].append(pick == logit.argmax(1))                      # numpy: the first of equal maxima = the smaller index
            for name in short:
                share = float(np.concatenate(same[name]).mean())
                print("\n%-36s %-12s largest shortfall %.3e logit units, exact agreement %.4f" % (r.tag(), name, short[name], share))
                worst = max(worst, short[name])
                pooled[name] += same[name]
        print("\nlargest shortfall over all shapes: %.3e (delta %.3e)" % (worst, DELTA))
        assert worst <= DELTA, worst
        for name in ("word_region", "region_word"):
            share = float(np.concatenate(pooled[name]).mean())
            print("exact agreement over all shapes, %s: %.4f" % (name, share))
            assert share >= AGREE_MIN, (name, share)

    def test_word_region_weight_against_the_reference_at_the_kernels_own_pick(self, runs):
        """5: word_region_weight against the reference's P[w, g*] at the kernel's g*; bar = twice the measured maximum (module docstring)."""
        worst = 0.0
        for r in runs:
            d = 0.0
            for j, k, ref in r.pairs():
                pick = r.out["word_region"][j, k].astype(np.int64)
                d = max(d, _dev_where_defined(r.out["word_region_weight"][j, k], np.take_along_axis(ref["P"], pick[:, None], 1)[:, 0], r.tag()))
            print("\n%-36s max |word_region_weight - fp64 P[w, g*]| %.3e" % (r.tag(), d))
            worst = max(worst, d)
        print("\nweight deviation over all shapes: %.3e (bar %.3e)" % (worst, WEIGHT_DEV_BAR))
        assert worst <= WEIGHT_DEV_BAR, worst

    def test_frame_scores_are_masked_means_of_the_region_scores(self, runs):
        """6: frame_scores = mean of the returned region_scores over the frame's unmasked regions (1e-6); -inf for a frame masked out whole."""
        for r in runs:
            Bi, Bj, G, W, K = r.shape
            F = r.frames
            for j in range(Bj):
                for k in range(K):
                    keep = (r.m_img[r.cand[j, k]] == 0).reshape(F, G // F)
                    rs = r.out["region_scores"][j, k].astype(np.float64).reshape(F, G // F)
                    assert keep.any(1).all()
                    want = (rs * keep).sum(1) / keep.sum(1)
                    assert np.abs(r.out["frame_scores"][j, k] - want).max() <= 1e-6, r.tag()
        # a video with frame 1 masked out whole (and frame 2 in part)
        Bi, Bj, G, W, K = SHAPES[0]
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 3, torch.bfloat16)
        mi[1, 30:60] = -100.0
        mi[1, 60:75] = -100.0
        cand = _cand(Bj, Bi, K, 2)
        cand[:, 1] = 1
        out = ops.xattn_index_pairs_ground(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, torch.from_numpy(cand).to(DEV), LAM, True, frames=8)
        fs, rs = out["frame_scores"].cpu().numpy(), out["region_scores"].cpu().numpy().astype(np.float64)
        hit = cand == 1
        assert hit.sum() >= Bj and np.isneginf(fs[hit][:, 1]).all() and np.isfinite(np.delete(fs[hit], 1, axis=1)).all() and np.isfinite(fs[~hit]).all()
        assert np.abs(fs[hit][:, 2] - rs[hit][:, 75:90].mean(1)).max() <= 1e-6 and np.abs(fs[hit][:, 0] - rs[hit][:, :30].mean(1)).max() <= 1e-6
        assert torch.isfinite(out["score"]).all() and torch.isfinite(out["region_scores"]).all()

    def test_indices_are_in_range_and_no_word_names_a_masked_region(self, runs):
        """7."""
        for r in runs:
            Bi, Bj, G, W, K = r.shape
            wr, rw = r.out["word_region"], r.out["region_word"]
            assert wr.min() >= 0 and wr.max() < G and rw.min() >= 0 and rw.max() < W, r.tag()
            masked = r.m_img[r.cand] != 0                                            # [Bj, K, G]
            assert (~masked).any(-1).all()
            assert not np.take_along_axis(masked, wr.astype(np.int64), 2).any(), r.tag()

    def test_out_of_range_candidates_give_nan_and_minus_one_and_leave_the_others(self):
        """8."""
        Bi, Bj, G, W, K = 4, 5, 240, 99, 4
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5, torch.bfloat16)
        index = _filled(C, 6, [Bi])                                                     # capacity 6: rows 4, 5 were never added
        mi6 = torch.cat([mi, torch.zeros(2, G, device=DEV)])
        cand = _cand(Bj, Bi, K, 1)
        good = ops.xattn_index_pairs_ground(index, 6, G, mi6, Q, mc, torch.from_numpy(cand).to(DEV), LAM, True, frames=8)
        bad = cand.copy()
        bad[1, 2], bad[3, 0], bad[4, 3] = -1, 6, 2 ** 31 - 1
        got = ops.xattn_index_pairs_ground(index, 6, G, mi6, Q, mc, torch.from_numpy(bad).to(DEV), LAM, True, frames=8)
        hole = torch.from_numpy(bad != cand).to(DEV)
        assert int(hole.sum()) == 3
        assert torch.isnan(got["score"][hole]).all() and torch.isfinite(good["score"]).all()
        for name in FLOAT_ROWS:
            assert torch.isnan(got[name][hole]).all(), name
        for name in INT_ROWS:
            assert (got[name][hole] == -1).all() and (good[name] >= 0).all(), name
        _same_bytes({k: v[~hole] for k, v in got.items()}, {k: v[~hole] for k, v in good.items()})

    def test_two_calls_give_identical_bytes(self, runs):
        """9: nothing depends on which wave or workgroup finished first."""
        for r in runs:
            _same_bytes(ops.xattn_index_pairs_ground(*r.args, frames=r.frames), r.dev)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 10. end to end on the retrieval set with signal (the g11 recipe of tests/test_gpu_search.py, restated)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _retrieval_model(F, R, sd, dtype):
    m = ObjectRelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None},
                       {"model": "pretrained/distilbert-base-uncased", "pretrained": True, "input": "text", "two_outputs": True}, pretrained_init=False, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.set_text_dropout(0.0)
    return m.to(DEV)


def _retrieval_batches(sd, F, R, BS, NB):
    for b in range(NB):
        obj, mask, ids, att = syn.retrieval_batch(sd, F, R, b * BS, BS)
        yield {"text": {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(att).to(DEV)},
               "object": torch.from_numpy(obj).to(DEV), "object_mask": torch.from_numpy(mask).to(DEV)}


@pytest.fixture(scope="module")
def g11():
    g = load_golden("g11_retrieval.npz")
    F, R, BS, NB = int(g["F"]), int(g["R"]), int(g["batch"]), int(g["batches"])
    sd = syn.retrieval_state_dict(F, R)
    model = _retrieval_model(F, R, sd, "bfloat16")
    loss = GlobalLocalLoss(use_local=True, use_global=True, coef=1.0, focal_type="equal")
    batches = list(_retrieval_batches(sd, F, R, BS, NB))
    index = search.VideoIndex(BS * NB, F * R, torch.bfloat16, DEV).add_batches(model, batches)
    return dict(model=model, loss=loss, batches=batches, index=index, F=F, R=R)


class TestSearchWithGrounding:
    def test_search_with_ground_returns_the_search_and_what_ground_returns(self, g11):
        ix, model, loss, F, R = g11["index"], g11["model"], g11["loss"], g11["F"], g11["R"]
        assert ix.fused and F == 8
        for b in g11["batches"][:2]:
            text = b["text"]
            Nq, W = text["input_ids"].shape[0], text["input_ids"].shape[1] - 1
            ids0, scores0 = ix.search(model, loss, text, k=5)
            res = ix.search(model, loss, text, k=5, ground=True, frames=8)
            assert len(res) == 3
            ids, scores, gr = res
            assert torch.equal(ids, ids0) and torch.equal(scores.view(torch.int32), scores0.view(torch.int32))
            assert gr["score"].shape == (Nq, 5) and gr["word_scores"].shape == (Nq, 5, W) and gr["region_scores"].shape == (Nq, 5, F * R)
            assert gr["frame_scores"].shape == (Nq, 5, 8) and gr["word_frame"].shape == (Nq, 5, W) and all(v.is_cuda for v in gr.values())
            # the local addend: score = cosine + grounding["score"]
            with torch.no_grad():
                gt = model.eval().compute_text(text)[0]
            all_ids, cos = ix.shortlist_by_cosine(gt, None)
            assert torch.equal(all_ids, torch.arange(len(ix), device=DEV).expand(Nq, -1))
            dev = float((gr["score"] + torch.gather(cos, 1, ids) - scores).abs().max())
            print("\nmax |grounding score + cosine - search score| %.2e" % dev)
            assert dev <= 1e-6
            _same_bytes(ix.ground(model, loss, text, ids, frames=8), gr)
            assert gr["word_valid"].dtype == torch.bool and torch.equal(gr["word_valid"], text["attention_mask"][:, 1:] > 0)
            assert torch.equal(gr["word_frame"], gr["word_region"] // R) and int(gr["word_frame"].max()) < F and int(gr["word_frame"].min()) >= 0
            assert not model.training
        model.train()
        try:
            again = ix.ground(model, loss, text, ids.int(), frames=8)
            assert model.training and not again["score"].requires_grad
            _same_bytes(again, gr)
        finally:
            model.eval()
