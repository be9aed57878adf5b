"""Video-to-text search on a real MI355X: the caption-index pair kernel against the fused full grid and against the video-index pair kernel
(bit for bit), its grounding twin against ``dvlp_xattn_index_pairs_ground`` (byte for byte), and ``search.CaptionIndex`` against
``trainer.evaluate`` on the retrieval set with signal (golden G11's inputs) in the search orientation ``global_sims.T + local_sims``.

Bounds.  ``SCORE_TOL`` and ``RANK_GAP`` are the ones of ``tests/test_gpu_search.py``: the cosine is a 256-term fp32 dot product of unit
vectors (256 x 2^-24 = 1.5e-5 between two summation orders) and the local addend is bit-equal.  Share of the top-10 positions clear of ties:
the golden's own matrices give 0.957 for ``global_sims + local_sims.T`` (t2v) and 0.932 for ``global_sims.T + local_sims`` (v2t), both above
the 0.9 the t2v test asks, so 0.9 is asked here too.  The partial-shortlist test does not cut at the t2v test's S = 32: along a video's row
this set's global cosines are nearly flat (every caption within 1e-3 of -0.042; it is why G11's v2t R@1 is 23 %), so 256 cosines share a range
of about 25 RANK_GAPs and a gap above RANK_GAP at one given position is the exception -- in ``trainer.evaluate``'s own bf16 ``global_sims.T``
23 of 256 rows have one between the 13th and 14th caption (MI355X; the fp32 golden's matrix, from which 13 was first taken, has 193 there and
says nothing about the bf16 run).  The test therefore reads the cut from the reference matrix itself: S is the size in [10, 64] at which
``trainer.evaluate``'s ``global_sims.T`` has the most rows with a clear cut (nothing the code under test computed enters that choice), at
least one such row must exist, and on those rows the shortlist must be the reference's set exactly.  The rule for rows without a clear cut
-- no left-out caption beats a shortlisted one by more than RANK_GAP -- is asserted on every row, as there."""
import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, metric, ops, search, synthetic as syn
from demovlp_amd import functional as Fn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from demovlp_amd.model import ObjectRelation
from demovlp_amd.trainer import evaluate
from helpers import load_golden
from oracle import restatement as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"

SCORE_TOL = 2e-5
RANK_GAP = 4e-5
LAM = 20.0
SHAPES = [(4, 9, 240, 99, 5), (3, 7, 288, 112, 4), (3, 5, 1, 99, 3), (3, 6, 240, 1, 5), (4, 6, 288, 99, 1), (1, 8, 240, 99, 6), (1, 1, 30, 99, 1)]
FOCAL = ["equal", "prob"]
FLOAT_ROWS = ("word_scores", "region_scores", "word_region_weight", "frame_scores")
INT_ROWS = ("word_region", "region_word")


# ---- the _inputs recipe of tests/test_gpu_search.py, restated; candidates per VIDEO here
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


def _cand(Bi, Bj, K, seed):
    """caption rows per video [Bi, K], with a repeat and an unordered row"""
    c = np.random.default_rng(seed).integers(0, Bj, (Bi, K))
    if K > 1:
        c[0, -1] = c[0, 0]
        c[-1] = np.sort(c[-1])[::-1]
    return c.astype(np.int32)


def _filled(Q, capacity, splits):
    W = Q.shape[1]
    index = torch.zeros(ops.xattn_caption_index_bytes(capacity, W), device=DEV, dtype=torch.uint8)
    r0 = 0
    for n in splits:
        ops.xattn_caption_index_add(index, capacity, W, r0, Q[r0:r0 + n].contiguous())
        r0 += n
    return index


def _video_index(C):
    index = torch.zeros(ops.xattn_index_bytes(C.shape[0], C.shape[1]), device=DEV, dtype=torch.uint8)
    ops.xattn_index_add(index, C.shape[0], C.shape[1], 0, C.contiguous())
    return index


def _all_videos(Bj, Bi):
    return torch.arange(Bi, device=DEV, dtype=torch.int32).expand(Bj, -1).contiguous()


def _frames(G):
    return max(f for f in range(1, 9) if G % f == 0)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for name in a:
        x, y = a[name], b[name]
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert torch.equal(_bits(x), _bits(y)), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the pair kernel against the full grid and against the other direction, bf16
# ---------------------------------------------------------------------------------------------------------------------------------------
class TestCaptionIndexPairsBf16BitEqualToFullGrid:
    @pytest.mark.parametrize("Bi,Bj,G,W,K", SHAPES)
    @pytest.mark.parametrize("focal", FOCAL)
    def test_equals_get_sim_entries_and_the_video_index_kernel(self, Bi, Bj, G, W, K, focal):
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 11 + G + W, torch.bfloat16)
        cand = torch.from_numpy(_cand(Bi, Bj, K, G + K)).to(DEV)
        index = _filled(Q, Bj, [Bj])
        with torch.no_grad():
            full = RWALoss(20, focal).get_sim(C, Q, mi, None, mc)                       # [Bi, Bj]
        got = ops.xattn_caption_index_pairs_fwd(index, Bj, W, mc, C, mi, cand, LAM, focal == "equal")
        want = full[torch.arange(Bi, device=DEV)[:, None], cand.long()]
        assert got.shape == (Bi, K) and got.dtype == torch.float32 and torch.isfinite(got).all()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), float((got - want).abs().max())
        # the same pairs through the other direction: every (caption j, video i) over a resident video index
        other = ops.xattn_index_pairs_fwd(_video_index(C), Bi, G, mi, Q, mc, _all_videos(Bj, Bi), LAM, focal == "equal")    # [Bj, Bi]
        want = other[cand.long(), torch.arange(Bi, device=DEV)[:, None]]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), float((got - want).abs().max())

    def test_three_adds_are_byte_equal_to_one_and_spare_rows_stay_untouched(self):
        C, Q, mi, mc = _inputs(3, 7, 240, 99, 3, torch.bfloat16)
        one, three = _filled(Q, 9, [7]), _filled(Q, 9, [2, 4, 1])
        assert torch.equal(one, three)
        assert one.any() and not torch.equal(one, _filled(Q.flip(0), 9, [7]))
        # rows 7, 8 of each section were never written: qhat [9][112][256], qhatT [9][256][128] (bf16), nq [9][99] (fp32)
        per_a, per_b = 112 * 256 * 2, 256 * 128 * 2
        assert ops.xattn_caption_index_bytes(9, 99) == 9 * (per_a + per_b) + 3584
        assert not one[7 * per_a:9 * per_a].any() and not one[9 * per_a + 7 * per_b:9 * (per_a + per_b)].any()
        assert not one[9 * (per_a + per_b) + 7 * 99 * 4:].any()
        assert one[6 * per_a:7 * per_a].any() and one[9 * per_a + 6 * per_b:9 * per_a + 7 * per_b].any()

    def test_out_of_range_candidate_scores_nan_and_leaves_the_others(self):
        Bi, Bj, G, W, K = 5, 4, 240, 99, 4
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5, torch.bfloat16)
        index = _filled(Q, 6, [Bj])                                                     # capacity 6: rows 4, 5 were never added
        mc6 = torch.cat([mc, torch.zeros(2, W, device=DEV)])
        cand = _cand(Bi, Bj, K, 1)
        good = ops.xattn_caption_index_pairs_fwd(index, 6, W, mc6, C, mi, torch.from_numpy(cand).to(DEV), LAM, True)
        bad = cand.copy()
        bad[1, 2], bad[3, 0], bad[4, 3] = -1, 6, 2 ** 31 - 1
        got = ops.xattn_caption_index_pairs_fwd(index, 6, W, mc6, C, mi, torch.from_numpy(bad).to(DEV), LAM, True)
        hole = torch.from_numpy(bad != cand).to(DEV)
        assert int(hole.sum()) == 3
        assert torch.isnan(got[hole]).all() and torch.isfinite(good).all()
        assert torch.equal(got[~hole].view(torch.int32), good[~hole].view(torch.int32))

    def test_forward_only(self):
        C, Q, mi, mc = _inputs(3, 2, 30, 20, 1, torch.bfloat16)
        C.requires_grad_(True)
        s = Fn.XattnCaptionIndexPairsFn.apply(_filled(Q, 2, [2]), 2, 20, mc, C, mi, torch.zeros(3, 2, device=DEV, dtype=torch.int32), LAM, True)
        assert s.shape == (3, 2) and torch.isfinite(s).all()
        with pytest.raises(DemoVLPHipError):
            s.sum().backward()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the grounding kernel against the score kernel and against the video-index grounding kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
class TestCaptionIndexGroundKernel:
    @pytest.mark.parametrize("Bi,Bj,G,W,K", SHAPES)
    @pytest.mark.parametrize("focal", FOCAL)
    def test_score_is_bit_equal_and_rows_are_byte_equal_to_the_video_index_grounding(self, Bi, Bj, G, W, K, focal):
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 11 + G + W, torch.bfloat16)
        cand = torch.from_numpy(_cand(Bi, Bj, K, G + K)).to(DEV)
        index, F, gate = _filled(Q, Bj, [Bj]), _frames(G), focal == "equal"
        fwd = ops.xattn_caption_index_pairs_fwd(index, Bj, W, mc, C, mi, cand, LAM, gate)
        out = ops.xattn_caption_index_pairs_ground(index, Bj, W, mc, C, mi, cand, LAM, gate, frames=F)
        assert out["score"].dtype == torch.float32 and torch.equal(out["score"].view(torch.int32), fwd.view(torch.int32))
        assert out["word_scores"].shape == (Bi, K, W) and out["region_scores"].shape == (Bi, K, G) and out["frame_scores"].shape == (Bi, K, F)
        assert out["word_region"].dtype == torch.int32 and out["region_word"].dtype == torch.int32 and out["word_region_weight"].shape == (Bi, K, W)
        none = ops.xattn_caption_index_pairs_ground(index, Bj, W, mc, C, mi, cand, LAM, gate)
        assert "frame_scores" not in none
        _same_bytes(none, {k: v for k, v in out.items() if k != "frame_scores"})
        # every pair through the other direction's grounding: row (i, k) here is row (cand[i, k], i) there
        other = ops.xattn_index_pairs_ground(_video_index(C), Bi, G, mi, Q, mc, _all_videos(Bj, Bi), LAM, gate, frames=F)      # [Bj, Bi, ...]
        rows = torch.arange(Bi, device=DEV)[:, None]
        _same_bytes(out, {name: v[cand.long(), rows] for name, v in other.items()})
        # two calls give identical bytes: nothing depends on which wave or workgroup finished first
        _same_bytes(ops.xattn_caption_index_pairs_ground(index, Bj, W, mc, C, mi, cand, LAM, gate, frames=F), out)

    def test_out_of_range_candidates_give_nan_and_minus_one_and_leave_the_others(self):
        Bi, Bj, G, W, K = 5, 4, 240, 99, 4
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5, torch.bfloat16)
        index = _filled(Q, 6, [Bj])
        mc6 = torch.cat([mc, torch.zeros(2, W, device=DEV)])
        cand = _cand(Bi, Bj, K, 1)
        good = ops.xattn_caption_index_pairs_ground(index, 6, W, mc6, C, mi, torch.from_numpy(cand).to(DEV), LAM, True, frames=8)
        bad = cand.copy()
        bad[1, 2], bad[3, 0], bad[4, 3] = -1, 6, 2 ** 31 - 1
        got = ops.xattn_caption_index_pairs_ground(index, 6, W, mc6, C, mi, torch.from_numpy(bad).to(DEV), LAM, True, frames=8)
        hole = torch.from_numpy(bad != cand).to(DEV)
        assert int(hole.sum()) == 3
        assert torch.isnan(got["score"][hole]).all() and torch.isfinite(good["score"]).all()
        for name in FLOAT_ROWS:
            assert torch.isnan(got[name][hole]).all(), name
        for name in INT_ROWS:
            assert (got[name][hole] == -1).all() and (good[name] >= 0).all(), name
        _same_bytes({k: v[~hole] for k, v in got.items()}, {k: v[~hole] for k, v in good.items()})


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. CaptionIndex against trainer.evaluate on the retrieval set with signal (bf16, fused route); inputs as in tests/test_gpu_search.py
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


LOSS = dict(use_local=True, use_global=True, coef=1.0, focal_type="equal")


@pytest.fixture(scope="module")
def g11():
    g = load_golden("g11_retrieval.npz")
    F, R, BS, NB = int(g["F"]), int(g["R"]), int(g["batch"]), int(g["batches"])
    sd = syn.retrieval_state_dict(F, R)
    model = _retrieval_model(F, R, sd, "bfloat16")
    loss = GlobalLocalLoss(**LOSS)
    batches = list(_retrieval_batches(sd, F, R, BS, NB))
    res = evaluate(model, loss, batches)
    W = batches[0]["text"]["input_ids"].shape[1] - 1
    index = search.CaptionIndex(BS * NB, W, torch.bfloat16, DEV).add_batches(model, batches)          # captions indexed batch by batch
    att = torch.cat([b["text"]["attention_mask"] for b in batches])
    full = res["global_sims"].T.astype(np.float64) + res["local_sims"].astype(np.float64)             # the search orientation: [video, caption]
    return dict(model=model, loss=loss, batches=batches, res=res, index=index, att=att, full=full, n=BS * NB, F=F, R=R, W=W)


def _videos(b):
    return {"object": b["object"], "object_mask": b["object_mask"]}


def _search(g11, index=None, **kw):
    """Every video of the set, searched batch by batch as ``trainer.evaluate`` runs the object tower (a tower's bf16 output depends on the
    batch it was computed in), results concatenated."""
    parts = [(index or g11["index"]).search(g11["model"], g11["loss"], _videos(b), **kw) for b in g11["batches"]]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _ordered(ids, scores):
    """best first, equal scores by smaller id"""
    s, i = scores[:, :-1], ids[:, :-1]
    return bool(((s > scores[:, 1:]) | ((s == scores[:, 1:]) & (i < ids[:, 1:]))).all())


class TestCaptionSearchOnTheRetrievalSet:
    def test_exact_search_equals_the_transposed_full_grid(self, g11):
        ix, full, n = g11["index"], g11["full"], g11["n"]
        assert len(ix) == n and ix.fused and ix.W == 99
        ids, scores = _search(g11, k=10, shortlist=None)
        assert ids.shape == (n, 10) and ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.is_cuda
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        dev = np.abs(scores - np.take_along_axis(full, ids, 1)).max()
        order = np.argsort(-full, axis=1, kind="stable")
        srt = np.take_along_axis(full, order, 1)
        gap = srt[:, :-1] - srt[:, 1:]                                                    # gap[p] = between positions p and p + 1
        clear = np.concatenate([np.ones((n, 1), bool), gap[:, :9] > RANK_GAP], 1) & (gap[:, :10] > RANK_GAP)
        print("\nexact v2t search: max |score - (global.T + local)| %.2e; %d of %d positions clear of ties" % (dev, clear.sum(), clear.size))
        assert dev < SCORE_TOL, dev
        assert np.array_equal(ids[clear], order[:, :10][clear])
        assert _ordered(ids, scores) and clear.mean() > 0.9
        # the quirk orientation of trainer.evaluate is a different matrix (its metrics are not comparable)
        assert np.abs(g11["res"]["o2t_sims"].T - full).max() > 1e-2

    def test_exact_search_is_the_transpose_of_exact_text_to_video_search(self, g11):
        model, loss, batches, n = g11["model"], g11["loss"], g11["batches"], g11["n"]
        vix = search.VideoIndex(n, g11["F"] * g11["R"], torch.bfloat16, DEV).add_batches(model, batches)
        t2v = [vix.search(model, loss, b["text"], k=n, shortlist=None) for b in batches]
        v2t = _search(g11, k=n, shortlist=None)

        def matrix(ids, scores):
            m = torch.full((n, n), float("nan"), device=DEV)
            m.scatter_(1, ids, scores)
            return m.cpu().numpy().astype(np.float64)

        a = matrix(torch.cat([p[0] for p in t2v]), torch.cat([p[1] for p in t2v]))        # [caption, video]
        b = matrix(*v2t)                                                                  # [video, caption]
        assert np.isfinite(a).all() and np.isfinite(b).all()
        dev = np.abs(b - a.T).max()
        print("\nmax |v2t score - t2v score of the same pair| %.2e" % dev)
        assert dev < SCORE_TOL, dev

    def test_partial_shortlist_is_exact_on_the_shortlist(self, g11):
        ix, full, n = g11["index"], g11["full"], g11["n"]
        model = g11["model"]
        glob = g11["res"]["global_sims"].T.astype(np.float64)                             # [video, caption], trainer.evaluate's
        order = np.argsort(-glob, axis=1, kind="stable")
        srt = np.take_along_axis(glob, order, 1)
        cuts = ((srt[:, :-1] - srt[:, 1:]) > RANK_GAP).sum(0)                             # cuts[p]: rows with a clear cut after p + 1 captions
        S = 10 + int(np.argmax(cuts[9:64]))                                               # from the reference matrix alone: module docstring
        decided = (srt[:, S - 1] - srt[:, S]) > RANK_GAP                                  # rows whose S-th / (S+1)-th are not within rounding
        print("\nshortlist %d: %d of %d rows have a clear cut (at 13: %d, at 32: %d)" % (S, decided.sum(), n, cuts[12], cuts[31]))
        with torch.no_grad():
            go = torch.cat([model.eval().compute_object(b["object"], b["object_mask"])[0] for b in g11["batches"]])
        sl, cos = ix.shortlist_by_cosine(go, S)
        sl = sl.cpu().numpy()
        assert 10 <= S <= 64 and decided.sum() >= 1 and (np.diff(sl, axis=1) > 0).all()
        assert np.array_equal(sl[decided], np.sort(order[:, :S], axis=1)[decided])
        # every row, clear cut or not: no caption left out beats a shortlisted one by more than rounding
        inside = np.zeros((n, n), bool)
        np.put_along_axis(inside, sl, True, 1)
        assert inside.sum(1).min() == S
        assert (np.where(inside, -np.inf, glob).max(1) <= np.where(inside, glob, np.inf).min(1) + RANK_GAP).all()
        assert np.abs(cos.cpu().numpy() - np.take_along_axis(glob, sl, 1)).max() < SCORE_TOL
        ids, scores = _search(g11, k=10, shortlist=S)
        all_ids, all_scores = _search(g11, k=S, shortlist=S)
        assert torch.equal(ids, all_ids[:, :10]) and torch.equal(scores, all_scores[:, :10])       # k = 10 is the head of k = S
        ids, scores, all_ids = ids.cpu().numpy(), scores.cpu().numpy(), all_ids.cpu().numpy()
        assert np.array_equal(np.sort(all_ids, axis=1), sl)                               # the re-ranked set IS the cosine shortlist
        assert np.abs(scores - np.take_along_axis(full, ids, 1)).max() < SCORE_TOL
        assert _ordered(ids, scores) and _ordered(all_ids, all_scores.cpu().numpy())

    def test_state_dict_round_trip_modes_and_chunks(self, g11, tmp_path):
        ix, model, loss = g11["index"], g11["model"], g11["loss"]
        ref = _search(g11, k=10, shortlist=32)
        torch.save(ix.state_dict(), tmp_path / "captions.pt")
        back = search.CaptionIndex(ix.capacity, ix.W, torch.bfloat16, DEV).load_state_dict(torch.load(tmp_path / "captions.pt"))
        assert len(back) == len(ix)
        for name in ("gn", "tm", "local"):
            assert torch.equal(_bits(getattr(back, name)), _bits(getattr(ix, name))), name
        got = _search(g11, back, k=10, shortlist=32)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))
        with pytest.raises(ValueError):
            search.CaptionIndex(ix.capacity + 1, ix.W, torch.bfloat16, DEV).load_state_dict(ix.state_dict())
        for chunk in (64, 100, 65536):                                                    # divides / does not divide the 256 rows / one product
            got = _search(g11, k=10, shortlist=32, chunk=chunk)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32)), chunk
        model.train()
        try:
            got = _search(g11, k=10, shortlist=32)
            assert model.training and not got[1].requires_grad and got[1].grad_fn is None
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))
            other = search.CaptionIndex(ix.capacity, ix.W, torch.bfloat16, DEV).add_batches(model, g11["batches"][:1])
            assert model.training and len(other) == g11["batches"][0]["object"].shape[0]
            model.eval()
            ix.search(model, loss, _videos(g11["batches"][0]), k=3, shortlist=8)
            assert not model.training
        finally:
            model.eval()
        with pytest.raises(ValueError, match="W = 99"):
            with torch.no_grad():
                gt, lt = model.compute_text(g11["batches"][0]["text"])
            ix.add(gt, lt[:, :-1].contiguous(), g11["batches"][0]["text"]["attention_mask"][:, :-1])

    def test_evaluate_v2t_with_a_full_shortlist_equals_the_metrics_of_the_full_grid(self, g11):
        keys = ("R1", "R10", "MedR")
        r = search.evaluate_v2t(g11["model"], g11["loss"], g11["batches"], shortlist=None)
        assert set(r) == {"v2t_metrics", "sims"} and r["sims"].shape == (g11["n"], g11["n"])
        assert np.abs(r["sims"] - g11["full"].T).max() < SCORE_TOL                        # text x video, as metric.v2t_metrics expects
        want = metric.v2t_metrics(g11["full"].T)
        print("\nsearch orientation v2t:", {k: r["v2t_metrics"][k] for k in keys}, "| full grid:", {k: want[k] for k in keys})
        assert abs(r["v2t_metrics"]["R1"] - want["R1"]) <= 100.0 * 3 / g11["n"]           # (a 2e-5 deviation can move a tied rank or two)
        part = search.evaluate_v2t(g11["model"], g11["loss"], g11["batches"], shortlist=64)
        print("shortlist 64 v2t:", {k: part["v2t_metrics"][k] for k in keys})            # recall here is a property of the synthetic weights: printed only

    def test_search_with_ground_returns_the_search_and_what_ground_returns(self, g11):
        ix, model, loss, F, R, W = g11["index"], g11["model"], g11["loss"], g11["F"], g11["R"], g11["W"]
        local = g11["res"]["local_sims"]                                                  # [video, caption], the fused full grid's fp32 values
        BS = g11["batches"][0]["object"].shape[0]
        for nb, b in enumerate(g11["batches"][:2]):
            data = _videos(b)
            ids0, scores0 = ix.search(model, loss, data, k=5)
            res = ix.search(model, loss, data, k=5, ground=True, frames=F)
            assert len(res) == 3
            ids, scores, gr = res
            assert torch.equal(ids, ids0) and torch.equal(scores.view(torch.int32), scores0.view(torch.int32))
            assert gr["score"].shape == (BS, 5) and gr["word_scores"].shape == (BS, 5, W) and gr["region_scores"].shape == (BS, 5, F * R)
            assert gr["frame_scores"].shape == (BS, 5, F) and gr["word_frame"].shape == (BS, 5, W) and all(v.is_cuda for v in gr.values())
            # its score is the local addend, bit for bit: what the score kernel gives for these pairs ...
            with torch.no_grad():
                go, lo, om = ix._video_side(model, data)
                addend = ix._local_stage(loss.local_loss, lo, om, ids.int().contiguous())
            assert torch.equal(gr["score"].view(torch.int32), addend.view(torch.int32))
            all_ids, cos = ix.shortlist_by_cosine(go, None)
            assert torch.equal(all_ids, torch.arange(len(ix), device=DEV).expand(BS, -1))
            dev = float((gr["score"] + torch.gather(cos, 1, ids) - scores).abs().max())
            print("\nmax |grounding score + cosine - search score| %.2e" % dev)
            assert dev <= 1e-6
            # ... which is the entry of the full grid trainer.evaluate computed
            want =np.take_along_axis(local[nb * BS:(nb + 1) * BS], ids.cpu().numpy(), 1)
            assert np.array_equal(gr["score"].cpu().numpy().astype(np.float64), want.astype(np.float64))
            _same_bytes(ix.ground(model, loss, data, ids, frames=F), gr)
            assert gr["word_valid"].dtype == torch.bool and gr["word_valid"].shape == (BS, 5, W)
            assert torch.equal(gr["word_valid"], (g11["att"][:, 1:] > 0)[ids])            # the stored masks, gathered per (video, k)
            assert torch.equal(gr["word_frame"], gr["word_region"] // R) and int(gr["word_frame"].max()) < F and int(gr["word_frame"].min()) >= 0
            assert not model.training
        model.train()
        try:
            again = ix.ground(model, loss, data, ids.int(), frames=F)
            assert model.training and not again["score"].requires_grad
            _same_bytes(again, gr)
        finally:
            model.eval()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. parity route (fp32): against the fp64 oracle, the bar of tests/test_gpu_search.py::TestParityRoute
# ---------------------------------------------------------------------------------------------------------------------------------------
class TestCaptionParityRoute:
    def test_fp32_scores_within_1e5_of_the_fp64_oracle(self):
        F, R, N, NV, S, K = 8, 30, 12, 6, 5, 3
        sd = syn.retrieval_state_dict(F, R)
        model = _retrieval_model(F, R, sd, "float32")
        loss = GlobalLocalLoss(**LOSS)
        batches = list(_retrieval_batches(sd, F, R, 6, N // 6))
        W = batches[0]["text"]["input_ids"].shape[1] - 1
        ix = search.CaptionIndex(N + 2, W, torch.float32, DEV)
        assert not ix.fused
        ix.add_batches(model, batches[:1])
        with torch.no_grad():
            out = model.eval()(batches[1], return_embeds=True)
        ix.add(out["global_text_embeddings"], out["local_text_embeddings"], batches[1]["text"]["attention_mask"])      # the tensor route
        assert len(ix) == N
        with pytest.raises(ValueError):
            ix.add_batches(model, batches[:1])                                            # 12 + 6 > 14
        data = {k: v[:NV] for k, v in _videos(batches[0]).items()}
        ids, scores = ix.search(model, loss, data, k=K, shortlist=S)
        with pytest.raises(DemoVLPHipError):
            ix.ground(model, loss, data, ids)
        with torch.no_grad():
            embeds = [model(b, return_embeds=True) for b in batches]
        gt = torch.cat([e["global_text_embeddings"] for e in embeds]).cpu().double()
        lt = torch.cat([e["local_text_embeddings"] for e in embeds]).cpu().double()
        tm = ((torch.cat([b["text"]["attention_mask"] for b in batches])[:, 1:] - 1.0) * 100.0).cpu().double()
        go = embeds[0]["global_object_embeddings"][:NV].cpu().double()
        lo = embeds[0]["local_object_embeddings"][:NV].cpu().double()
        om = embeds[0]["object_mask"][:NV].cpu().double()
        unit = lambda a: a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
        cos = unit(go) @ unit(gt).T
        err = 0.0
        for i in range(NV):
            for p in range(K):
                j = int(ids[i, p])
                want = float(orc.xattn_pair(lo[i], lt[j], om[i], tm[j], 20.0, True)) + float(cos[i, j])
                err = max(err, abs(float(scores[i, p]) - want))
        print("\ncaption parity route: max |score - fp64 oracle| %.2e" % err)
        assert err < 1e-5, err
        assert _ordered(ids.cpu().numpy(), scores.cpu().numpy())
