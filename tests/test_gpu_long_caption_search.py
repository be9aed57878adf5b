"""Video-to-text search and grounding for long videos on a real MI355X (product library): the region-tiled pair kernel on the video-major
grid over a resident caption index (``dvlp_xattn_long_caption_index_*``).

What is checked, and against what:
  * bit-equality with the query-major tiled kernel (``dvlp_xattn_long_index_*``) on the same pairs, scores and every grounding row: the
    per-pair code is shared, contraction is off for it, and a prepared row's bytes do not depend on the call that wrote it;
  * the fp64 oracle ``xattn_pair`` on the bf16-rounded inputs under ``SCORE_BAR = 2e-3``, the project's bar for the pair kernels against
    this oracle on this recipe (``tests/test_gpu_long_search.py``);
  * the fused caption-index kernel inside its range (G <= 288) on the same index bytes, under the same 2e-3 (the two kernels sum the
    softmax numerators in different orders: DESIGN.md 6g);
  * ``CaptionIndex(..., tiled=True)`` end to end against ``VideoIndex(..., tiled=True)``: the search scores of the same pair within
    ``SCORE_TOL = 2e-5`` of ``tests/test_gpu_caption_search.py`` (the two cosine products may sum in a different order), the local addends
    bit for bit.  No ranking condition is asserted.

Inputs: ``_inputs`` of ``tests/test_gpu_long_search.py`` (correlated leading channels, a masked video tail, ragged captions)."""
import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, functional as Fn, ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss
from oracle import restatement as orc
from test_gpu_long_search import _filled as _video_index, _inputs, _retrieval_model, _same_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAM = 20.0
SCORE_BAR = 2e-3
SCORE_TOL = 2e-5
#          G     W    frames (a divisor of G where G has one worth the name)
SHAPES = [(1, 99, None),      # single region
          (129, 7, 3),        # one region past a 128-region tile
          (289, 37, 17),      # first G out of the fused range, ragged 16-row block
          (1152, 99, 32),     # top of the range: 32 frames x 36 regions
          (1152, 1, 32)]      # single word
GATES = [True, False]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _caption_index(Q, capacity, splits):
    W = Q.shape[1]
    index = torch.zeros(ops.xattn_caption_index_bytes(capacity, W), device=DEV, dtype=torch.uint8)
    r0 = 0
    for n in splits:
        ops.xattn_caption_index_add(index, capacity, W, r0, Q[r0:r0 + n].contiguous())
        r0 += n
    return index


def _pad_rows(m, capacity):
    return torch.cat([m, torch.zeros(capacity - m.shape[0], m.shape[1], device=DEV)])


def _cand(Bi, Bj, K, seed):
    cand = np.random.default_rng(seed).integers(0, Bj, (Bi, K)).astype(np.int32)
    cand[0, -1] = cand[0, 0]                                              # a repeated candidate in a row
    return cand


def _grid(rows, n):
    return torch.arange(n, device=DEV, dtype=torch.int32).expand(rows, -1).contiguous()


class TestBitEqualToTheQueryMajorTiledKernel:
    @pytest.mark.parametrize("G,W,frames", SHAPES)
    @pytest.mark.parametrize("gate", GATES)
    def test_scores_and_grounding_rows(self, G, W, frames, gate):
        Bi, Bj, cap, K = 3, 4, 6, 5
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 4000 + G + W)
        cidx, mc6 = _caption_index(Q, cap, [Bj]), _pad_rows(mc, cap)
        cand = _cand(Bi, Bj, K, G + W)
        cand_d = torch.from_numpy(cand).to(DEV)
        vidx = _video_index(C, Bi, [Bi])
        # the query-major kernel on every (caption, video) pair, from a video index of the same videos
        ref = ops.xattn_long_index_pairs_fwd(vidx, Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, gate)                     # [Bj, Bi]
        ref_g = ops.xattn_long_index_pairs_ground(vidx, Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, gate, frames=frames)  # [Bj, Bi, ...]
        got = ops.xattn_long_caption_index_pairs_fwd(cidx, cap, W, mc6, C, mi, cand_d, LAM, gate)
        assert got.shape == (Bi, K) and got.dtype == torch.float32 and torch.isfinite(got).all()
        rows = torch.arange(Bi, device=DEV)[:, None].expand(Bi, K)
        want = ref[cand_d.long(), rows]                                   # want[i, k] = ref[cand[i, k], i]
        assert torch.equal(_bits(got), _bits(want)), float((got - want).abs().max())
        assert _bits(got)[0, -1] == _bits(got)[0, 0]
        gr = ops.xattn_long_caption_index_pairs_ground(cidx, cap, W, mc6, C, mi, cand_d, LAM, gate, frames=frames)
        assert ("frame_scores" in gr) == (frames is not None)
        assert torch.equal(_bits(gr["score"]), _bits(got))
        _same_bytes(gr, {name: t[cand_d.long(), rows] for name, t in ref_g.items()})


class TestAgainstTheOracle:
    @staticmethod
    def _check(C, Q, mi, mc, gate, tag):
        cand = torch.tensor([[0, 1], [1, 0]], device=DEV, dtype=torch.int32)
        got = ops.xattn_long_caption_index_pairs_fwd(_caption_index(Q, 2, [2]), 2, Q.shape[1], mc, C, mi, cand, LAM, gate).cpu().numpy()
        c, q, a, b = C.cpu().double(), Q.cpu().double(), mi.cpu().double(), mc.cpu().double()
        ref = np.array([[float(orc.xattn_pair(c[i], q[j], a[i], b[j], LAM, gate)) for j in cand[i].tolist()] for i in range(2)])
        assert np.isfinite(got).all() and np.isfinite(ref).all(), tag
        dev = float(np.abs(got - ref).max())
        print("\n%-44s max |score - fp64| %.3e" % (tag, dev))
        assert dev <= SCORE_BAR, (tag, dev)

    @pytest.mark.parametrize("G,W", [(289, 37), (1152, 99)])
    @pytest.mark.parametrize("gate", GATES)
    def test_scores_within_2e3_of_the_fp64_oracle(self, G, W, gate):
        self._check(*_inputs(2, 2, G, W, 6000 + G + W), gate, "G = %d, W = %d, gate %s" % (G, W, gate))

    @pytest.mark.parametrize("gate", GATES)
    def test_whole_tiles_of_masked_regions(self, gate):
        """video 0: the last 200 regions masked (the last tile holds masked regions only); video 1: the first 130 (the first tile, and two
        regions of the second)"""
        G = 1152
        C, Q, mi, mc = _inputs(2, 2, G, 99, 77)
        mi.zero_()
        mi[0, G - 200:] = -100.0
        mi[1, :130] = -100.0
        self._check(C, Q, mi, mc, gate, "G = 1152, W = 99, masked tiles, gate %s" % gate)


class TestInsideTheFusedRange:
    @pytest.mark.parametrize("G", [240, 288])
    @pytest.mark.parametrize("gate", GATES)
    def test_within_2e3_of_the_fused_caption_index_kernel_on_the_same_bytes(self, G, gate):
        Bi, Bj, W, K = 3, 4, 99, 5
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 700 + G)
        cidx = _caption_index(Q, Bj, [Bj])
        cand = torch.from_numpy(_cand(Bi, Bj, K, G)).to(DEV)
        want = ops.xattn_caption_index_pairs_fwd(cidx, Bj, W, mc, C, mi, cand, LAM, gate)
        got = ops.xattn_long_caption_index_pairs_fwd(cidx, Bj, W, mc, C, mi, cand, LAM, gate)
        dev = float((got - want).abs().max())
        print("\nG = %d, gate %s: max |tiled - fused| %.3e" % (G, gate, dev))
        assert torch.isfinite(got).all() and dev <= SCORE_BAR, dev


class TestHoles:
    def test_out_of_range_candidates_give_nan_and_minus_one_and_leave_the_others(self):
        Bi, Bj, cap, G, W, K = 3, 4, 6, 304, 99, 5
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5)
        cidx, mc6 = _caption_index(Q, cap, [Bj]), _pad_rows(mc, cap)          # capacity 6: rows 4, 5 were never added
        cand = _cand(Bi, Bj, K, 1)
        args = (cidx, cap, W, mc6, C, mi)
        good = ops.xattn_long_caption_index_pairs_fwd(*args, torch.from_numpy(cand).to(DEV), LAM, True)
        again = ops.xattn_long_caption_index_pairs_fwd(*args, torch.from_numpy(cand).to(DEV), LAM, True)
        assert torch.isfinite(good).all() and torch.equal(_bits(good), _bits(again))
        good_g = ops.xattn_long_caption_index_pairs_ground(*args, torch.from_numpy(cand).to(DEV), LAM, True, frames=8)
        _same_bytes(ops.xattn_long_caption_index_pairs_ground(*args, torch.from_numpy(cand).to(DEV), LAM, True, frames=8), good_g)
        bad = cand.copy()
        bad[1, 2], bad[2, 0], bad[2, 4] = -1, cap, 2 ** 31 - 1
        hole = torch.from_numpy(bad != cand).to(DEV)
        got = ops.xattn_long_caption_index_pairs_fwd(*args, torch.from_numpy(bad).to(DEV), LAM, True)
        assert int(hole.sum()) == 3 and torch.isnan(got[hole]).all()
        assert torch.equal(_bits(got[~hole]), _bits(good[~hole]))
        gr = ops.xattn_long_caption_index_pairs_ground(*args, torch.from_numpy(bad).to(DEV), LAM, True, frames=8)
        for name in ("score", "word_scores", "region_scores", "word_region_weight", "frame_scores"):
            assert torch.isnan(gr[name][hole]).all(), name
            assert torch.equal(_bits(gr[name][~hole]), _bits(good_g[name][~hole])), name
        for name in ("word_region", "region_word"):
            assert (gr[name][hole] == -1).all() and torch.equal(gr[name][~hole], good_g[name][~hole]), name

    def test_forward_only(self):
        C, Q, mi, mc = _inputs(2, 3, 30, 20, 1)
        C.requires_grad_(True)
        s = Fn.XattnLongCaptionIndexPairsFn.apply(_caption_index(Q, 3, [3]), 3, 20, mc, C, mi, torch.zeros(2, 3, device=DEV, dtype=torch.int32), LAM,
                                                  True)
        with pytest.raises(DemoVLPHipError):
            s.sum().backward()


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: F = 10, R = 30 (G = 300, just out of the fused range), 12 (video, caption) pairs in two batches of 6
# ---------------------------------------------------------------------------------------------------------------------------------------
def _videos(b):
    return {"object": b["object"], "object_mask": b["object_mask"]}


def _matrix(ids, scores, n):
    m = torch.full((n, n), float("nan"), device=DEV)
    m.scatter_(1, ids, scores)
    return m


@pytest.fixture(scope="module")
def e2e():
    F, R, N = 10, 30, 12
    sd = syn.retrieval_state_dict(F, R)
    model = _retrieval_model(F, R, sd, "bfloat16")
    loss = GlobalLocalLoss(use_local=True, use_global=True, coef=1.0, focal_type="equal")
    batches = []
    for b in range(N // 6):
        obj, mask, ids, att = syn.retrieval_batch(sd, F, R, b * 6, 6)
        batches.append({"text": {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(att).to(DEV)},
                        "object": torch.from_numpy(obj).to(DEV), "object_mask": torch.from_numpy(mask).to(DEV)})
    W = batches[0]["text"]["input_ids"].shape[1] - 1
    cix = search.CaptionIndex(N, W, torch.bfloat16, DEV, tiled=True).add_batches(model, batches)
    vix = search.VideoIndex(N, F * R, torch.bfloat16, DEV, tiled=True).add_batches(model, batches)
    return dict(model=model, loss=loss, batches=batches, cix=cix, vix=vix, F=F, R=R, N=N, W=W)


class TestTiledCaptionIndex:
    def test_three_adds_are_byte_equal_to_one_and_to_a_non_tiled_index(self, e2e):
        model, batches, N, W = e2e["model"], e2e["batches"], e2e["N"], e2e["W"]
        with torch.no_grad():
            sides = [model.eval().compute_text(b["text"]) for b in batches]
        gt, lt = torch.cat([s[0] for s in sides]), torch.cat([s[1] for s in sides])
        att = torch.cat([b["text"]["attention_mask"] for b in batches])
        one = search.CaptionIndex(N + 2, W, torch.bfloat16, DEV, tiled=True)
        one.add(gt, lt, att)
        three = search.CaptionIndex(N + 2, W, torch.bfloat16, DEV, tiled=True)
        for r0, n in ((0, 5), (5, 4), (9, 3)):
            three.add(gt[r0:r0 + n], lt[r0:r0 + n], att[r0:r0 + n])
        plain = search.CaptionIndex(N + 2, W, torch.bfloat16, DEV)
        plain.add(gt, lt, att)
        assert len(one) == len(three) == len(plain) == N and one.tiled and one.fused and not plain.tiled
        assert one.local.numel() == ops.xattn_caption_index_bytes(N + 2, W)
        for name in ("gn", "tm", "local"):
            assert torch.equal(getattr(one, name), getattr(three, name)) and torch.equal(getattr(one, name), getattr(plain, name)), name

    def test_state_dict_round_trip_and_route_mismatch(self, e2e, tmp_path):
        cix, model, loss, N, W = e2e["cix"], e2e["model"], e2e["loss"], e2e["N"], e2e["W"]
        state = cix.state_dict()
        plain = search.CaptionIndex(N, W, torch.bfloat16, DEV)
        assert state["tiled"] is True and "tiled" not in plain.state_dict()
        torch.save(state, tmp_path / "captions.pt")
        fresh = search.CaptionIndex(N, W, torch.bfloat16, DEV, tiled=True).load_state_dict(torch.load(tmp_path / "captions.pt"))
        assert len(fresh) == N
        for name in ("gn", "tm", "local"):
            assert torch.equal(getattr(fresh, name), getattr(cix, name)), name
        data = _videos(e2e["batches"][0])
        a, b = cix.search(model, loss, data, k=3, shortlist=5), fresh.search(model, loss, data, k=3, shortlist=5)
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))
        with pytest.raises(ValueError, match="route"):
            plain.load_state_dict(state)
        with pytest.raises(ValueError, match="route"):
            search.CaptionIndex(N, W, torch.bfloat16, DEV, tiled=True).load_state_dict(plain.state_dict())

    def test_search_with_ground_and_frames(self, e2e):
        cix, model, loss, F, R, W = e2e["cix"], e2e["model"], e2e["loss"], e2e["F"], e2e["R"], e2e["W"]
        data = _videos(e2e["batches"][0])
        ids0, scores0 = cix.search(model, loss, data, k=3, shortlist=5)
        ids, scores, gr = cix.search(model, loss, data, k=3, shortlist=5, ground=True, frames=F)
        assert torch.equal(ids, ids0) and torch.equal(_bits(scores), _bits(scores0))
        assert gr["word_frame"].shape == (6, 3, W) and int(gr["word_frame"].min()) >= 0 and int(gr["word_frame"].max()) < F
        assert torch.equal(gr["word_frame"], gr["word_region"] // R) and gr["frame_scores"].shape == (6, 3, F)
        assert gr["region_scores"].shape == (6, 3, F * R) and gr["word_valid"].shape == (6, 3, W) and torch.isfinite(gr["score"]).all()
        _same_bytes(cix.ground(model, loss, data, ids, frames=F), gr)
        # a plain bf16 index still refuses these videos (G = 300 is beyond the fused kernel)
        plain = search.CaptionIndex(e2e["N"], W, torch.bfloat16, DEV).add_batches(model, e2e["batches"])
        with pytest.raises(DemoVLPHipError, match="beyond the fused kernel's range"):
            plain.search(model, loss, data, k=3, shortlist=5)

    def test_exact_search_is_the_transpose_of_tiled_text_to_video_search(self, e2e):
        cix, vix, model, loss, batches, N = e2e["cix"], e2e["vix"], e2e["model"], e2e["loss"], e2e["batches"], e2e["N"]
        v2t = [cix.search(model, loss, _videos(b), k=N, shortlist=None) for b in batches]
        t2v = [vix.search(model, loss, b["text"], k=N, shortlist=None) for b in batches]
        b_m = _matrix(torch.cat([p[0] for p in v2t]), torch.cat([p[1] for p in v2t]), N).cpu().numpy().astype(np.float64)      # [video, caption]
        a_m = _matrix(torch.cat([p[0] for p in t2v]), torch.cat([p[1] for p in t2v]), N).cpu().numpy().astype(np.float64)      # [caption, video]
        assert np.isfinite(a_m).all() and np.isfinite(b_m).all()
        dev = float(np.abs(b_m - a_m.T).max())
        print("\nmax |v2t score - t2v score of the same pair| %.2e" % dev)
        assert dev < SCORE_TOL, dev
        # the local addends: bit for bit
        every = torch.arange(N, device=DEV).expand(6, -1).contiguous()
        lv = torch.cat([cix.ground(model, loss, _videos(b), every)["score"] for b in batches])                            # [video, caption]
        lt = torch.cat([vix.ground(model, loss, b["text"], every)["score"] for b in batches])                             # [caption, video]
        assert torch.isfinite(lv).all() and torch.equal(_bits(lv), _bits(lt.t()))
        # evaluate_v2t(tiled=True): the same matrix, text x video
        r = search.evaluate_v2t(model, loss, batches, shortlist=None, tiled=True)
        assert set(r) == {"v2t_metrics", "sims"} and r["sims"].shape == (N, N)
        assert np.array_equal(r["sims"], b_m.T)
