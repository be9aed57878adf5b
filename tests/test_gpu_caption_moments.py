"""Moment search in the video-to-text direction on a real MI355X (product library): ``dvlp_xattn_long_caption_index_moments_fwd`` (DESIGN.md
6j), where one workgroup stages its caption once and walks a chunk of the windows of its pair, and ``CaptionIndex.moments`` /
``search(..., moments=...)`` / ``timeline`` on top of it.

What is checked, and against what:
  * bit-equality with the other direction (``dvlp_xattn_long_index_moments_fwd`` on a video index of the same videos) for every window of
    every pair: the per-window code is shared and contraction is off for it;
  * the fp64 oracle ``xattn_pair`` on the bf16-rounded SLICE of the query video under ``SCORE_BAR = 2e-3``, the bar of this kernel family
    against this oracle (``tests/test_gpu_long_search.py``); the maxima are printed and recorded in DESIGN.md 6j.  As in
    ``tests/test_gpu_moments.py`` two kinds of window have no oracle value: gate on and a one-region window (or W = 1), where the oracle is
    0 / 0 and a finite value is asserted, and a window without an unmasked region, which must be exactly -inf;
  * that neither the chunking (``windows_per_group``) nor the layout (``window_major``) changes a byte, also when a live window follows an
    empty one in the same workgroup;
  * the whole-video kernel at ``win = frames``, garbage in the neighbouring frames, holes and repeats in the candidate list;
  * ``timeline`` on a planted pair of captions (the oracle decides first) and against a brute-force ranking of ``moments``.

Inputs: ``tests/test_gpu_long_search.py::_inputs`` (correlated channels, video 1 with a masked tail, ragged captions), Bi = 3, Bj = 2, both
gates, unless stated."""
import numpy as np
import pytest
import torch

from demovlp_amd import ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from test_gpu_long_search import GATES, LAM, SCORE_BAR, _filled, _grid, _inputs, _retrieval_model, _same_bytes
from test_gpu_moments import SHAPES, _check_windows, _empty_windows, _oracle_windows, _planted

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _caption_index(Q, capacity=None):
    n, W = Q.shape[:2]
    index = torch.zeros(ops.xattn_caption_index_bytes(capacity or n, W), device=DEV, dtype=torch.uint8)
    ops.xattn_caption_index_add(index, capacity or n, W, 0, Q)
    return index


def _pad_rows(m, capacity):
    return torch.cat([m, torch.zeros(capacity - m.shape[0], m.shape[1], device=DEV)])


def _cmoments(C, Q, mi, mc, F, win, stride, gate, cand=None, capacity=None, **kw):
    """the new entry on a caption index of Q; by default every caption for every video -> [Bi, Bj, M]"""
    cap = capacity or Q.shape[0]
    cand = _grid(C.shape[0], Q.shape[0]) if cand is None else cand
    return ops.xattn_long_caption_index_moments_fwd(_caption_index(Q, cap), cap, Q.shape[1], _pad_rows(mc, cap), C, mi, cand, F, win, stride, LAM,
                                                    gate, **kw)


class TestBitEqualToTheOtherDirection:
    @pytest.mark.parametrize("G,F,W,win,stride", SHAPES)
    @pytest.mark.parametrize("gate", GATES)
    def test_every_window_of_every_pair(self, G, F, W, win, stride, gate):
        Bi, Bj = 3, 2
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 3000 + G + W)
        ref = ops.xattn_long_index_moments_fwd(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, _grid(Bj, Bi), F, win, stride, LAM, gate)      # [Bj, Bi, M]
        cand = torch.tensor([[0, 1, 0], [1, 0, 1], [1, 1, 0]], device=DEV, dtype=torch.int32)
        got = _cmoments(C, Q, mi, mc, F, win, stride, gate, cand)
        M = (F - win) // stride + 1
        assert got.shape == (Bi, 3, M) and got.dtype == torch.float32 and ref.shape == (Bj, Bi, M)
        want = ref[cand.long(), torch.arange(Bi, device=DEV)[:, None].expand(Bi, 3)]            # want[i, k, m] = ref[cand[i, k], i, m]
        assert torch.equal(_bits(got), _bits(want)), float((got - want).abs().max())


class TestAgainstTheOracle:
    @pytest.mark.parametrize("G,F,W,win,stride", SHAPES)
    @pytest.mark.parametrize("gate", GATES)
    def test_every_window_within_2e3_of_the_fp64_oracle_on_the_slice(self, G, F, W, win, stride, gate):
        Bi, Bj = 3, 2
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 3000 + G + W)
        got = _cmoments(C, Q, mi, mc, F, win, stride, gate)                                     # [Bi, Bj, M]
        assert got.shape == (Bi, Bj, (F - win) // stride + 1)
        ref = _oracle_windows(C, Q, mi, mc, F, win, stride, gate)                               # [Bj, Bi, M]
        empty = _empty_windows(mi, F, win, stride)
        assert not empty.any() or G // F == 1                               # only the R = 1 shape has windows inside the masked tail
        _check_windows(got.permute(1, 0, 2), ref, empty, gate and (win * (G // F) == 1 or W == 1),
                       "v2t G = %d, F = %d, W = %d, win = %d, stride = %d, gate %s" % (G, F, W, win, stride, gate))


class TestChunkingAndLayout:
    @pytest.mark.parametrize("G,F,W,win,stride", [(1152, 32, 99, 8, 4), (300, 10, 37, 3, 1)])
    @pytest.mark.parametrize("gate", GATES)
    def test_no_byte_depends_on_them(self, G, F, W, win, stride, gate):
        C, Q, mi, mc = _inputs(3, 2, G, W, 8100 + G)
        M = (F - win) // stride + 1
        one = _cmoments(C, Q, mi, mc, F, win, stride, gate, windows_per_group=1)
        assert one.shape == (3, 2, M) and torch.isfinite(one).all()
        for n in (2, 3, M, M + 5, 0):
            assert torch.equal(_bits(_cmoments(C, Q, mi, mc, F, win, stride, gate, windows_per_group=n)), _bits(one)), n
        for n in (1, 3, 0):
            major = _cmoments(C, Q, mi, mc, F, win, stride, gate, windows_per_group=n, window_major=True)
            assert major.shape == (3, M, 2) and torch.equal(_bits(major), _bits(one.transpose(1, 2))), n
        assert torch.equal(_bits(_cmoments(C, Q, mi, mc, F, win, stride, gate)), _bits(_cmoments(C, Q, mi, mc, F, win, stride, gate)))      # two runs


class TestMasks:
    @pytest.mark.parametrize("gate", GATES)
    def test_a_live_window_after_an_empty_one_in_the_same_workgroup(self, gate):
        Bi, Bj, G, F, W, win = 3, 2, 300, 10, 37, 2
        R, M = G // F, F - win + 1
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 6300)
        mi[2, 2 * R:4 * R] = -100.0                                        # video 2: frames 2..3 fully masked
        got = _cmoments(C, Q, mi, mc, F, win, 1, gate, windows_per_group=M)
        empty = _empty_windows(mi, F, win, 1)
        assert empty.sum() == 1 and empty[2, 2]
        assert torch.isneginf(got[2, :, 2]).all()
        assert torch.equal(_bits(got), _bits(_cmoments(C, Q, mi, mc, F, win, 1, gate, windows_per_group=1)))
        # the windows after the empty one (and the partly masked ones: frames 1..2 and 3..4 of video 2, the tail of video 1) stay within the bar
        _check_windows(got.permute(1, 0, 2), _oracle_windows(C, Q, mi, mc, F, win, 1, gate), empty, False,
                       "v2t G = 300, frames 2..3 of video 2 masked, one workgroup per pair, gate %s" % gate)


class TestWholeVideo:
    @pytest.mark.parametrize("G,F,W", [(1152, 32, 99), (300, 10, 37)])
    @pytest.mark.parametrize("gate", GATES)
    def test_a_window_of_all_frames_is_bit_equal_to_the_pair_kernel(self, G, F, W, gate):
        Bi, Bj = 3, 2
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5200 + G)
        got = _cmoments(C, Q, mi, mc, F, F, 1, gate)
        want = ops.xattn_long_caption_index_pairs_fwd(_caption_index(Q), Bj, W, mc, C, mi, _grid(Bi, Bj), LAM, gate)
        assert got.shape == (Bi, Bj, 1) and torch.isfinite(want).all()
        assert torch.equal(_bits(got[:, :, 0]), _bits(want)), float((got[:, :, 0] - want).abs().max())


class TestNeighboursDoNotLeak:
    @pytest.mark.parametrize("G,F,W,f0,f1", [(300, 10, 37, 3, 5), (1152, 32, 99, 12, 19)])
    @pytest.mark.parametrize("gate", GATES)
    def test_garbage_outside_the_window_changes_no_byte(self, G, F, W, f0, f1, gate):
        Bi, Bj, R, win = 3, 2, G // F, f1 - f0 + 1
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 4100 + G)
        dirty = C.clone()
        outside = torch.ones(G, dtype=torch.bool, device=DEV)
        outside[f0 * R:(f1 + 1) * R] = False
        gen = torch.Generator(device="cpu").manual_seed(G)
        dirty[:, outside] = (1e4 * torch.randn(Bi, int(outside.sum()), 256, generator=gen)).to(DEV).bfloat16()
        clean = _cmoments(C, Q, mi, mc, F, win, 1, gate)
        other = _cmoments(dirty, Q, mi, mc, F, win, 1, gate)
        assert torch.isfinite(clean[:, :, f0]).all()
        assert torch.equal(_bits(clean[:, :, f0]), _bits(other[:, :, f0]))
        assert not torch.equal(_bits(clean), _bits(other))                  # (the garbage is seen by the windows that hold it)


def _caption_ix(Q, mc, capacity=None):
    """a tiled ``CaptionIndex`` of the captions Q with the additive masks mc (the global embeddings do not matter to moments)"""
    n, W = Q.shape[:2]
    ix = search.CaptionIndex(capacity or n, W, torch.bfloat16, DEV, tiled=True)
    att = torch.cat([torch.ones(n, 1, device=DEV), (mc == 0).float()], 1)  # tm = (att - 1) * 100 = mc
    ix.add(torch.ones(n, 256, device=DEV, dtype=torch.bfloat16), Q, att)
    assert torch.equal(ix.tm[:n], mc)
    return ix


def _block(ix, C, mi, ids, F, windows, stride=1, gate=True):
    return ix._moments_block(RWALoss(LAM, "equal" if gate else "prob"), (None, C, mi), ids, F, ix._moment_checks(F, windows, stride, C.shape[1]),
                             stride)


class TestMechanics:
    def test_bad_and_repeated_candidates_in_both_layouts(self):
        Bi, Bj, G, F, W, K, win, cap = 3, 4, 300, 10, 37, 5, 3, 6
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 7)
        ix = _caption_ix(Q, mc, capacity=cap)                                 # capacity 6: rows 4, 5 were never added
        cand = np.random.default_rng(1).integers(0, Bj, (Bi, K)).astype(np.int32)
        cand[0, -1] = cand[0, 0]                                              # a repeated candidate in a row
        dev = lambda a: torch.from_numpy(a).to(DEV)
        run = lambda c, **kw: ops.xattn_long_caption_index_moments_fwd(ix.local, cap, W, ix.tm, C, mi, dev(c), F, win, 1, LAM, True, **kw)
        good = run(cand)
        assert good.shape == (Bi, K, 8) and torch.isfinite(good).all() and torch.equal(_bits(good[0, -1]), _bits(good[0, 0]))
        bad = cand.copy()
        bad[1, 2], bad[2, 0], bad[2, 4] = -1, cap, 2 ** 31 - 1
        hole = dev(bad != cand)
        assert int(hole.sum()) == 3
        for n in (0, 1, 3, 8):
            got = run(bad, windows_per_group=n)
            assert torch.isnan(got[hole]).all() and torch.equal(_bits(got[~hole]), _bits(good[~hole])), n
            major = run(bad, windows_per_group=n, window_major=True)
            assert major.shape == (Bi, 8, K) and torch.isnan(major.transpose(1, 2)[hole]).all(), n
            assert torch.equal(_bits(major.transpose(1, 2)[~hole]), _bits(good[~hole])), n
        out = _block(ix, C, mi, dev(bad), F, win, 1, True)
        assert torch.equal(_bits(out["scores"][~hole]), _bits(good[~hole])) and torch.isnan(out["scores"][hole]).all()
        for name in ("best", "best_start", "best_length"):
            assert out[name].dtype == torch.int64 and (out[name][hole] == -1).all() and (out[name][~hole] >= 0).all(), name
        assert torch.isnan(out["best_score"][hole]).all() and torch.isfinite(out["best_score"][~hole]).all()

    def test_several_window_lengths_and_the_tie_rule(self):
        Bi, Bj, G, F, W = 3, 2, 300, 10, 37
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 8)
        ix = _caption_ix(Q, mc)
        windows, stride = (3, 10, 3, 1), 2                                    # a repeated length: its windows tie with their first copies
        out = _block(ix, C, mi, _grid(Bi, Bj), F, windows, stride, True)
        per = [_cmoments(C, Q, mi, mc, F, w, stride, True) for w in windows]
        assert [p.shape[2] for p in per] == [4, 1, 4, 5]
        scores = torch.cat(per, 2)
        assert torch.equal(_bits(out["scores"]), _bits(scores))
        starts, lengths = search.moment_windows(F, windows, stride)
        assert torch.equal(out["start"].cpu(), starts) and torch.equal(out["length"].cpu(), lengths) and out["start"].dtype == torch.int64
        # the smaller position among equal scores: the first entry of a stable descending sort
        want = torch.sort(scores, dim=2, descending=True, stable=True)[1][:, :, 0]
        assert torch.equal(out["best"], want)
        # a winner of length 3 is always named in its first copy (positions 0..3), never in the second (5..8)
        assert not ((out["best"] >= 5) & (out["best"] < 9)).any() and (out["best"] < 5 + 4 + 5).all()
        assert torch.equal(out["best_start"], starts.to(DEV)[out["best"]]) and torch.equal(out["best_length"], lengths.to(DEV)[out["best"]])
        assert torch.equal(_bits(out["best_score"]), _bits(torch.gather(scores, 2, out["best"][..., None])[..., 0]))


def _with_side(ix, side):
    """``ix`` with its object tower replaced by the given outputs (global [Nv, 256], local [Nv, G, 256], additive mask [Nv, G])"""
    ix._video_side = lambda model, block: side
    return ix


class TestTimelinePlanted:
    @pytest.mark.parametrize("seed", [0, 1, 2])
    @pytest.mark.parametrize("gate", GATES)
    def test_each_planted_caption_wins_its_window(self, seed, gate):
        F, R, W, win = 8, 16, 20, 2
        C, Q0, mi, mc0 = _planted(F, R, W, win, 1, seed)                      # caption 0 planted at frame 1
        C1, Q1, _, mc1 = _planted(F, R, W, win, 5, seed)                      # caption 1 at frame 5 of the same video (same seed: same regions)
        assert torch.equal(C, C1)
        Q, mc = torch.cat([Q0, Q1]), torch.cat([mc0, mc1])
        ref = _oracle_windows(C, Q, mi, mc, F, win, 1, gate)[:, 0]            # [2 captions, M]
        gaps = (ref[0, 1] - ref[1, 1], ref[1, 5] - ref[0, 5])
        print("\nseed %d, gate %s: the oracle's gaps %.4f (caption 0 at start 1), %.4f (caption 1 at start 5)" % (seed, gate, *gaps))
        assert min(gaps) > 0.1
        ix = _with_side(_caption_ix(Q, mc), (torch.ones(1, 256, device=DEV, dtype=torch.bfloat16), C, mi))
        data = dict(object=torch.zeros(1, F, R, 1, device=DEV), object_mask=torch.ones(1, F, R, device=DEV))
        tl = ix.timeline(torch.nn.Identity(), RWALoss(LAM, "equal" if gate else "prob"), data, F, win, k=1, shortlist=None)
        assert tl["ids"].shape == (1, F - win + 1, 1) and tl["ids"].dtype == torch.int64 and tl["start"].tolist() == list(range(F - win + 1))
        assert int(tl["ids"][0, 1, 0]) == 0 and int(tl["ids"][0, 5, 0]) == 1
        got = _cmoments(C, Q, mi, mc, F, win, 1, gate)                         # [1, 2, M]
        assert torch.equal(_bits(tl["scores"][0, :, 0]), _bits(got[0].max(0)[0]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: the fixture recipe of tests/test_gpu_long_search.py (F = 10, R = 30, 12 (video, caption) pairs in two batches of 6)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _videos(b):
    return {"object": b["object"], "object_mask": b["object_mask"]}


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


class TestTimeline:
    def test_against_a_brute_force_ranking_of_moments(self, e2e):
        cix, model, loss, F, R, N = e2e["cix"], e2e["model"], e2e["loss"], e2e["F"], e2e["R"], e2e["N"]
        data = _videos(e2e["batches"][0])
        with torch.no_grad():
            go, lo, om = cix._video_side(model.eval(), data)
        om = om.clone()
        om[0, 2 * R:4 * R] = -100.0                                            # video 0: frames 2..3 fully masked -> its window (2, 2) is empty
        try:
            _with_side(cix, (go, lo, om))
            windows = (2, 5)
            tl = cix.timeline(model, loss, data, F, windows, k=3, shortlist=None)
            every = torch.arange(N, device=DEV).expand(6, -1).contiguous()
            mo = cix.moments(model, loss, data, every, F, windows)
            part = cix.timeline(model, loss, data, F, windows, k=3, shortlist=5)
        finally:
            del cix._video_side
        Mt = 9 + 6
        assert tl["ids"].shape == (6, Mt, 3) and tl["scores"].shape == (6, Mt, 3) and tl["cosine"].shape == (6, Mt, 3)
        assert tl["ids"].dtype == torch.int64 and tl["scores"].dtype == torch.float32 and tl["cosine"].dtype == torch.float32
        assert torch.equal(tl["start"], mo["start"]) and torch.equal(tl["length"], mo["length"]) and tl["start"].dtype == torch.int64
        val, pos = torch.sort(mo["scores"].transpose(1, 2), dim=2, descending=True, stable=True)      # [6, Mt, N]
        empty = torch.zeros(6, Mt, dtype=torch.bool, device=DEV)
        empty[0, 2] = True
        assert torch.isneginf(mo["scores"][0, :, 2]).all() and torch.isfinite(mo["scores"].transpose(1, 2)[~empty]).all()
        assert torch.equal(_bits(tl["scores"]), _bits(val[:, :, :3]))
        assert torch.equal(tl["ids"][~empty], pos[:, :, :3][~empty])
        assert (tl["ids"][empty] == -1).all() and torch.isneginf(tl["scores"][empty]).all() and torch.isnan(tl["cosine"][empty]).all()
        sl_ids, sl_cos = cix.shortlist_by_cosine(go, None)
        assert torch.equal(sl_ids, every)
        want = torch.gather(sl_cos[:, None, :].expand(6, Mt, N), 2, tl["ids"].clamp(min=0))
        assert torch.equal(_bits(tl["cosine"][~empty]), _bits(want[~empty]))
        # a partial shortlist: every id comes from the video's shortlist, with the score it has in the full table
        short, _ = cix.shortlist_by_cosine(go, 5)
        assert (part["ids"][~empty][..., None] == short[:, None, None, :].expand(6, Mt, 3, 5)[~empty]).any(-1).all()
        full = torch.gather(mo["scores"].transpose(1, 2), 2, part["ids"].clamp(min=0))
        assert torch.equal(_bits(part["scores"][~empty]), _bits(full[~empty])) and (part["ids"][empty] == -1).all()


class TestEndToEnd:
    def test_search_with_moments(self, e2e):
        cix, vix, model, loss, batches, F = e2e["cix"], e2e["vix"], e2e["model"], e2e["loss"], e2e["batches"], e2e["F"]
        data = _videos(batches[0])
        model.train()
        ids0, scores0 = cix.search(model, loss, data, k=3, shortlist=5)
        res = cix.search(model, loss, data, k=3, shortlist=5, frames=F, moments=(2, 5))
        assert model.training                                                # the training flag is restored
        model.eval()
        assert len(res) == 3
        ids, scores, mo = res
        assert torch.equal(ids, ids0) and torch.equal(_bits(scores), _bits(scores0))
        assert mo["scores"].shape == (6, 3, 9 + 6) and mo["scores"].dtype == torch.float32 and torch.isfinite(mo["scores"]).all()
        assert mo["start"].tolist() == list(range(9)) + list(range(6)) and mo["length"].tolist() == [2] * 9 + [5] * 6
        assert torch.equal(mo["best"], mo["scores"].argmax(2))
        _same_bytes(cix.moments(model, loss, data, ids, F, (2, 5)), mo)
        _same_bytes(cix.moments(model, loss, data, ids.int(), F, (2, 5), stride=1), mo)
        # the other direction on the transposed pairs: every caption (in its own batch, as it was indexed) against the six videos
        vids = torch.arange(6, device=DEV).expand(6, -1).contiguous()
        vm = torch.cat([vix.moments(model, loss, b["text"], vids, F, (2, 5))["scores"] for b in batches])      # [caption, video, M]
        want = vm[ids, torch.arange(6, device=DEV)[:, None].expand(6, 3)]
        assert torch.equal(_bits(mo["scores"]), _bits(want))
        # with grounding too: four elements, the moments last
        four = cix.search(model, loss, data, k=3, shortlist=5, ground=True, frames=F, moments=(2, 5))
        assert len(four) == 4 and "word_scores" in four[2]
        _same_bytes(four[3], mo)
