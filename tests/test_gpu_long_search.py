"""Search and grounding for long videos on a real MI355X (product library): the region-tiled pair kernel (``dvlp_xattn_long_index_*``,
DESIGN.md 6g) against the fp64 oracle on the same bf16-rounded inputs, against the kernels it stands beside (the fused pair kernel inside
its range, bf16 ``RWALoss.get_sim`` outside it), the mechanics of its resident index, its grounding against ``ground_reference`` of
``tests/test_ground.py`` under the bars of ``tests/test_gpu_ground.py``, and ``VideoIndex(..., tiled=True)`` end to end.

Inputs: the recipe of ``test_fused_local_loss_forward_vs_oracle`` (correlated leading channels, a masked video tail, ragged captions) on a
[videos x captions] candidate grid, both gate settings.  At G = 1 or W = 1 with the gate on the oracle is 0 / 0 (header of
``tests/test_gpu_ground.py``): a finite value is asserted there.

Bars.  Scores: 2e-3 absolute, the project's bar for the fused kernel against this oracle on this recipe (an fp32 emulation of the tiled
arithmetic stayed within 2.5e-4 on these shapes).  Grounding: the bars of ``tests/test_gpu_ground.py``, measured there for the short kernel.
Frame means: 36 fp32 additions of terms below 1, 36 x 2^-24 doubled.  Measured values are printed by the tests and recorded in DESIGN.md 6g."""
import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, functional as Fn, ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from demovlp_amd.model import ObjectRelation
from oracle import restatement as orc
from test_ground import ground_reference
from test_gpu_ground import AGREE_MIN, DELTA, SCORE_DEV_BAR, WEIGHT_DEV_BAR

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAM = 20.0
SCORE_BAR = 2e-3
FRAME_BAR = 2 * 36 * 2.0 ** -24
#          G     W     the edge
SHAPES = [(1, 99),      # single region
          (16, 99),     # one block
          (128, 99),    # exactly one tile
          (129, 7),     # one region past a 128-region tile
          (289, 37),    # first G out of the fused range, ragged 16-row block
          (304, 99),
          (960, 112),
          (1152, 99),   # top of the range
          (1152, 1)]    # single word
GATES = [True, False]


def _inputs(Bi, Bj, G, W, seed):
    rng = np.random.default_rng(seed)
    im = rng.standard_normal((Bi, G, 256), dtype=np.float32)
    cap = rng.standard_normal((Bj, W, 256), dtype=np.float32)
    n = min(G, W)
    for b in range(min(Bi, Bj)):
        cap[b, :n, :64] += im[b, :n, :64] * 0.5
    m_img = np.zeros((Bi, G), np.float32)
    m_img[1, max(0, G - 5):] = -100.0 if G > 5 else 0.0          # a masked video tail (never a whole video)
    lens = rng.integers(min(2, W), max(min(30, W), min(2, W) + 1), Bj).clip(1, W)
    m_cap = np.full((Bj, W), -100.0, np.float32)
    for b in range(Bj):
        m_cap[b, : lens[b]] = 0.0
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(im).bfloat16(), t(cap).bfloat16(), t(m_img), t(m_cap)


def _grid(Bj, Bi):
    """every video for every caption, int32 [Bj, Bi]"""
    return torch.arange(Bi, device=DEV, dtype=torch.int32).expand(Bj, -1).contiguous()


def _filled(C, capacity, splits):
    G = C.shape[1]
    index = torch.zeros(ops.xattn_long_index_bytes(capacity, G), device=DEV, dtype=torch.uint8)
    r0 = 0
    for n in splits:
        ops.xattn_long_index_add(index, capacity, G, r0, C[r0:r0 + n].contiguous())
        r0 += n
    return index


def _oracle(C, Q, mi, mc, gate):
    """fp64 ``xattn_pair`` of every (caption, video) pair on the bf16-rounded inputs -> numpy [Bj, Bi]"""
    c, q, a, b = C.cpu().double(), Q.cpu().double(), mi.cpu().double(), mc.cpu().double()
    return np.array([[float(orc.xattn_pair(c[i], q[j], a[i], b[j], LAM, gate)) for i in range(c.shape[0])] for j in range(q.shape[0])])


def _check_scores(got, ref, tag):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), tag
    ok = ~np.isnan(ref)
    dev = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    print("\n%-44s max |score - fp64| %.3e%s" % (tag, dev, "" if ok.all() else "   (oracle 0 / 0 at %d of %d pairs: finite asserted)" % ((~ok).sum(), ok.size)))
    assert dev <= SCORE_BAR, (tag, dev)


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        assert torch.equal(a[name].contiguous().view(torch.uint8), b[name].contiguous().view(torch.uint8)), name


class TestScoreAgainstTheOracle:
    @pytest.mark.parametrize("G,W", SHAPES)
    @pytest.mark.parametrize("gate", GATES)
    def test_scores_within_2e3_of_the_fp64_oracle(self, G, W, gate):
        Bi, Bj = 3, 2
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 3000 + G + W)
        got = ops.xattn_long_index_pairs_fwd(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, gate)
        assert got.shape == (Bj, Bi) and got.dtype == torch.float32
        ref = _oracle(C, Q, mi, mc, gate)
        if not (gate and (G == 1 or W == 1)):
            assert np.isfinite(ref).all()
        _check_scores(got, ref, "G = %d, W = %d, gate %s" % (G, W, gate))

    @pytest.mark.parametrize("gate", GATES)
    def test_whole_tiles_of_masked_regions(self, gate):
        """video 0: the last 200 regions masked (the last tile holds masked regions only); video 1: the first 130 (the first tile, and two
        regions of the second)"""
        Bi, Bj, G, W = 2, 2, 1152, 99
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 77)
        mi.zero_()
        mi[0, G - 200:] = -100.0
        mi[1, :130] = -100.0
        got = ops.xattn_long_index_pairs_fwd(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, gate)
        ref = _oracle(C, Q, mi, mc, gate)
        assert np.isfinite(ref).all()
        _check_scores(got, ref, "G = 1152, W = 99, masked tiles, gate %s" % gate)


class TestAgainstTheExistingKernels:
    @pytest.mark.parametrize("G", [240, 288])
    @pytest.mark.parametrize("gate", GATES)
    def test_inside_the_fused_range_within_2e3_of_the_fused_pair_kernel(self, G, gate):
        Bi, Bj, W = 3, 3, 99
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 500 + G)
        cand = _grid(Bj, Bi)
        short = torch.zeros(ops.xattn_index_bytes(Bi, G), device=DEV, dtype=torch.uint8)
        ops.xattn_index_add(short, Bi, G, 0, C)
        index = _filled(C, Bi, [Bi])
        assert torch.equal(short, index)                                   # one resident layout
        want = ops.xattn_index_pairs_fwd(short, Bi, G, mi, Q, mc, cand, LAM, gate)
        got = ops.xattn_long_index_pairs_fwd(index, Bi, G, mi, Q, mc, cand, LAM, gate)
        dev = float((got - want).abs().max())
        print("\nG = %d, gate %s: max |tiled - fused| %.3e" % (G, gate, dev))
        assert dev <= SCORE_BAR, dev

    @pytest.mark.parametrize("focal", ["equal", "prob"])
    def test_outside_it_within_2e3_of_bf16_get_sim(self, focal):
        Bi, Bj, G, W = 3, 3, 304, 99
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 804)
        with torch.no_grad():
            want = RWALoss(20, focal).get_sim(C, Q, mi, None, mc).t()      # [Bj, Bi]
        got = ops.xattn_long_index_pairs_fwd(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, focal == "equal")
        dev = float((got - want.float()).abs().max())
        print("\nG = 304, %s: max |tiled - get_sim| %.3e" % (focal, dev))
        assert dev <= SCORE_BAR, dev


class TestIndexMechanics:
    def test_three_adds_are_byte_equal_to_one_and_spare_rows_stay_untouched(self):
        C, _, _, _ = _inputs(7, 2, 304, 20, 3)
        one, three = _filled(C, 9, [7]), _filled(C, 9, [2, 4, 1])
        assert torch.equal(one, three)
        # rows 7, 8 of every section keep their zeros: chat [9][304][256], chatT [9][256][320] (bf16), nc [9][304] (fp32)
        a, b = 9 * 304 * 512, 9 * 256 * 320 * 2
        assert one.numel() == a + b + 11008 and int(one[:a].view(9, -1)[:7].count_nonzero()) > 0
        assert not one[:a].view(9, -1)[7:].any() and not one[a:a + b].view(9, -1)[7:].any() and not one[a + b:a + b + 9 * 304 * 4].view(9, -1)[7:].any()

    def test_out_of_range_and_repeated_candidates_and_two_runs(self):
        Bi, Bj, G, W, K = 4, 3, 304, 99, 5
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5)
        index = _filled(C, 6, [Bi])                                           # capacity 6: rows 4, 5 were never added
        mi6 = torch.cat([mi, torch.zeros(2, G, device=DEV)])
        cand = np.random.default_rng(1).integers(0, Bi, (Bj, K)).astype(np.int32)
        cand[0, -1] = cand[0, 0]                                              # a repeated candidate in a row
        good = ops.xattn_long_index_pairs_fwd(index, 6, G, mi6, Q, mc, torch.from_numpy(cand).to(DEV), LAM, True)
        assert torch.isfinite(good).all() and good[0, -1].view(torch.int32) == good[0, 0].view(torch.int32)
        again = ops.xattn_long_index_pairs_fwd(index, 6, G, mi6, Q, mc, torch.from_numpy(cand).to(DEV), LAM, True)
        assert torch.equal(good.view(torch.int32), again.view(torch.int32))
        bad = cand.copy()
        bad[1, 2], bad[2, 0], bad[2, 4] = -1, 6, 2 ** 31 - 1
        got = ops.xattn_long_index_pairs_fwd(index, 6, G, mi6, Q, mc, torch.from_numpy(bad).to(DEV), LAM, True)
        hole = torch.from_numpy(bad != cand).to(DEV)
        assert int(hole.sum()) == 3 and torch.isnan(got[hole]).all()
        assert torch.equal(got[~hole].view(torch.int32), good[~hole].view(torch.int32))
        gr = ops.xattn_long_index_pairs_ground(index, 6, G, mi6, Q, mc, torch.from_numpy(bad).to(DEV), LAM, True, frames=8)
        for name in ("score", "word_scores", "region_scores", "word_region_weight", "frame_scores"):
            assert torch.isnan(gr[name][hole]).all() and torch.isfinite(gr[name][~hole]).all(), name
        for name in ("word_region", "region_word"):
            assert (gr[name][hole] == -1).all() and (gr[name][~hole] >= 0).all(), name

    def test_forward_only(self):
        C, Q, mi, mc = _inputs(2, 3, 30, 20, 1)
        Q.requires_grad_(True)
        s = Fn.XattnLongIndexPairsFn.apply(_filled(C, 2, [2]), 2, 30, mi, Q, mc, torch.zeros(3, 2, device=DEV, dtype=torch.int32), LAM, True)
        with pytest.raises(DemoVLPHipError):
            s.sum().backward()


GROUND_SHAPES = [(304, 99, 8), (1152, 99, 32), (129, 7, 3)]      # G, W, frames


class GroundRun:
    """One shape and gate: the grounding launch's outputs on the host and the fp64 reference of every pair."""

    def __init__(self, G, W, frames, gate):
        Bi, Bj = 3, 2
        self.G, self.W, self.frames, self.gate = G, W, frames, gate
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 9000 + G + W)
        self.args = (_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, gate)
        self.dev = ops.xattn_long_index_pairs_ground(*self.args, frames=frames)
        self.out = {k: v.cpu().numpy() for k, v in self.dev.items()}
        self.m_img = mi.cpu().numpy()
        c, q, a, b = C.cpu().double(), Q.cpu().double(), mi.cpu().double(), mc.cpu().double()
        self.ref = {(j, i): {k: v.numpy() for k, v in ground_reference(c[i], q[j], a[i], b[j], LAM, gate).items()} for j in range(Bj) for i in range(Bi)}

    def tag(self):
        return "G = %d, W = %d, gate %s" % (self.G, self.W, self.gate)


@pytest.fixture(scope="module")
def runs():
    return [GroundRun(G, W, F, gate) for G, W, F in GROUND_SHAPES for gate in GATES]


class TestGrounding:
    def test_score_is_bit_equal_to_the_score_launch_and_two_calls_agree(self, runs):
        for r in runs:
            fwd = ops.xattn_long_index_pairs_fwd(*r.args)
            assert torch.equal(r.dev["score"].view(torch.int32), fwd.view(torch.int32)), (r.tag(), float((r.dev["score"] - fwd).abs().max()))
            _same_bytes(ops.xattn_long_index_pairs_ground(*r.args, frames=r.frames), r.dev)
            none = ops.xattn_long_index_pairs_ground(*r.args)
            assert "frame_scores" not in none
            _same_bytes(none, {k: v for k, v in r.dev.items() if k != "frame_scores"})

    def test_word_and_region_scores_against_the_fp64_reference(self, runs):
        worst = 0.0
        for r in runs:
            d = 0.0
            for (j, i), ref in r.ref.items():
                for name in ("word_scores", "region_scores"):
                    got = r.out[name][j, i]
                    assert np.isfinite(got).all() and np.isfinite(ref[name]).all(), (r.tag(), name)
                    d = max(d, float(np.abs(got - ref[name]).max()))
            print("\n%-36s max |word / region score - fp64| %.3e" % (r.tag(), d))
            worst = max(worst, d)
        print("\nper-term deviation over all shapes: %.3e (bar %.3e)" % (worst, SCORE_DEV_BAR))
        assert worst <= SCORE_DEV_BAR, worst

    def test_argmaxes_against_the_fp64_reference(self, runs):
        worst, pooled = 0.0, {"word_region": [], "region_word": []}
        for r in runs:
            for name, key in (("word_region", "logit_wr"), ("region_word", "logit_rw")):
                short, same = 0.0, []
                for (j, i), ref in r.ref.items():
                    logit = ref[key]
                    pick = r.out[name][j, i].astype(np.int64)
                    assert pick.min() >= 0 and pick.max() < logit.shape[1], (r.tag(), name)
                    at = np.take_along_axis(logit, pick[:, None], 1)[:, 0]
                    short = max(short, float((logit.max(1) - at).max()))
                    same.append(pick == logit.argmax(1))
                print("\n%-36s %-12s largest shortfall %.3e logit units, exact agreement %.4f" % (r.tag(), name, short, float(np.concatenate(same).mean())))
                worst = max(worst, short)
                pooled[name] += same
            wr = r.out["word_region"].astype(np.int64)                      # [Bj, Bi, W]: no word names a masked region
            assert not np.take_along_axis(np.broadcast_to(r.m_img[None] != 0, wr.shape[:2] + (r.G,)), wr, 2).any(), r.tag()
        print("\nlargest shortfall over all shapes: %.3e (delta %.3e)" % (worst, DELTA))
        assert worst <= DELTA, worst
        for name in pooled:
            share = float(np.concatenate(pooled[name]).mean())
            print("exact agreement over all shapes, %s: %.4f" % (name, share))
            assert share >= AGREE_MIN, (name, share)

    def test_word_region_weight_against_the_reference_at_the_kernels_own_pick(self, runs):
        worst = 0.0
        for r in runs:
            d = 0.0
            for (j, i), ref in r.ref.items():
                pick = r.out["word_region"][j, i].astype(np.int64)
                want = np.take_along_axis(ref["P"], pick[:, None], 1)[:, 0]
                got = r.out["word_region_weight"][j, i]
                assert np.isfinite(got).all() and np.isfinite(want).all(), r.tag()
                d = max(d, float(np.abs(got - want).max()))
            print("\n%-36s max |word_region_weight - fp64 P[w, g*]| %.3e" % (r.tag(), d))
            worst = max(worst, d)
        print("\nweight deviation over all shapes: %.3e (bar %.3e)" % (worst, WEIGHT_DEV_BAR))
        assert worst <= WEIGHT_DEV_BAR, worst

    def test_frame_scores_are_masked_means_of_the_region_scores(self, runs):
        worst = 0.0
        for r in runs:
            F, G = r.frames, r.G
            assert (r.G, F) != (1152, 32) or G // F == 36
            for j in range(r.out["score"].shape[0]):
                for i in range(r.out["score"].shape[1]):
                    keep = (r.m_img[i] == 0).reshape(F, G // F)
                    rs = r.out["region_scores"][j, i].astype(np.float64).reshape(F, G // F)
                    assert keep.any(1).all()
                    worst = max(worst, float(np.abs(r.out["frame_scores"][j, i] - (rs * keep).sum(1) / keep.sum(1)).max()))
        print("\nmax |frame_scores - masked mean of region_scores| %.3e (bar %.3e)" % (worst, FRAME_BAR))
        assert worst <= FRAME_BAR, worst

    def test_means_of_the_rows_add_up_to_the_score(self, runs):
        for r in runs:
            o = r.out
            d = np.abs(o["word_scores"].astype(np.float64).mean(-1) + o["region_scores"].astype(np.float64).mean(-1) - o["score"]).max()
            assert d <= 2 * (r.G + r.W) * 2.0 ** -24, (r.tag(), d)      # G + W fp32 additions of terms below 1, doubled


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: F = 10, R = 30 (G = 300, just out of the fused range), 12 videos, 6 queries
# ---------------------------------------------------------------------------------------------------------------------------------------
def _retrieval_model(F, R, sd, dtype):
    m = ObjectRelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None},
                       {"model": "pretrained/distilbert-base-uncased", "pretrained": True, "input": "text", "two_outputs": True}, pretrained_init=False, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.set_text_dropout(0.0)
    return m.to(DEV)


@pytest.fixture(scope="module")
def e2e():
    F, R, N, NQ = 10, 30, 12, 6
    sd = syn.retrieval_state_dict(F, R)
    model = _retrieval_model(F, R, sd, "bfloat16")
    loss = GlobalLocalLoss(use_local=True, use_global=True, coef=1.0, focal_type="equal")
    batches = []
    for b in range(N // 6):
        obj, mask, ids, att = syn.retrieval_batch(sd, F, R, b * 6, 6)
        batches.append({"text": {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(att).to(DEV)},
                        "object": torch.from_numpy(obj).to(DEV), "object_mask": torch.from_numpy(mask).to(DEV)})
    tiled = search.VideoIndex(N, F * R, torch.bfloat16, DEV, tiled=True).add_batches(model, batches)
    parity = search.VideoIndex(N, F * R, torch.bfloat16, DEV).add_batches(model, batches)
    return dict(model=model, loss=loss, text=batches[0]["text"], tiled=tiled, parity=parity, F=F, R=R, N=N, NQ=NQ)


class TestTiledVideoIndex:
    def test_search_agrees_with_the_parity_route(self, e2e):
        tiled, parity, model, loss, text = e2e["tiled"], e2e["parity"], e2e["model"], e2e["loss"], e2e["text"]
        assert tiled.tiled and not tiled.fused and not parity.fused and not parity.tiled and len(tiled) == 12
        ids, scores = tiled.search(model, loss, text, k=3, shortlist=5)
        pid, pscores = parity.search(model, loss, text, k=4, shortlist=5)      # one more: the gap behind the last position
        assert ids.shape == (6, 3) and scores.dtype == torch.float32
        # the same shortlist (one global stage); scores of the same video within 2e-3
        t_all, p_all = tiled.search(model, loss, text, k=5, shortlist=5), parity.search(model, loss, text, k=5, shortlist=5)
        t_by_id = torch.gather(t_all[1], 1, torch.argsort(t_all[0], 1))
        p_by_id = torch.gather(p_all[1], 1, torch.argsort(p_all[0], 1))
        assert torch.equal(torch.sort(t_all[0], 1)[0], torch.sort(p_all[0], 1)[0])
        dev = float((t_by_id - p_by_id).abs().max())
        print("\nmax |tiled - parity| search score %.3e" % dev)
        assert dev <= SCORE_BAR, dev
        # the same ids wherever the parity route's adjacent score gaps exceed 4e-3
        ps = pscores.cpu().numpy().astype(np.float64)
        gap = ps[:, :-1] - ps[:, 1:]                                         # [6, 3]: gap[p] between positions p and p + 1
        decided = gap > 4e-3
        decided[:, 1:] &= gap[:, :-1] > 4e-3
        print("positions decided by more than 4e-3: %d of %d" % (decided.sum(), decided.size))
        assert decided.sum() * 2 >= decided.size
        assert (ids.cpu().numpy()[decided] == pid.cpu().numpy()[:, :3][decided]).all()

    def test_search_with_ground_and_frames(self, e2e):
        tiled, model, loss, text, F, R = e2e["tiled"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"], e2e["R"]
        ids0, scores0 = tiled.search(model, loss, text, k=3, shortlist=5)
        ids, scores, gr = tiled.search(model, loss, text, k=3, shortlist=5, ground=True, frames=F)
        assert torch.equal(ids, ids0) and torch.equal(scores.view(torch.int32), scores0.view(torch.int32))
        W = text["input_ids"].shape[1] - 1
        assert gr["word_frame"].shape == (6, 3, W) and int(gr["word_frame"].min()) >= 0 and int(gr["word_frame"].max()) < F
        assert torch.equal(gr["word_frame"], gr["word_region"] // R) and gr["frame_scores"].shape == (6, 3, F)
        assert gr["region_scores"].shape == (6, 3, F * R) and torch.isfinite(gr["score"]).all()
        _same_bytes(tiled.ground(model, loss, text, ids, frames=F), gr)

    def test_state_dict_round_trip(self, e2e, tmp_path):
        tiled, parity, model, loss, text = e2e["tiled"], e2e["parity"], e2e["model"], e2e["loss"], e2e["text"]
        state = tiled.state_dict()
        assert state["tiled"] is True and "tiled" not in parity.state_dict()
        torch.save(state, tmp_path / "index.pt")
        fresh = search.VideoIndex(12, 300, torch.bfloat16, DEV, tiled=True).load_state_dict(torch.load(tmp_path / "index.pt"))
        assert len(fresh) == 12 and torch.equal(fresh.local, tiled.local) and torch.equal(fresh.gn, tiled.gn) and torch.equal(fresh.om, tiled.om)
        a, b = tiled.search(model, loss, text, k=3, shortlist=5), fresh.search(model, loss, text, k=3, shortlist=5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        with pytest.raises(ValueError):
            search.VideoIndex(12, 300, torch.bfloat16, DEV).load_state_dict(state)
