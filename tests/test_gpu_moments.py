"""Moment search on a real MI355X (product library): the region-range form of the tiled pair kernel (``dvlp_xattn_long_index_moments_fwd``,
DESIGN.md 6i) against the fp64 oracle ``xattn_pair`` on the bf16-rounded SLICE of the video, against garbage in the neighbouring frames,
against the whole-video kernel at ``win = frames``, under masks, on a planted moment, its mechanics, and ``VideoIndex.moments`` /
``search(..., moments=...)`` end to end.

Inputs: ``tests/test_gpu_long_search.py::_inputs`` (correlated channels, video 1 with a masked tail, ragged captions), Bi = 3, Bj = 2, both
gates.  Bar: 2e-3 absolute, the bar of this kernel family against this oracle; the measured maxima are printed and recorded
in DESIGN.md 6i.  Two kinds of window have no oracle value to compare with:
  * gate on and a one-region window (or W = 1): the oracle is 0 / 0 -- a finite value is asserted, as in ``tests/test_gpu_long_search.py``;
  * a window without an unmasked region: -inf by definition (R = 1: the windows inside the masked tail of video 1) -- exactly -inf is asserted.
Every other window of every pair is compared."""
import numpy as np
import pytest
import torch

from demovlp_amd import ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from oracle import restatement as orc
from test_gpu_long_search import GATES, LAM, SCORE_BAR, _filled, _grid, _inputs, _retrieval_model, _same_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda"
#          G     F    W   win stride   the hazard
SHAPES = [(21, 3, 7, 1, 1),          # odd offsets, a window shorter than a 16-row block
          (300, 10, 37, 3, 1),       # R = 30: 4-byte-aligned offsets
          (129, 3, 20, 2, 1),        # R = 43: a window straddling the 128-region tile edge
          (1152, 32, 99, 8, 4),      # R = 36: multi-tile windows starting mid-tile
          (1152, 32, 112, 31, 1),    # the largest proper window
          (16, 16, 99, 1, 5)]        # R = 1: single-region windows


def _bits(t):
    return t.contiguous().view(torch.int32)


def _moments(index, Bi, G, mi, Q, mc, F, win, stride, gate, cand=None):
    cand = _grid(Q.shape[0], Bi) if cand is None else cand
    return ops.xattn_long_index_moments_fwd(index, Bi, G, mi, Q, mc, cand, F, win, stride, LAM, gate)


def _oracle_windows(C, Q, mi, mc, F, win, stride, gate):
    """fp64 ``xattn_pair`` of every (caption, video, window) on the sliced bf16-rounded inputs -> numpy [Bj, Bi, M]"""
    c, q, a, b = C.cpu().double(), Q.cpu().double(), mi.cpu().double(), mc.cpu().double()
    R = C.shape[1] // F
    M = (F - win) // stride + 1
    out = np.empty((q.shape[0], c.shape[0], M))
    for j in range(q.shape[0]):
        for i in range(c.shape[0]):
            for m in range(M):
                g0, g1 = m * stride * R, (m * stride + win) * R
                out[j, i, m] = float(orc.xattn_pair(c[i, g0:g1], q[j], a[i, g0:g1], b[j], LAM, gate))
    return out


def _empty_windows(mi, F, win, stride):
    """bool [Bi, M]: the windows without an unmasked region"""
    keep = (mi.cpu().numpy() == 0).reshape(mi.shape[0], F, -1).any(2)                                    # [Bi, F]: the frame has an unmasked region
    M = (F - win) // stride + 1
    return np.stack([~keep[:, m * stride:m * stride + win].any(1) for m in range(M)], 1)


def _check_windows(got, ref, empty, one_region_gate, tag):
    """every window within the bar of the oracle; -inf exactly where the window is empty; finite where the oracle is 0 / 0"""
    got = got.cpu().numpy()
    hole = np.broadcast_to(empty[None], got.shape)
    assert np.isneginf(got[hole]).all() and np.isfinite(got[~hole]).all(), tag
    if not one_region_gate:
        assert np.isfinite(ref[~hole]).all(), tag                          # nothing else is left out
    ok = ~hole & ~np.isnan(ref)
    dev = float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0
    print("\n%-64s max |moment - fp64| %.3e over %d windows (%d empty, %d with a 0 / 0 oracle)" % (tag, dev, ok.sum(), hole.sum(), (~hole & ~ok).sum()))
    assert dev <= SCORE_BAR, (tag, dev)
    return dev


class TestAgainstTheOracle:
    @pytest.mark.parametrize("G,F,W,win,stride", SHAPES)
    @pytest.mark.parametrize("gate", GATES)
    def test_every_window_within_2e3_of_the_fp64_oracle_on_the_slice(self, G, F, W, win, stride, gate):
        Bi, Bj = 3, 2
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 3000 + G + W)
        got = _moments(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, F, win, stride, gate)
        M = (F - win) // stride + 1
        assert got.shape == (Bj, Bi, M) and got.dtype == torch.float32
        ref = _oracle_windows(C, Q, mi, mc, F, win, stride, gate)
        empty = _empty_windows(mi, F, win, stride)
        assert not empty.any() or G // F == 1                               # only the R = 1 shape has windows inside the masked tail
        _check_windows(got, ref, empty, gate and (win * (G // F) == 1 or W == 1),
                       "G = %d, F = %d, W = %d, win = %d, stride = %d, gate %s" % (G, F, W, win, stride, gate))


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
        clean = _moments(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, F, win, 1, gate)
        other = _moments(_filled(dirty, Bi, [Bi]), Bi, G, mi, Q, mc, F, win, 1, gate)
        assert torch.isfinite(clean[:, :, f0]).all()
        assert torch.equal(_bits(clean[:, :, f0]), _bits(other[:, :, f0]))
        assert not torch.equal(_bits(clean), _bits(other))                  # (the garbage is seen by the windows that hold it)


class TestWholeVideo:
    @pytest.mark.parametrize("G,F,W", [(1152, 32, 99), (300, 10, 37)])
    @pytest.mark.parametrize("gate", GATES)
    def test_a_window_of_all_frames_is_bit_equal_to_the_pair_kernel(self, G, F, W, gate):
        Bi, Bj = 3, 2
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5200 + G)
        index = _filled(C, Bi, [Bi])
        got = _moments(index, Bi, G, mi, Q, mc, F, F, 1, gate)
        want = ops.xattn_long_index_pairs_fwd(index, Bi, G, mi, Q, mc, _grid(Bj, Bi), LAM, gate)
        assert got.shape == (Bj, Bi, 1) and torch.isfinite(want).all()
        assert torch.equal(_bits(got[:, :, 0]), _bits(want)), float((got[:, :, 0] - want).abs().max())


def _video_index(C, mi, capacity=None):
    """a tiled ``VideoIndex`` of the videos C with the additive masks mi (the global embeddings do not matter to moments)"""
    n, G = C.shape[:2]
    ix = search.VideoIndex(capacity or n, G, torch.bfloat16, DEV, tiled=True)
    ix.add(dict(global_object_embeddings=torch.ones(n, 256, device=DEV, dtype=torch.bfloat16), local_object_embeddings=C, object_mask=mi))
    return ix


def _block(ix, Q, mc, ids, F, windows, stride=1, gate=True):
    return ix._moments_block(RWALoss(LAM, "equal" if gate else "prob"), (None, Q, mc), ids, F, ix._moment_checks(F, windows, stride), stride)


class TestMasks:
    @pytest.mark.parametrize("gate", GATES)
    def test_an_empty_window_is_minus_inf_and_never_the_best(self, gate):
        Bi, Bj, G, F, W, win = 3, 2, 300, 10, 37, 2
        R = G // F
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 6300)
        mi[2, 2 * R:4 * R] = -100.0                                        # video 2: frames 2..3 fully masked
        got = _moments(_filled(C, Bi, [Bi]), Bi, G, mi, Q, mc, F, win, 1, gate)
        empty = _empty_windows(mi, F, win, 1)
        assert empty.sum() == 1 and empty[2, 2]
        assert torch.isneginf(got[:, 2, 2]).all()
        # the windows partly masked (frames 1..2 and 3..4 of video 2, the tail of video 1) stay within the bar
        _check_windows(got, _oracle_windows(C, Q, mi, mc, F, win, 1, gate), empty, False, "G = 300, frames 2..3 of video 2 masked, gate %s" % gate)
        out = _block(_video_index(C, mi), Q, mc, _grid(Bj, Bi), F, win, 1, gate)
        assert torch.equal(_bits(out["scores"]), _bits(got))
        assert (out["best"][:, 2] != 2).all() and torch.isfinite(out["best_score"]).all()
        assert torch.equal(out["best"], got.argmax(2))


def _planted(F, R, W, win, f0, seed):
    rng = np.random.default_rng(seed)
    im = rng.standard_normal((F * R, 256), dtype=np.float32)
    cap = rng.standard_normal((W, 256), dtype=np.float32)
    n, g0 = min(W, win * R), f0 * R
    cap[:n] = im[g0:g0 + n] + 0.5 * cap[:n]
    m_cap = np.zeros((1, W), np.float32)
    m_cap[0, W - 3:] = -100.0                                              # the last three words masked
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(im)[None].bfloat16(), t(cap)[None].bfloat16(), torch.zeros(1, F * R, device=DEV), t(m_cap)


class TestPlantedMoment:
    @pytest.mark.parametrize("F,R,W,win,f0", [(8, 16, 20, 2, 4), (3, 7, 7, 1, 2)])
    @pytest.mark.parametrize("seed", [0, 1, 2])
    @pytest.mark.parametrize("gate", GATES)
    def test_the_planted_window_is_the_best(self, F, R, W, win, f0, seed, gate):
        C, Q, mi, mc = _planted(F, R, W, win, f0, seed)
        ref = _oracle_windows(C, Q, mi, mc, F, win, 1, gate)[0, 0]
        order = np.argsort(-ref)
        gap = ref[order[0]] - ref[order[1]]
        print("\nF = %d, R = %d, W = %d, win = %d, seed %d, gate %s: the oracle's gap %.4f" % (F, R, W, win, seed, gate, gap))
        assert order[0] == f0 and gap > 0.1
        out = _block(_video_index(C, mi), Q, mc, torch.zeros(1, 1, device=DEV, dtype=torch.int64), F, win, 1, gate)
        assert int(out["best_start"][0, 0]) == f0 and int(out["best_length"][0, 0]) == win and int(out["best"][0, 0]) == f0
        assert float(out["best_score"][0, 0]) == float(out["scores"][0, 0, f0])


class TestMechanics:
    def test_bad_and_repeated_candidates_and_two_runs(self):
        Bi, Bj, G, F, W, K, win = 4, 3, 300, 10, 37, 5, 3
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 7)
        ix = _video_index(C, mi, capacity=6)                                  # capacity 6: rows 4, 5 were never added
        cand = np.random.default_rng(1).integers(0, Bi, (Bj, K)).astype(np.int32)
        cand[0, -1] = cand[0, 0]                                              # a repeated candidate in a row
        dev = lambda a: torch.from_numpy(a).to(DEV)
        good = _moments(ix.local, 6, G, ix.om, Q, mc, F, win, 1, True, dev(cand))
        assert good.shape == (Bj, K, 8) and torch.isfinite(good).all() and torch.equal(_bits(good[0, -1]), _bits(good[0, 0]))
        assert torch.equal(_bits(good), _bits(_moments(ix.local, 6, G, ix.om, Q, mc, F, win, 1, True, dev(cand))))      # two runs
        bad = cand.copy()
        bad[1, 2], bad[2, 0], bad[2, 4] = -1, 6, 2 ** 31 - 1
        got = _moments(ix.local, 6, G, ix.om, Q, mc, F, win, 1, True, dev(bad))
        hole = dev(bad != cand)
        assert int(hole.sum()) == 3 and torch.isnan(got[hole]).all()
        assert torch.equal(_bits(got[~hole]), _bits(good[~hole]))
        out = _block(ix, Q, mc, dev(bad), F, win, 1, True)
        assert torch.equal(_bits(out["scores"]), _bits(got))
        for name in ("best", "best_start", "best_length"):
            assert out[name].dtype == torch.int64 and (out[name][hole] == -1).all() and (out[name][~hole] >= 0).all(), name
        assert torch.isnan(out["best_score"][hole]).all() and torch.isfinite(out["best_score"][~hole]).all()

    def test_several_window_lengths_and_the_tie_rule(self):
        Bi, Bj, G, F, W = 3, 2, 300, 10, 37
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 8)
        ix = _video_index(C, mi)
        windows, stride = (3, 10, 3, 1), 2                                    # a repeated length: its windows tie with their first copies
        out = _block(ix, Q, mc, _grid(Bj, Bi), F, windows, stride, True)
        per = [_moments(ix.local, Bi, G, ix.om, Q, mc, F, w, stride, True) for w in windows]
        assert [p.shape[2] for p in per] == [4, 1, 4, 5]
        scores = torch.cat(per, 2)
        assert torch.equal(_bits(out["scores"]), _bits(scores))
        starts, lengths = search.moment_windows(F, windows, stride)
        assert torch.equal(out["start"].cpu(), starts) and torch.equal(out["length"].cpu(), lengths) and out["start"].dtype == torch.int64
        # the smaller position among equal scores: torch.argmax over a stable descending sort
        want = torch.sort(scores, dim=2, descending=True, stable=True)[1][:, :, 0]
        assert torch.equal(out["best"], want)
        first = torch.cat([per[0], per[1]], 2).argmax(2)
        assert ((out["best"] >= 5) | (out["best"] == first)).all() and (out["best"] < 5 + 4 + 5).all()
        # a winner of length 3 is always named in its first copy (positions 0..3), never in the second (5..8)
        assert not ((out["best"] >= 5) & (out["best"] < 9)).any()
        assert torch.equal(out["best_start"], starts.to(DEV)[out["best"]]) and torch.equal(out["best_length"], lengths.to(DEV)[out["best"]])
        assert torch.equal(_bits(out["best_score"]), _bits(torch.gather(scores, 2, out["best"][..., None])[..., 0]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# end to end: the fixture recipe of tests/test_gpu_long_search.py (F = 10, R = 30, 12 videos, 6 queries)
# ---------------------------------------------------------------------------------------------------------------------------------------
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
    tiled = search.VideoIndex(N, F * R, torch.bfloat16, DEV, tiled=True).add_batches(model, batches)
    return dict(model=model, loss=loss, text=batches[0]["text"], tiled=tiled, F=F, R=R)


class TestEndToEnd:
    def test_search_with_moments(self, e2e):
        tiled, model, loss, text, F = e2e["tiled"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"]
        model.train()
        ids0, scores0 = tiled.search(model, loss, text, k=3, shortlist=5)
        res = tiled.search(model, loss, text, k=3, shortlist=5, frames=F, moments=(2, 10))
        assert model.training                                                # the training flag is restored
        model.eval()
        assert len(res) == 3
        ids, scores, mo = res
        assert torch.equal(ids, ids0) and torch.equal(_bits(scores), _bits(scores0))
        assert mo["scores"].shape == (6, 3, 9 + 1) and mo["scores"].dtype == torch.float32 and torch.isfinite(mo["scores"]).all()
        assert mo["start"].tolist() == list(range(9)) + [0] and mo["length"].tolist() == [2] * 9 + [10]
        for name in ("best", "best_start", "best_length", "best_score"):
            assert mo[name].shape == (6, 3), name
        assert torch.equal(mo["best"], mo["scores"].argmax(2))
        # the window of all ten frames is the local score of the pair: the grounding launch's `score`, bit for bit
        gr = tiled.ground(model, loss, text, ids, frames=F)
        assert torch.equal(_bits(mo["scores"][:, :, 9]), _bits(gr["score"]))
        _same_bytes(tiled.moments(model, loss, text, ids, F, (2, 10)), mo)
        _same_bytes(tiled.moments(model, loss, text, ids.int(), F, (2, 10), stride=1), mo)

    def test_search_with_ground_and_moments(self, e2e):
        tiled, model, loss, text, F = e2e["tiled"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"]
        ids0, scores0, gr0 = tiled.search(model, loss, text, k=3, shortlist=5, ground=True, frames=F)
        res = tiled.search(model, loss, text, k=3, shortlist=5, ground=True, frames=F, moments=(2, 10), moment_stride=4)
        assert len(res) == 4
        ids, scores, gr, mo = res
        assert torch.equal(ids, ids0) and torch.equal(_bits(scores), _bits(scores0))
        _same_bytes(gr, gr0)
        assert mo["start"].tolist() == [0, 4, 8, 0] and mo["length"].tolist() == [2, 2, 2, 10]
        assert torch.equal(_bits(mo["scores"][:, :, 3]), _bits(gr["score"]))
        _same_bytes(tiled.moments(model, loss, text, ids, F, (2, 10), stride=4), mo)
