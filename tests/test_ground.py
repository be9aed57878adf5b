"""Grounding of search results, host side: the fp64 reference of the grounding outputs (pinned to ``oracle.restatement.xattn_pair``), the
size helper and the argument checks of ``dvlp_xattn_index_pairs_ground``, and the host checks of ``VideoIndex.ground`` (no GPU needed).
``tests/test_gpu_ground.py`` compares the kernel with ``ground_reference``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss
from oracle import restatement as orc

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (demovlp_amd/csrc/common.h)


def ground_reference(C, Q, m_img, m_cap, lam=20.0, gate=True):
    """``oracle.restatement.xattn_pair`` with its intermediate results kept: the same helpers in the same composition, so that
    ``word_scores.mean() + region_scores.mean()`` IS its return value.  C [G, d], Q [W, d] raw, additive masks [G], [W] (float64 for a reference).
    ``logit_wr`` [W, G] and ``logit_rw`` [G, W] are the logits the two argmaxes are defined on (a word's own mask / a region's own mask is a
    constant along the axis it is taken over and is left out, as the kernel's definition does)."""
    Ch, Qh = orc._unit(C), orc._unit(Q)
    S = F.leaky_relu(Ch @ Qh.t(), 0.1)
    A = S / (S.pow(2).sum(1, keepdim=True).sqrt() + 1e-8)
    P = orc._focal_softmax(lam * (A.t() + m_cap[:, None] + m_img[None, :]), gate)          # [W, G]
    word_scores = orc._cos_rows(Q, P @ Ch)
    A2 = S / (S.pow(2).sum(0, keepdim=True).sqrt() + 1e-8)
    P2 = orc._focal_softmax(lam * (A2 + m_img[:, None] + m_cap[None, :]), gate)            # [G, W]
    region_scores = orc._cos_rows(C, P2 @ Qh)
    return dict(word_scores=word_scores, region_scores=region_scores, P=P, P2=P2, logit_wr=lam * (A.t() + m_img[None, :]),
                logit_rw=lam * (A2 + m_cap[None, :]))


def _pair(G, W, seed, words):
    rng = np.random.default_rng(seed)
    C, Q = torch.from_numpy(rng.standard_normal((G, 256))), torch.from_numpy(rng.standard_normal((W, 256)))
    m_img, m_cap = torch.zeros(G, dtype=torch.float64), torch.full((W,), -100.0, dtype=torch.float64)
    if G > 4:
        m_img[G - 4:] = -100.0
    m_cap[:words] = 0.0
    return C, Q, m_img, m_cap


class TestReferenceIsTheOracle:
    @pytest.mark.parametrize("G,W,words", [(240, 99, 13), (288, 112, 112), (1, 99, 8), (48, 37, 1)])
    @pytest.mark.parametrize("gate", [True, False])
    def test_means_of_the_per_word_and_per_region_cosines_are_xattn_pair(self, G, W, words, gate):
        C, Q, m_img, m_cap = _pair(G, W, G + W, words)
        ref = ground_reference(C, Q, m_img, m_cap, 20.0, gate)
        want = orc.xattn_pair(C, Q, m_img, m_cap, 20.0, gate)
        assert ref["word_scores"].shape == (W,) and ref["region_scores"].shape == (G,) and ref["word_scores"].dtype == torch.float64
        got = ref["word_scores"].mean() + ref["region_scores"].mean()
        assert np.array_equal(got.numpy(), want.numpy(), equal_nan=True)                                # difference 0 in float64
        # one region and the 'equal' gate: the gate keeps P G > sum P, which a single entry never is, and the reference divides 0 by 0
        assert bool(torch.isnan(want)) == (gate and G == 1)
        if not torch.isnan(want):
            # the rows of both attention matrices sum to one, and the left-out mask terms do not move an argmax
            assert torch.allclose(ref["P"].sum(1), torch.ones(W, dtype=torch.float64)) and torch.allclose(ref["P2"].sum(1), torch.ones(G, dtype=torch.float64))
        assert torch.equal(ref["logit_wr"].argmax(1), (ref["logit_wr"] + 20.0 * m_cap[:, None]).argmax(1))


class TestEntryArgumentChecks:
    def test_workspace_helper_runs_on_the_host(self):
        assert "dvlp_xattn_index_ground_workspace_bytes" in _lib.exported_symbols() and "dvlp_xattn_index_pairs_ground" in _lib.exported_symbols()
        wb = lambda Bj, W, K, G: _lib.call("dvlp_xattn_index_ground_workspace_bytes", Bj, W, K, G)
        assert wb(1, 99, 10, 240) > 0 and wb(1000, 112, 10, 288) > 0 and wb(3, 1, 1, 1) > 0
        assert wb(1000, 99, 10, 240) == _lib.call("dvlp_xattn_index_query_workspace_bytes", 1000, 99)      # the caption side only: no new buffer
        assert wb(8, 99, 5, 240) == wb(8, 99, 500, 30)
        for bad in [(4, 113, 5, 240), (4, 99, 5, 289), (4, 99, 5, 1152), (0, 99, 5, 240), (4, 0, 5, 240), (4, 99, 0, 240), (4, 99, 5, 0), (65536, 99, 5, 240)]:
            assert wb(*bad) < 0, bad

    def test_bad_arguments_return_err_shape_without_launching(self):
        fn = getattr(_lib.load(), "dvlp_xattn_index_pairs_ground")
        ok = dict(cap=4, G=240, index=ONE, mimg=ONE, Bj=2, W=99, d=256, Q=ONE, mcap=ONE, cand=ONE, K=3, frames=8, score=ONE, ws=ONE, wr=ONE, rs=ONE,
                  wreg=ONE, wwt=ONE, rw=ONE, fs=ONE, work=ONE)
        bad = [dict(frames=7), dict(frames=9), dict(frames=-1), dict(frames=241), dict(frames=0), dict(fs=None), dict(d=128), dict(K=0), dict(K=-1), dict(cap=0), dict(G=0),
               dict(G=289, frames=1), dict(W=113), dict(W=0), dict(Bj=0), dict(Bj=65536), dict(index=None), dict(mimg=None), dict(Q=None), dict(mcap=None),
               dict(cand=None), dict(score=None), dict(ws=None), dict(rs=None), dict(wreg=None), dict(wwt=None), dict(rw=None), dict(work=None)]
        for b in bad:
            a = {**ok, **b}
            rc = fn(a["cap"], a["G"], a["index"], a["mimg"], a["Bj"], a["W"], a["d"], a["Q"], a["mcap"], a["cand"], a["K"], a["frames"], 20.0, 1,
                    a["score"], a["ws"], a["rs"], a["wreg"], a["wwt"], a["rw"], a["fs"], a["work"], None)
            assert rc == ERR_SHAPE, (b, rc)
        with pytest.raises(DemoVLPHipError):
            _lib.call("dvlp_xattn_index_pairs_ground", 4, 240, ONE, ONE, 2, 99, 256, ONE, ONE, ONE, 0, 8, 20.0, 1, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None)


class TestHostChecks:
    TEXT = dict(input_ids=torch.zeros(2, 100, dtype=torch.long), attention_mask=torch.ones(2, 100, dtype=torch.long))

    def test_ground_needs_the_fused_route_and_the_device(self):
        ids = torch.zeros(2, 3, dtype=torch.long)
        for ix in (search.VideoIndex(8, 30, torch.float32, device="cpu"), search.VideoIndex(8, 1152, torch.bfloat16, device="cpu")):
            ix.n = 8
            with pytest.raises(DemoVLPHipError, match="fused"):
                ix.ground(None, RWALoss(20, "equal"), self.TEXT, ids)
            with pytest.raises(DemoVLPHipError, match="fused"):
                ix.search(None, RWALoss(20, "equal"), self.TEXT, k=3, shortlist=5, ground=True)
        ix = search.VideoIndex(8, 30, torch.bfloat16, device="cpu")
        ix.n = 8
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.ground(None, RWALoss(20, "equal"), self.TEXT, ids)                              # well-formed, but on the host
        with pytest.raises(ValueError, match="divisor"):
            ix.ground(None, RWALoss(20, "equal"), self.TEXT, ids, frames=7)
        with pytest.raises(ValueError, match="divisor"):
            ix.search(None, RWALoss(20, "equal"), self.TEXT, k=3, shortlist=5, ground=True, frames=4)
        with pytest.raises(DemoVLPHipError):
            ix.search(None, RWALoss(20, "equal"), self.TEXT, k=3, shortlist=5, ground=True, frames=5)      # passes the checks, then needs the device

    def test_wrapper_refuses_host_tensors_and_wrong_arguments(self):
        index = torch.zeros(ops.xattn_index_bytes(2, 30), dtype=torch.uint8)
        mi, Q, mc, cand = torch.zeros(2, 30), torch.zeros(3, 20, 256, dtype=torch.bfloat16), torch.zeros(3, 20), torch.zeros(3, 2, dtype=torch.int32)
        with pytest.raises(DemoVLPHipError, match="MI355X|device|cuda|GPU"):
            ops.xattn_index_pairs_ground(index, 2, 30, mi, Q, mc, cand, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="bf16"):
            ops.xattn_index_pairs_ground(index, 2, 30, mi, Q.float(), mc, cand, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="cand"):
            ops.xattn_index_pairs_ground(index, 2, 30, mi, Q, mc, cand.long(), 20.0, True)
        with pytest.raises(DemoVLPHipError, match="masks"):
            ops.xattn_index_pairs_ground(index, 2, 30, mi[:, :29], Q, mc, cand, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="divisor"):
            ops.xattn_index_pairs_ground(index, 2, 30, mi, Q, mc, cand, 20.0, True, frames=4)
