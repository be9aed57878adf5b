"""Video-to-text search for long videos, host side: the size helpers and argument checks of the ``dvlp_xattn_long_caption_index_*`` entries
(the region-tiled pair kernel on the video-major grid, G <= 1152), the ``ops`` wrappers and the constructor rules of
``search.CaptionIndex(..., tiled=True)``.  No GPU needed: every call returns before a launch.  ``tests/test_gpu_long_caption_search.py`` runs
the kernels."""
import inspect

import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (demovlp_amd/csrc/common.h)


class TestSizeHelpers:
    def test_query_workspace(self):
        qb = lambda Bi, G, W: _lib.call("dvlp_xattn_long_caption_index_query_workspace_bytes", Bi, G, W)
        short = lambda Bi, G, W: _lib.call("dvlp_xattn_caption_index_query_workspace_bytes", Bi, G, W)
        # inside the fused range: the video-side scratch of the short family, whose answers stay what they were
        for shape in [(8, 288, 99), (3, 240, 99), (1, 1, 1), (5, 129, 7)]:
            assert qb(*shape) == short(*shape) > 0, shape
        assert short(4, 289, 99) < 0 and short(4, 1152, 99) < 0
        per = 1152 * 256 * 2 * 2 + 1152 * 4                               # both orientations in bf16 + the norms: ~1.18 MB per video
        assert qb(1, 1152, 99) == per and qb(7, 1152, 1) == 7 * per and qb(65535, 1152, 112) > 0
        for bad in [(4, 1153, 99), (4, 1152, 113), (65536, 1152, 99), (0, 1152, 99), (4, 0, 99), (4, 1152, 0)]:
            assert qb(*bad) < 0, bad

    def test_ground_workspace(self):
        qb = lambda Bi, G, W: _lib.call("dvlp_xattn_long_caption_index_query_workspace_bytes", Bi, G, W)
        gb = lambda Bi, G, K, W: _lib.call("dvlp_xattn_long_caption_index_ground_workspace_bytes", Bi, G, K, W)
        short = lambda Bi, G, K, W: _lib.call("dvlp_xattn_caption_index_ground_workspace_bytes", Bi, G, K, W)
        for shape in [(8, 288, 5, 99), (3, 240, 500, 99), (1, 1, 1, 1)]:
            assert gb(*shape) == short(*shape) > 0, shape
        assert gb(8, 1152, 5, 99) == qb(8, 1152, 99) > 0 and gb(8, 289, 500, 37) == qb(8, 289, 37)
        for bad in [(4, 1153, 5, 99), (4, 1152, 5, 113), (65536, 1152, 5, 99), (0, 1152, 5, 99), (4, 0, 5, 99), (4, 1152, 0, 99), (4, 1152, 5, 0),
                    (65535, 1152, 1 << 16, 99)]:                          # the last: Bi K > INT32_MAX
            assert gb(*bad) < 0, bad


class TestEntryArgumentChecks:
    def test_pairs_fwd_rejects(self):
        ok = dict(cap=4, W=99, index=ONE, mcap=ONE, Bi=2, G=1152, d=256, C=ONE, mimg=ONE, K=3, cand=ONE, scores=ONE, ws=ONE)
        bad = [dict(d=128), dict(cap=0), dict(G=0), dict(G=1153), dict(W=113), dict(W=0), dict(Bi=0), dict(Bi=65536), dict(K=0),
               dict(Bi=65535, K=1 << 16), dict(index=None), dict(mcap=None), dict(C=None), dict(mimg=None), dict(cand=None), dict(scores=None),
               dict(ws=None)]
        for b in bad:
            a = {**ok, **b}
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_long_caption_index_pairs_fwd", a["cap"], a["W"], a["index"], a["mcap"], a["Bi"], a["G"], a["d"], a["C"],
                          a["mimg"], a["K"], a["cand"], 20.0, 1, a["scores"], a["ws"], None)
        fn = getattr(_lib.load(), "dvlp_xattn_long_caption_index_pairs_fwd")
        assert fn(4, 99, ONE, ONE, 2, 1152, 128, ONE, ONE, 3, ONE, 20.0, 1, ONE, ONE, None) == ERR_SHAPE          # d != 256
        assert fn(4, 99, ONE, ONE, 2, 1153, 256, ONE, ONE, 3, ONE, 20.0, 1, ONE, ONE, None) == -4                 # as dvlp_xattn_long_index_pairs_fwd
        assert fn(4, 113, ONE, ONE, 2, 1152, 256, ONE, ONE, 3, ONE, 20.0, 1, ONE, ONE, None) == -4

    def test_ground_returns_err_shape_without_launching(self):
        fn = getattr(_lib.load(), "dvlp_xattn_long_caption_index_pairs_ground")
        ok = dict(cap=4, W=99, index=ONE, mcap=ONE, Bi=2, G=1152, d=256, C=ONE, mimg=ONE, cand=ONE, K=3, frames=32, score=ONE, ws=ONE, rs=ONE,
                  wreg=ONE, wwt=ONE, rw=ONE, fs=ONE, work=ONE)
        bad = [dict(frames=7), dict(frames=31), dict(frames=-1), dict(frames=1153), dict(frames=0), dict(fs=None), dict(d=128), dict(K=0), dict(K=-1),
               dict(cap=0), dict(G=0), dict(G=1153, frames=1), dict(W=113), dict(W=0), dict(Bi=0), dict(Bi=65536), dict(Bi=65535, K=1 << 16),
               dict(index=None), dict(mcap=None), dict(C=None), dict(mimg=None), dict(cand=None), dict(score=None), dict(ws=None), dict(rs=None),
               dict(wreg=None), dict(wwt=None), dict(rw=None), dict(work=None)]
        for b in bad:
            a = {**ok, **b}
            rc = fn(a["cap"], a["W"], a["index"], a["mcap"], a["Bi"], a["G"], a["d"], a["C"], a["mimg"], a["cand"], a["K"], a["frames"], 20.0, 1,
                    a["score"], a["ws"], a["rs"], a["wreg"], a["wwt"], a["rw"], a["fs"], a["work"], None)
            assert rc == ERR_SHAPE, (b, rc)

    def test_wrappers_refuse_host_tensors_and_wrong_arguments(self):
        index = torch.zeros(ops.xattn_caption_index_bytes(2, 20), dtype=torch.uint8)
        mc, C, mi, cand = torch.zeros(2, 20), torch.zeros(3, 300, 256, dtype=torch.bfloat16), torch.zeros(3, 300), torch.zeros(3, 2, dtype=torch.int32)
        for fn in (ops.xattn_long_caption_index_pairs_fwd, ops.xattn_long_caption_index_pairs_ground):
            with pytest.raises(DemoVLPHipError, match="MI355X|device|cuda|GPU"):
                fn(index, 2, 20, mc, C, mi, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="bf16"):
                fn(index, 2, 20, mc, C.float(), mi, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="cand"):
                fn(index, 2, 20, mc, C, mi, cand.long(), 20.0, True)
            with pytest.raises(DemoVLPHipError, match="masks"):
                fn(index, 2, 20, mc, C, mi[:, :29], cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="index buffer"):
                fn(index[:-1], 2, 20, mc, C, mi, cand, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="divisor"):
            ops.xattn_long_caption_index_pairs_ground(index, 2, 20, mc, C, mi, cand, 20.0, True, frames=7)


class TestConstructorRules:
    def test_tiled_needs_bf16_and_the_range(self):
        with pytest.raises(ValueError, match="tiled"):
            search.CaptionIndex(4, 99, torch.float32, tiled=True)
        with pytest.raises(ValueError, match="tiled"):
            search.CaptionIndex(4, 113, torch.bfloat16, tiled=True)
        ix = search.CaptionIndex(4, 99, torch.bfloat16, tiled=True)
        assert ix.tiled and ix.fused                                      # one resident layout: the bytes of a fused index
        # the defaults are what they were
        plain = search.CaptionIndex(4, 99, torch.bfloat16)
        assert plain.fused and plain.tiled is False
        assert search.CaptionIndex(4, 113, torch.bfloat16).fused is False and search.CaptionIndex(4, 99, torch.float32).tiled is False

    def test_ground_checks_pass_for_a_tiled_index_and_then_need_the_device(self):
        ix = search.CaptionIndex(8, 99, torch.bfloat16, device="cpu", tiled=True)
        ix.n = 8                                                          # (as if filled: the checks below are host logic)
        data = dict(object=torch.zeros(2, 32, 36, 8), object_mask=torch.ones(2, 32, 36))       # G = 1152
        ids = torch.zeros(2, 3, dtype=torch.long)
        with pytest.raises(ValueError, match="divisor"):
            ix.ground(None, RWALoss(20, "equal"), data, ids, frames=7)
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.ground(None, RWALoss(20, "equal"), data, ids, frames=32)
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.search(None, RWALoss(20, "equal"), data, k=3, shortlist=5, ground=True, frames=32)

    def test_state_dict_of_another_route_is_refused(self):
        tiled, plain = search.CaptionIndex(4, 99, torch.bfloat16, device="cpu", tiled=True), search.CaptionIndex(4, 99, torch.bfloat16, device="cpu")
        state = dict(capacity=4, W=99, dtype="bfloat16", n=0, fused=True, gn=None, tm=None, local=None)
        with pytest.raises(ValueError, match="route"):
            tiled.load_state_dict(state)                                  # written by a default index: no 'tiled' key
        with pytest.raises(ValueError, match="route"):
            plain.load_state_dict({**state, "tiled": True})

    def test_evaluate_v2t_accepts_tiled(self):
        sig = inspect.signature(search.evaluate_v2t)
        assert "tiled" in sig.parameters and sig.parameters["tiled"].default is False
        assert inspect.signature(search.CaptionIndex.__init__).parameters["tiled"].default is False
