"""Search for long videos, host side: the size helpers and argument checks of the ``dvlp_xattn_long_index_*`` entries (the region-tiled pair
kernel, G <= 1152) and the constructor rules of ``search.VideoIndex(..., tiled=True)``.  No GPU needed: every call returns before a launch.
``tests/test_gpu_long_search.py`` runs the kernel."""
import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (demovlp_amd/csrc/common.h)


class TestSizeHelpers:
    def test_index_bytes_range_and_scaling(self):
        ib = lambda c, G: _lib.call("dvlp_xattn_long_index_bytes", c, G)
        per = 1152 * 256 * 2 * 2 + 1152 * 4                               # both orientations in bf16 + the norms: ~1.18 MB
        assert ib(1, 1152) == per and ib(2, 1152) == 2 * per and ib(1000, 1152) == 1000 * per      # linear in the capacity
        assert 1.18e6 < per < 1.19e6
        assert ib(4, 1) > 0 and ib(4, 289) > 0 and ib(4, 1152) > 0
        assert ib(4, 0) < 0 and ib(4, 1153) < 0 and ib(0, 1152) < 0
        # one resident layout: inside the fused range a row costs what it costs in the short family, whose answers stay what they were
        assert ib(1, 288) == _lib.call("dvlp_xattn_index_bytes", 1, 288) and ib(7, 240) == _lib.call("dvlp_xattn_index_bytes", 7, 240)
        assert _lib.call("dvlp_xattn_index_bytes", 4, 289) < 0 and _lib.call("dvlp_xattn_index_bytes", 4, 1152) < 0
        assert ops.xattn_long_index_bytes(3, 960) == ib(3, 960)
        with pytest.raises(DemoVLPHipError):
            ops.xattn_long_index_bytes(3, 1153)

    def test_workspace_helpers(self):
        qb = lambda Bj, W: _lib.call("dvlp_xattn_long_index_query_workspace_bytes", Bj, W)
        gb = lambda Bj, W, K, G: _lib.call("dvlp_xattn_long_index_ground_workspace_bytes", Bj, W, K, G)
        assert qb(8, 99) == _lib.call("dvlp_xattn_index_query_workspace_bytes", 8, 99) > 0 and qb(1, 1) > 0 and qb(3, 112) > 0
        assert qb(4, 113) < 0 and qb(0, 99) < 0 and qb(4, 0) < 0
        assert gb(8, 99, 5, 1152) == qb(8, 99) and gb(8, 99, 500, 289) == qb(8, 99) and gb(3, 1, 1, 1) > 0
        for bad in [(4, 113, 5, 1152), (4, 99, 5, 1153), (0, 99, 5, 1152), (4, 0, 5, 1152), (4, 99, 0, 1152), (4, 99, 5, 0), (65536, 99, 5, 1152)]:
            assert gb(*bad) < 0, bad


class TestEntryArgumentChecks:
    def test_index_add_rejects(self):
        for args in [(4, 1152, 0, 5, ONE, ONE), (4, 1152, -1, 1, ONE, ONE), (4, 1152, 3, 2, ONE, ONE), (4, 1152, 0, 0, ONE, ONE), (0, 1152, 0, 1, ONE, ONE),
                     (4, 1153, 0, 1, ONE, ONE), (4, 1152, 0, 1, None, ONE), (4, 1152, 0, 1, ONE, None)]:
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_long_index_add", *args, None)

    def test_index_pairs_rejects(self):
        ok = dict(cap=4, G=1152, index=ONE, mimg=ONE, Bj=2, W=99, d=256, Q=ONE, mcap=ONE, K=3, cand=ONE, scores=ONE, ws=ONE)
        bad = [dict(d=128), dict(cap=0), dict(G=0), dict(G=1153), dict(W=113), dict(W=0), dict(Bj=0), dict(Bj=65536), dict(K=0), dict(index=None),
               dict(mimg=None), dict(Q=None), dict(mcap=None), dict(cand=None), dict(scores=None), dict(ws=None)]
        for b in bad:
            a = {**ok, **b}
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_long_index_pairs_fwd", a["cap"], a["G"], a["index"], a["mimg"], a["Bj"], a["W"], a["d"], a["Q"], a["mcap"], a["K"],
                          a["cand"], 20.0, 1, a["scores"], a["ws"], None)
        fn = getattr(_lib.load(), "dvlp_xattn_long_index_pairs_fwd")
        assert fn(4, 1152, ONE, ONE, 2, 99, 128, ONE, ONE, 3, ONE, 20.0, 1, ONE, ONE, None) == ERR_SHAPE          # d != 256

    def test_ground_returns_err_shape_without_launching(self):
        fn = getattr(_lib.load(), "dvlp_xattn_long_index_pairs_ground")
        ok = dict(cap=4, G=1152, index=ONE, mimg=ONE, Bj=2, W=99, d=256, Q=ONE, mcap=ONE, cand=ONE, K=3, frames=32, score=ONE, ws=ONE, wr=ONE, rs=ONE,
                  wreg=ONE, wwt=ONE, rw=ONE, fs=ONE, work=ONE)
        bad = [dict(frames=7), dict(frames=31), dict(frames=-1), dict(frames=1153), dict(frames=0), dict(fs=None), dict(d=128), dict(K=0), dict(K=-1),
               dict(cap=0), dict(G=0), dict(G=1153, frames=1), dict(W=113), dict(W=0), dict(Bj=0), dict(Bj=65536), dict(index=None), dict(mimg=None),
               dict(Q=None), dict(mcap=None), dict(cand=None), dict(score=None), dict(ws=None), dict(rs=None), dict(wreg=None), dict(wwt=None),
               dict(rw=None), dict(work=None)]
        for b in bad:
            a = {**ok, **b}
            rc = fn(a["cap"], a["G"], a["index"], a["mimg"], a["Bj"], a["W"], a["d"], a["Q"], a["mcap"], a["cand"], a["K"], a["frames"], 20.0, 1,
                    a["score"], a["ws"], a["rs"], a["wreg"], a["wwt"], a["rw"], a["fs"], a["work"], None)
            assert rc == ERR_SHAPE, (b, rc)

    def test_wrappers_refuse_host_tensors_and_wrong_arguments(self):
        index = torch.zeros(ops.xattn_long_index_bytes(2, 300), dtype=torch.uint8)
        mi, Q, mc, cand = torch.zeros(2, 300), torch.zeros(3, 20, 256, dtype=torch.bfloat16), torch.zeros(3, 20), torch.zeros(3, 2, dtype=torch.int32)
        with pytest.raises(DemoVLPHipError):
            ops.xattn_long_index_add(index, 2, 300, 0, torch.zeros(2, 300, 256))                               # fp32
        with pytest.raises(DemoVLPHipError):
            ops.xattn_long_index_add(index, 2, 300, 0, torch.zeros(2, 300, 256, dtype=torch.bfloat16))         # on the host
        for fn in (ops.xattn_long_index_pairs_fwd, ops.xattn_long_index_pairs_ground):
            with pytest.raises(DemoVLPHipError, match="MI355X|device|cuda|GPU"):
                fn(index, 2, 300, mi, Q, mc, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="bf16"):
                fn(index, 2, 300, mi, Q.float(), mc, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="cand"):
                fn(index, 2, 300, mi, Q, mc, cand.long(), 20.0, True)
            with pytest.raises(DemoVLPHipError, match="masks"):
                fn(index, 2, 300, mi[:, :29], Q, mc, cand, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="divisor"):
            ops.xattn_long_index_pairs_ground(index, 2, 300, mi, Q, mc, cand, 20.0, True, frames=7)


class TestConstructorRules:
    TEXT = dict(input_ids=torch.zeros(2, 100, dtype=torch.long), attention_mask=torch.ones(2, 100, dtype=torch.long))

    def test_tiled_needs_bf16_and_the_range(self):
        with pytest.raises(ValueError, match="tiled"):
            search.VideoIndex(4, 1152, torch.float32, tiled=True)
        with pytest.raises(ValueError, match="tiled"):
            search.VideoIndex(4, 1153, torch.bfloat16, tiled=True)
        ix = search.VideoIndex(4, 1152, torch.bfloat16, tiled=True)
        assert ix.tiled and not ix.fused
        short = search.VideoIndex(4, 240, torch.bfloat16, tiled=True)         # allowed inside the fused range too
        assert short.tiled and short.fused
        # the default is what it was
        plain = search.VideoIndex(10, 1152, torch.bfloat16)
        assert plain.fused is False and plain.tiled is False and search.VideoIndex(10, 240).tiled is False

    def test_ground_checks_pass_for_a_tiled_index_and_then_need_the_device(self):
        ix = search.VideoIndex(8, 1152, torch.bfloat16, device="cpu", tiled=True)
        ix.n = 8                                                               # (as if filled: the checks below are host logic)
        ids = torch.zeros(2, 3, dtype=torch.long)
        with pytest.raises(ValueError, match="divisor"):
            ix.ground(None, RWALoss(20, "equal"), self.TEXT, ids, frames=7)
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.ground(None, RWALoss(20, "equal"), self.TEXT, ids, frames=32)
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.search(None, RWALoss(20, "equal"), self.TEXT, k=3, shortlist=5, ground=True, frames=32)

    def test_state_dict_of_another_route_is_refused(self):
        tiled, plain = search.VideoIndex(4, 300, torch.bfloat16, device="cpu", tiled=True), search.VideoIndex(4, 300, torch.bfloat16, device="cpu")
        state = dict(capacity=4, G=300, dtype="bfloat16", n=0, fused=False, gn=None, om=None, local=None)
        with pytest.raises(ValueError, match="route"):
            tiled.load_state_dict(state)                                       # written by a default index: no 'tiled' key
        with pytest.raises(ValueError, match="route"):
            plain.load_state_dict({**state, "tiled": True})
