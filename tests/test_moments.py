"""Moment search, host side: ``search.moment_windows``, the window arithmetic and argument checks of ``dvlp_xattn_long_index_moments_*`` and
the rules of ``VideoIndex.moments`` / ``search(..., moments=...)`` that hold before anything is launched.  No GPU needed.
``tests/test_gpu_moments.py`` runs the kernel."""
import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (demovlp_amd/csrc/common.h)
ERR_UNSUPPORTED = -4


class TestMomentWindows:
    def test_lengths_in_the_order_given_starts_ascending(self):
        starts, lengths = search.moment_windows(32, (8, 32), 4)
        assert starts.dtype == torch.int64 and lengths.dtype == torch.int64
        assert starts.tolist() == [0, 4, 8, 12, 16, 20, 24, 0] and lengths.tolist() == [8] * 7 + [32]
        starts, lengths = search.moment_windows(3, 1, 1)
        assert starts.tolist() == [0, 1, 2] and lengths.tolist() == [1, 1, 1]
        starts, lengths = search.moment_windows(10, [10, 2], 3)               # the order given, not sorted; the last start is 6: 6 + 2 <= 10
        assert starts.tolist() == [0, 0, 3, 6] and lengths.tolist() == [10, 2, 2, 2]

    @pytest.mark.parametrize("frames,windows,stride", [(32, 0, 1), (32, 33, 1), (32, 8, 0), (32, (), 1), (32, (8, 33), 1), (0, 1, 1)])
    def test_refusals(self, frames, windows, stride):
        with pytest.raises(ValueError):
            search.moment_windows(frames, windows, stride)


class TestCount:
    def test_values_and_refusals(self):
        cnt = lambda *a: _lib.call("dvlp_xattn_long_index_moments_count", *a)
        assert cnt(1152, 32, 8, 4) == 7 and cnt(1152, 32, 32, 4) == 1 and cnt(3, 3, 1, 1) == 3 and cnt(1152, 32, 1, 1) == 32
        assert cnt(300, 10, 3, 1) == 8 and cnt(16, 16, 1, 5) == 4 and cnt(1152, 32, 31, 1) == 2
        assert cnt(1152, 7, 1, 1) < 0                      # frames does not divide G
        assert cnt(1153, 1153, 1, 1) < 0 and cnt(1153, 1, 1, 1) == ERR_UNSUPPORTED      # G out of range
        for bad in [(1152, 32, 0, 1), (1152, 32, 33, 1), (1152, 32, 8, 0), (1152, 0, 1, 1), (0, 1, 1, 1), (1152, 32, -1, 1), (1152, 2304, 1, 1)]:
            assert cnt(*bad) == ERR_SHAPE, bad


class TestEntryArgumentChecks:
    OK = dict(cap=4, G=1152, index=ONE, mimg=ONE, Bj=2, W=99, d=256, Q=ONE, mcap=ONE, K=3, cand=ONE, frames=32, win=8, stride=1, scores=ONE, ws=ONE)
    BAD = [dict(d=128), dict(cap=0), dict(G=0), dict(G=1153, frames=1153), dict(W=113), dict(W=0), dict(Bj=0), dict(Bj=65536), dict(K=0),
           dict(index=None), dict(mimg=None), dict(Q=None), dict(mcap=None), dict(cand=None), dict(scores=None), dict(ws=None),
           dict(frames=7), dict(frames=0), dict(frames=-1), dict(win=0), dict(win=33), dict(stride=0), dict(stride=-2), dict(K=2 ** 31 // 25 + 1)]

    @staticmethod
    def _args(a):
        return (a["cap"], a["G"], a["index"], a["mimg"], a["Bj"], a["W"], a["d"], a["Q"], a["mcap"], a["K"], a["cand"], a["frames"], a["win"],
                a["stride"], 20.0, 1, a["scores"], a["ws"], None)

    def test_every_bad_argument_is_refused_before_a_launch(self):
        fn = getattr(_lib.load(), "dvlp_xattn_long_index_moments_fwd")
        for b in self.BAD:
            a = {**self.OK, **b}
            rc = fn(*self._args(a))
            assert rc in (ERR_SHAPE, ERR_UNSUPPORTED), (b, rc)
            assert (rc == ERR_UNSUPPORTED) == (a["G"] > 1152 or a["W"] > 112), (b, rc)
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_long_index_moments_fwd", *self._args(a))
        assert fn(*self._args({**self.OK, "d": 128})) == ERR_SHAPE

    def test_wrapper_refuses_host_tensors_and_wrong_arguments(self):
        index = torch.zeros(ops.xattn_long_index_bytes(2, 300), dtype=torch.uint8)
        mi, Q, mc, cand = torch.zeros(2, 300), torch.zeros(3, 20, 256, dtype=torch.bfloat16), torch.zeros(3, 20), torch.zeros(3, 2, dtype=torch.int32)
        fn = ops.xattn_long_index_moments_fwd
        with pytest.raises(DemoVLPHipError, match="MI355X|device|cuda|GPU"):
            fn(index, 2, 300, mi, Q, mc, cand, 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="bf16"):
            fn(index, 2, 300, mi, Q.float(), mc, cand, 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="cand"):
            fn(index, 2, 300, mi, Q, mc, cand.long(), 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="masks"):
            fn(index, 2, 300, mi[:, :29], Q, mc, cand, 10, 3, 1, 20.0, True)
        for frames, win, stride in [(7, 1, 1), (10, 0, 1), (10, 11, 1), (10, 3, 0)]:
            with pytest.raises(DemoVLPHipError, match="moments_count"):
                fn(index, 2, 300, mi, Q, mc, cand, frames, win, stride, 20.0, True)


class TestVideoIndexRules:
    TEXT = dict(input_ids=torch.zeros(2, 100, dtype=torch.long), attention_mask=torch.ones(2, 100, dtype=torch.long))
    IDS = torch.zeros(2, 3, dtype=torch.long)

    def test_only_tiled_indexes_have_moments(self):
        for ix in (search.VideoIndex(8, 1152, torch.bfloat16, device="cpu"), search.VideoIndex(8, 240, torch.bfloat16, device="cpu"),
                   search.VideoIndex(8, 240, torch.float32, device="cpu")):
            ix.n = 8                                                           # (as if filled: the checks below are host logic)
            with pytest.raises(DemoVLPHipError, match="tiled=True"):
                ix.moments(None, RWALoss(20, "equal"), self.TEXT, self.IDS, ix.G // 36 if ix.G > 240 else 8, 2)
            with pytest.raises(DemoVLPHipError, match="tiled=True"):
                ix.search(None, RWALoss(20, "equal"), self.TEXT, k=3, shortlist=5, frames=8, moments=(2,))

    def test_a_tiled_index_checks_its_arguments_and_then_needs_the_device(self):
        ix = search.VideoIndex(8, 1152, torch.bfloat16, device="cpu", tiled=True)
        ix.n = 8
        loss = RWALoss(20, "equal")
        with pytest.raises(ValueError, match="divisor"):
            ix.moments(None, loss, self.TEXT, self.IDS, 7, 2)
        with pytest.raises(ValueError, match="divisor"):
            ix.search(None, loss, self.TEXT, k=3, shortlist=5, moments=(2,))              # moments need frames
        for windows, stride in [(0, 1), (33, 1), ((8, 33), 1), ((), 1), (8, 0)]:
            with pytest.raises(ValueError):
                ix.moments(None, loss, self.TEXT, self.IDS, 32, windows, stride)
            with pytest.raises(ValueError):
                ix.search(None, loss, self.TEXT, k=3, shortlist=5, frames=32, moments=windows, moment_stride=stride)
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.moments(None, loss, self.TEXT, self.IDS, 32, (4, 8))
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.search(None, loss, self.TEXT, k=3, shortlist=5, frames=32, moments=(4, 8))
