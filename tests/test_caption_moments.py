"""Moment search in the video-to-text direction, host side: the export and argument checks of ``dvlp_xattn_long_caption_index_moments_fwd``,
the ``ops`` wrapper and the rules of ``CaptionIndex.moments`` / ``search(..., moments=...)`` / ``timeline`` that hold before anything is
launched.  No GPU needed: every call returns before a launch.  ``tests/test_gpu_caption_moments.py`` runs the kernel."""
import inspect

import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (demovlp_amd/csrc/common.h)
ERR_UNSUPPORTED = -4
NAME = "dvlp_xattn_long_caption_index_moments_fwd"


class TestSymbol:
    def test_exported_and_bound(self):
        assert NAME in _lib.exported_symbols()
        fn = getattr(_lib.load(), NAME)
        assert fn.restype is _lib.ctypes.c_int and len(fn.argtypes) == 21
        # ... frames, win, stride, windows_per_group (int64), window_major (int), lam (float), gate (int), scores, workspace, stream
        assert fn.argtypes[11:15] == [_lib.ctypes.c_int64] * 4 and fn.argtypes[15:18] == [_lib.ctypes.c_int, _lib.ctypes.c_float, _lib.ctypes.c_int]
        sig = inspect.signature(ops.xattn_long_caption_index_moments_fwd)
        assert sig.parameters["window_major"].default is False and sig.parameters["windows_per_group"].default == 0


class TestEntryArgumentChecks:
    OK = dict(cap=4, W=99, index=ONE, mcap=ONE, Bi=2, G=1152, d=256, C=ONE, mimg=ONE, K=3, cand=ONE, frames=32, win=8, stride=1, wpg=0, major=0,
              scores=ONE, ws=ONE)
    BAD = [dict(d=128), dict(cap=0), dict(G=0), dict(G=1153, frames=1153), dict(G=1153, frames=1), dict(W=113), dict(W=0), dict(Bi=0),
           dict(Bi=65536), dict(K=0), dict(K=-1), dict(index=None), dict(mcap=None), dict(C=None), dict(mimg=None), dict(cand=None),
           dict(scores=None), dict(ws=None), dict(frames=7), dict(frames=0), dict(frames=-1), dict(frames=2304), dict(win=0), dict(win=33),
           dict(win=-1), dict(stride=0), dict(stride=-2), dict(wpg=-1), dict(wpg=-(1 << 40)),
           dict(Bi=65535, K=1 << 16),                    # Bi K > 2^31 - 1: the pair offsets
           dict(K=2 ** 31 // 25 + 1),                    # K M > 2^31 - 1 at M = 25: the grid axis
           dict(Bi=64, K=2 ** 31 // (25 * 64) + 1)]      # Bi K M > 2^31 - 1 with K M inside: the score offsets

    @staticmethod
    def _args(a):
        return (a["cap"], a["W"], a["index"], a["mcap"], a["Bi"], a["G"], a["d"], a["C"], a["mimg"], a["K"], a["cand"], a["frames"], a["win"],
                a["stride"], a["wpg"], a["major"], 20.0, 1, a["scores"], a["ws"], None)

    def test_every_bad_argument_is_refused_before_a_launch(self):
        fn = getattr(_lib.load(), NAME)
        for b in self.BAD:
            a = {**self.OK, **b}
            rc = fn(*self._args(a))
            assert rc in (ERR_SHAPE, ERR_UNSUPPORTED), (b, rc)
            assert (rc == ERR_UNSUPPORTED) == (a["G"] > 1152 or a["W"] > 112), (b, rc)
            with pytest.raises(DemoVLPHipError):
                _lib.call(NAME, *self._args(a))

    def test_what_the_count_refuses_is_refused_with_its_code(self):
        fn = getattr(_lib.load(), NAME)
        for b in [dict(frames=7), dict(win=0), dict(win=33), dict(stride=0), dict(G=1153, frames=1, win=1)]:
            a = {**self.OK, **b}
            want = _lib.call("dvlp_xattn_long_index_moments_count", a["G"], a["frames"], a["win"], a["stride"])
            assert want < 0 and fn(*self._args(a)) == want, b

    def test_wrapper_refuses_host_tensors_and_wrong_arguments(self):
        index = torch.zeros(ops.xattn_caption_index_bytes(2, 20), dtype=torch.uint8)
        mc, C, mi, cand = torch.zeros(2, 20), torch.zeros(3, 300, 256, dtype=torch.bfloat16), torch.zeros(3, 300), torch.zeros(3, 2, dtype=torch.int32)
        fn = ops.xattn_long_caption_index_moments_fwd
        for major in (False, True):
            with pytest.raises(DemoVLPHipError, match="MI355X|device|cuda|GPU"):
                fn(index, 2, 20, mc, C, mi, cand, 10, 3, 1, 20.0, True, window_major=major)
        with pytest.raises(DemoVLPHipError, match="bf16"):
            fn(index, 2, 20, mc, C.float(), mi, cand, 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="cand"):
            fn(index, 2, 20, mc, C, mi, cand.long(), 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="masks"):
            fn(index, 2, 20, mc, C, mi[:, :29], cand, 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="index buffer"):
            fn(index[:-1], 2, 20, mc, C, mi, cand, 10, 3, 1, 20.0, True)
        with pytest.raises(DemoVLPHipError, match="windows_per_group"):
            fn(index, 2, 20, mc, C, mi, cand, 10, 3, 1, 20.0, True, windows_per_group=-1)
        for frames, win, stride in [(7, 1, 1), (10, 0, 1), (10, 11, 1), (10, 3, 0)]:
            with pytest.raises(DemoVLPHipError, match="moments_count"):
                fn(index, 2, 20, mc, C, mi, cand, frames, win, stride, 20.0, True)


class TestCaptionIndexRules:
    DATA = dict(object=torch.zeros(2, 32, 36, 8), object_mask=torch.ones(2, 32, 36))       # G = 1152
    IDS = torch.zeros(2, 3, dtype=torch.long)
    LOSS = RWALoss(20, "equal")

    @staticmethod
    def _index(tiled=True, W=99, dtype=torch.bfloat16, n=8):
        ix = search.CaptionIndex(8, W, dtype, device="cpu", tiled=tiled)
        ix.n = n                                                           # (as if filled: the checks below are host logic)
        return ix

    def test_only_tiled_indexes_have_moments(self):
        for ix in (self._index(False), self._index(False, 113), self._index(False, 99, torch.float32)):
            with pytest.raises(DemoVLPHipError, match="tiled=True"):
                ix.moments(None, self.LOSS, self.DATA, self.IDS, 32, 2)
            with pytest.raises(DemoVLPHipError, match="tiled=True"):
                ix.search(None, self.LOSS, self.DATA, k=3, shortlist=5, frames=32, moments=(2,))
            with pytest.raises(DemoVLPHipError, match="tiled=True"):
                ix.timeline(None, self.LOSS, self.DATA, 32, 2, k=3, shortlist=5)

    def test_a_tiled_index_checks_its_arguments_and_then_needs_the_device(self):
        ix, loss = self._index(), self.LOSS
        with pytest.raises(ValueError, match="divisor"):
            ix.moments(None, loss, self.DATA, self.IDS, 7, 2)
        with pytest.raises(ValueError, match="divisor"):
            ix.timeline(None, loss, self.DATA, 7, 2, k=3, shortlist=5)
        with pytest.raises(ValueError, match="divisor"):
            ix.search(None, loss, self.DATA, k=3, shortlist=5, moments=(2,))              # moments need frames
        for windows, stride in [(0, 1), (33, 1), ((8, 33), 1), ((), 1), (8, 0)]:
            with pytest.raises(ValueError):
                ix.moments(None, loss, self.DATA, self.IDS, 32, windows, stride)
            with pytest.raises(ValueError):
                ix.search(None, loss, self.DATA, k=3, shortlist=5, frames=32, moments=windows, moment_stride=stride)
            with pytest.raises(ValueError):
                ix.timeline(None, loss, self.DATA, 32, windows, stride, k=3, shortlist=5)
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.moments(None, loss, self.DATA, self.IDS, 32, (4, 8))
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.search(None, loss, self.DATA, k=3, shortlist=5, frames=32, moments=(4, 8))
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
            ix.timeline(None, loss, self.DATA, 32, (4, 8), k=3, shortlist=5)

    def test_an_empty_index_and_bad_ids_are_refused(self):
        empty, ix, loss = self._index(n=0), self._index(), self.LOSS
        with pytest.raises(ValueError, match="empty"):
            empty.moments(None, loss, self.DATA, self.IDS, 32, 4)
        with pytest.raises(ValueError, match="empty"):
            empty.search(None, loss, self.DATA, k=3, shortlist=5, frames=32, moments=4)
        with pytest.raises(ValueError, match="empty"):
            empty.timeline(None, loss, self.DATA, 32, 4, k=3, shortlist=5)
        for ids in (self.IDS[0], self.IDS[:1], self.IDS.float(), torch.zeros(3, 3, dtype=torch.long)):
            with pytest.raises(ValueError, match="ids must be int"):
                ix.moments(None, loss, self.DATA, ids, 32, 4)

    def test_timeline_checks_k_shortlist_and_chunk_as_search_does(self):
        ix, loss = self._index(), self.LOSS
        for kw in (dict(k=0), dict(k=6, shortlist=5), dict(k=9, shortlist=None), dict(k=3, shortlist=5, chunk=0)):
            with pytest.raises(ValueError) as a:
                ix.timeline(None, loss, self.DATA, 32, 4, **kw)
            with pytest.raises(ValueError) as b:
                ix.search(None, loss, self.DATA, **kw)
            assert str(a.value) == str(b.value), kw
        big = search.CaptionIndex(5000, 99, torch.bfloat16, device="cpu", tiled=True)
        big.n = 5000
        with pytest.raises(ValueError, match="1024"):
            big.timeline(None, loss, self.DATA, 32, 4, k=3, shortlist=2000)
        sig = inspect.signature(search.CaptionIndex.timeline)
        assert [sig.parameters[n].default for n in ("stride", "k", "shortlist", "chunk")] == [1, 5, 100, 65536]

    def test_search_without_moments_returns_what_it_returned(self, monkeypatch):
        """the device stages replaced by host stand-ins: the tuple is (ids, scores) or (ids, scores, grounding) unless ``moments`` is given"""
        ix, loss = self._index(), self.LOSS
        sig = inspect.signature(search.CaptionIndex.search)
        assert sig.parameters["moments"].default is None and sig.parameters["moment_stride"].default == 1
        assert list(sig.parameters)[:9] == ["self", "model", "loss_fn", "data", "k", "shortlist", "chunk", "ground", "frames"]

        class Model:
            training = False

            def eval(self):
                return self

        data = {name: _Cuda(t) for name, t in self.DATA.items()}
        side = (torch.zeros(2, 256), torch.zeros(2, 1152, 256), torch.zeros(2, 1152))
        monkeypatch.setattr(search.CaptionIndex, "_blocks", staticmethod(lambda d: iter([(0, d)])))
        monkeypatch.setattr(search.CaptionIndex, "_video_side", lambda self, model, block: side)
        monkeypatch.setattr(search.CaptionIndex, "_score", lambda self, model, loss_fn, block, S, chunk, side=None: (
            None, torch.arange(5, dtype=torch.int32).expand(2, 5).contiguous(), torch.zeros(2, 5), torch.arange(5.0).expand(2, 5).contiguous()))
        monkeypatch.setattr(ops, "topk_rows", lambda x, K: tuple(t[:, :K].contiguous() for t in torch.sort(x, dim=1, descending=True, stable=True)))
        monkeypatch.setattr(search.CaptionIndex, "_ground_block", lambda self, loss_fn, side, ids, frames: dict(score=torch.zeros(ids.shape)))
        monkeypatch.setattr(search.CaptionIndex, "_moments_block", lambda self, loss_fn, side, ids, frames, windows, stride: dict(
            scores=torch.zeros(*ids.shape, len(windows[0])), start=windows[0], length=windows[1]))
        two = ix.search(Model(), loss, data, k=3, shortlist=5)
        assert isinstance(two, tuple) and len(two) == 2 and two[0].tolist() == [[4, 3, 2]] * 2 and two[1].tolist() == [[4.0, 3.0, 2.0]] * 2
        three = ix.search(Model(), loss, data, k=3, shortlist=5, ground=True, frames=32)
        assert len(three) == 3 and set(three[2]) == {"score"} and torch.equal(three[0], two[0])
        with_m = ix.search(Model(), loss, data, k=3, shortlist=5, frames=32, moments=(8, 32), moment_stride=8)
        assert len(with_m) == 3 and with_m[2]["start"].tolist() == [0, 8, 16, 24, 0] and with_m[2]["scores"].shape == (2, 3, 5)
        both = ix.search(Model(), loss, data, k=3, shortlist=5, ground=True, frames=32, moments=8)
        assert len(both) == 4 and set(both[2]) == {"score"} and both[3]["length"].tolist() == [8] * 25


class _Cuda:
    """a host tensor that says it is on the device: what the host-side rules of ``search`` look at, and nothing more"""

    def __init__(self, t):
        self.t, self.shape, self.is_cuda = t, t.shape, True
