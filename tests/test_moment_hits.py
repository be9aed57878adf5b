"""Moment retrieval, host side: the numpy restatement of ``dvlp_moment_select`` (``tests/moment_select_ref.py``) pinned by properties, the
argument checks of the entry and of ``ops.moment_select``, and the rules of ``VideoIndex.search_moments`` / ``moments(..., top=...)`` that
hold before anything is launched.  No GPU needed.  ``tests/test_gpu_moment_hits.py`` runs the kernel."""
import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss
from moment_select_ref import moment_select_ref, overlap, suppresses

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (demovlp_amd/csrc/common.h)
ERR_UNSUPPORTED = -4
IOUS = [0.0, 0.3, 0.5, 1.0]


def _windows(F, lengths, stride=1):
    s, l = search.moment_windows(F, lengths, stride)
    return s.numpy(), l.numpy()


def _rows(seed, P, M, quantised):
    x = np.random.default_rng(seed).standard_normal((P, M)).astype(np.float32)
    return (np.round(x * 2) / 4).astype(np.float32) if quantised else x          # multiples of 0.25 (and some -0.0): many ties


class TestTheRestatement:
    @pytest.mark.parametrize("iou", IOUS)
    @pytest.mark.parametrize("quantised", [False, True])
    def test_greedy_suppression_properties(self, iou, quantised):
        start, length = _windows(12, (1, 2, 4, 8))                              # M = 12 + 11 + 9 + 5
        M, T = start.size, 5
        x = _rows(11, 40, M, quantised)
        x[3, ::3] = -np.inf
        x[4, 5] = np.nan
        val, pos = moment_select_ref(x, start, length, T, iou)
        for r in range(x.shape[0]):
            picks = [int(p) for p in pos[r] if p >= 0]
            assert len(set(picks)) == len(picks) and (pos[r, len(picks):] == -1).all()
            assert np.array_equal(val[r, :len(picks)].view(np.uint32), x[r, picks].view(np.uint32))
            for a, p in enumerate(picks):                                       # no later pick overlaps an earlier one beyond iou
                inter, union = overlap(start, length, p)
                assert not suppresses(inter, union, iou)[picks[a + 1:]].any()
            assert all(x[r, picks[a]] >= x[r, picks[a + 1]] for a in range(len(picks) - 1))
            selectable = np.isfinite(x[r]) | np.isposinf(x[r])
            if len(picks) < T:                                                  # every selectable window left is suppressed by some pick
                gone = np.zeros(M, bool)
                for p in picks:
                    gone |= suppresses(*overlap(start, length, p), iou)
                    gone[p] = True
                assert gone[selectable].all()
                pad = val[r, len(picks):].view(np.uint32)
                assert (pad == (0x7FC00000 if np.isnan(x[r]).any() else 0xFF800000)).all()
            # greedy: pick a is the best (topk order) of the windows no earlier pick suppressed
            free = selectable.copy()
            for p in picks:
                cand = np.flatnonzero(free)
                assert p == cand[np.argmax(x[r, cand])]
                free &= ~suppresses(*overlap(start, length, p), iou)
                free[p] = False

    @pytest.mark.parametrize("quantised", [False, True])
    def test_iou_one_is_a_stable_descending_sort(self, quantised):
        start, length = _windows(16, (1, 2, 4, 8))
        M, T = start.size, 7
        x = _rows(5, 30, M, quantised)
        x[0, 1], x[0, 2] = 0.0, -0.0                                            # -0.0 == +0.0: position decides
        val, pos = moment_select_ref(x, start, length, T, 1.0)
        want = np.argsort(-x, axis=1, kind="stable")[:, :T]
        assert np.array_equal(pos, want.astype(np.int32))
        assert np.array_equal(val.view(np.uint32), np.take_along_axis(x, want, 1).view(np.uint32))

    def test_iou_zero_on_disjoint_windows_is_plain_top_t(self):
        for stride in (3, 5):
            start, length = _windows(60, 3, stride)                             # one length, stride >= length: no two windows overlap
            x = _rows(stride, 20, start.size, True)
            val, pos = moment_select_ref(x, start, length, 6, 0.0)
            assert np.array_equal(pos, np.argsort(-x, axis=1, kind="stable")[:, :6].astype(np.int32))

    def test_touching_windows_do_not_overlap_and_the_bound_itself_is_kept(self):
        start, length = np.array([0, 4, 2]), np.array([4, 4, 4])
        _, pos = moment_select_ref(np.array([[3.0, 2.0, 1.0]], np.float32), start, length, 3, 0.0)
        assert pos.tolist() == [[0, 1, -1]]                                     # [0, 4) and [4, 8) touch: inter = 0; [2, 6) overlaps both
        start, length = np.array([0, 1]), np.array([2, 1])                      # [0, 2) and [1, 2): inter / union = 1 / 2
        x = np.array([[1.0, 0.5]], np.float32)
        assert moment_select_ref(x, start, length, 2, 0.5)[1].tolist() == [[0, 1]]             # 1 > 2 * 0.5 is false: an overlap of exactly iou stays
        assert moment_select_ref(x, start, length, 2, 0.49)[1].tolist() == [[0, -1]]
        assert moment_select_ref(x, start, length, 2, 1.0)[1].tolist() == [[0, 1]]


class TestEntryArgumentChecks:
    OK = dict(P=5, M=85, scores=ONE, ld=88, start=ONE, length=ONE, T=3, iou=0.5, val=ONE, pos=ONE)
    SHAPE = [dict(scores=None), dict(start=None), dict(length=None), dict(val=None), dict(pos=None), dict(scores=ONE + 2), dict(pos=ONE + 1),
             dict(ld=84), dict(T=0), dict(T=-1), dict(M=0), dict(P=-1), dict(iou=-0.1), dict(iou=1.5), dict(iou=float("nan")),
             dict(P=2 ** 31 // 88 + 1), dict(P=2 ** 26, M=4, ld=4, T=32)]
    UNSUPPORTED = [dict(T=33), dict(M=4097, ld=4097)]

    @staticmethod
    def _args(a):
        return (a["P"], a["M"], a["scores"], a["ld"], a["start"], a["length"], a["T"], a["iou"], a["val"], a["pos"], None)

    def test_every_bad_argument_is_refused_before_a_launch(self):
        fn = getattr(_lib.load(), "dvlp_moment_select")
        for bad, code in [(b, ERR_SHAPE) for b in self.SHAPE] + [(b, ERR_UNSUPPORTED) for b in self.UNSUPPORTED]:
            assert fn(*self._args({**self.OK, **bad})) == code, bad
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_moment_select", *self._args({**self.OK, **bad}))

    def test_no_rows_is_no_launch(self):
        assert getattr(_lib.load(), "dvlp_moment_select")(*self._args({**self.OK, "P": 0})) == 0


class TestWrapperRefusals:
    X = torch.zeros(4, 6)

    def test_windows_on_the_host_are_validated(self):
        start, length = torch.arange(6), torch.full((6,), 2)
        for s, l, what in [(start[:5], length, "start"), (start, length[:5], "length"), (start - 1, length, "start"), (start, length - 2, "length"),
                           (start.float(), length, "start")]:
            with pytest.raises(ValueError, match=what):
                ops.moment_select(self.X, s, l, 2, 0.5)

    def test_limits_are_named(self):
        start, length = torch.arange(6), torch.full((6,), 2)
        for kw, what in [(dict(T=0), "T = 0"), (dict(T=33), "T = 33"), (dict(iou=-0.1), "iou"), (dict(iou=1.5), "iou"), (dict(M=7), "M = 7"),
                         (dict(M=0), "M = 0")]:
            with pytest.raises(ValueError, match=what):
                ops.moment_select(self.X, start, length, **{"T": 2, "iou": 0.5, **kw})
        with pytest.raises(ValueError, match="4096"):
            ops.moment_select(torch.zeros(1, 4097), torch.arange(4097), torch.ones(4097, dtype=torch.int64), 2, 0.5)
        with pytest.raises(DemoVLPHipError):
            ops.moment_select(self.X.double(), start, length, 2, 0.5)
        with pytest.raises(DemoVLPHipError, match="MI355X|device|GPU"):                # valid arguments: then it needs the device
            ops.moment_select(self.X, start, length, 2, 0.5)


class TestIndexRules:
    TEXT = dict(input_ids=torch.zeros(2, 100, dtype=torch.long), attention_mask=torch.ones(2, 100, dtype=torch.long))
    IDS = torch.zeros(2, 3, dtype=torch.long)
    DATA = dict(object=torch.zeros(2, 32, 36, 4), object_mask=torch.ones(2, 32, 36))
    LOSS = RWALoss(20, "equal")

    @staticmethod
    def _video_index(tiled=True):
        ix = search.VideoIndex(8, 1152, torch.bfloat16, device="cpu", tiled=tiled)
        ix.n = 8                                                              # (as if filled: the checks below are host logic)
        return ix

    @staticmethod
    def _caption_index(tiled=True):
        ix = search.CaptionIndex(8, 99, torch.bfloat16, device="cpu", tiled=tiled)
        ix.n = 8
        return ix

    def test_search_moments_refuses_before_the_device_is_touched(self):
        ix = self._video_index()
        ok = dict(k=3, frames=32, windows=(4,), stride=1, per_video=2, iou=0.5, shortlist=5)
        for bad, what in [(dict(per_video=0), "per_video = 0"), (dict(per_video=33), "per_video = 33"), (dict(iou=-0.1), "iou"), (dict(iou=1.5), "iou"),
                          (dict(k=11), "k = 11"), (dict(k=0), "k = 0"), (dict(k=9, per_video=1, shortlist=None), "k = 9"), (dict(frames=7), "frames = 7"),
                          (dict(frames=None), "frames"), (dict(windows=(1,) * 129), "4128"), (dict(windows=33), "33"), (dict(stride=0), "stride"),
                          (dict(shortlist=5, chunk=0), "chunk")]:
            with pytest.raises(ValueError, match=what):
                ix.search_moments(None, self.LOSS, self.TEXT, **{**ok, **bad})
        with pytest.raises(ValueError, match="tiled"):
            self._video_index(tiled=False).search_moments(None, self.LOSS, self.TEXT, **ok)
        big = search.VideoIndex(2000, 1152, torch.bfloat16, device="cpu", tiled=True)
        big.n = 2000
        with pytest.raises(ValueError, match="1024"):
            big.search_moments(None, self.LOSS, self.TEXT, **{**ok, "k": 1025, "per_video": 2, "shortlist": 1000})
        with pytest.raises(DemoVLPHipError, match="no CPU fallback"):           # every rule passed: then it needs the device
            ix.search_moments(None, self.LOSS, self.TEXT, **ok)

    def test_moments_with_top_refuses_before_the_device_is_touched(self):
        for ix, q, name in [(self._video_index(), self.TEXT, "video"), (self._caption_index(), self.DATA, "caption")]:
            for kw, what in [(dict(top=0), "top = 0"), (dict(top=33), "top = 33"), (dict(top=2, iou=-0.1), "iou"), (dict(top=2, iou=1.5), "iou")]:
                with pytest.raises(ValueError, match=what):
                    ix.moments(None, self.LOSS, q, self.IDS, 32, (4, 8), **kw)
                with pytest.raises(ValueError, match=what.replace("top", "moment_top")):
                    ix.search(None, self.LOSS, q, k=3, shortlist=5, frames=32, moments=(4, 8), moment_top=kw["top"], moment_iou=kw.get("iou", 0.5))
            with pytest.raises(ValueError, match="divisor"):
                ix.moments(None, self.LOSS, q, self.IDS, 7, (4, 8), top=2)
            with pytest.raises(ValueError, match="4128"):
                ix.moments(None, self.LOSS, q, self.IDS, 32, (1,) * 129, top=2)
            with pytest.raises(ValueError, match="moments"):                    # moment_top without moments
                ix.search(None, self.LOSS, q, k=3, shortlist=5, frames=32, moment_top=2)
            with pytest.raises(DemoVLPHipError, match="no CPU fallback"):
                ix.moments(None, self.LOSS, q, self.IDS, 32, (4, 8), top=2)
        with pytest.raises(ValueError, match="tiled"):
            self._video_index(tiled=False).moments(None, self.LOSS, self.TEXT, self.IDS, 32, (4, 8), top=2)
        with pytest.raises(ValueError, match="tiled"):
            self._caption_index(tiled=False).moments(None, self.LOSS, self.DATA, self.IDS, 32, (4, 8), top=2)

    def test_without_top_the_old_refusals_stand(self):
        with pytest.raises(DemoVLPHipError, match="tiled=True"):
            self._video_index(tiled=False).moments(None, self.LOSS, self.TEXT, self.IDS, 32, (4, 8))
