"""Video-to-text search, host side: the size helpers and argument checks of the six ``dvlp_xattn_caption_index_*`` entries and the host
checks of ``search.CaptionIndex`` (no GPU needed for any of them)."""
import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched


class TestCaptionEntrySizeHelpers:
    def test_one_caption_of_99_words_takes_123392_bytes(self):
        # qhat [112][256] bf16 + qhatT [256][128] bf16 + nq [99] fp32 rounded up to 256 bytes
        assert 112 * 256 * 2 == 57344 and 256 * 128 * 2 == 65536
        assert _lib.call("dvlp_xattn_caption_index_bytes", 1, 99) == 57344 + 65536 + 512 == 123392
        assert ops.xattn_caption_index_bytes(1, 99) == 123392

    def test_index_bytes_scale_linearly_in_the_capacity(self):
        ib = lambda c, W: _lib.call("dvlp_xattn_caption_index_bytes", c, W)
        per = 96 * 256 * 2 * 2 + 96 * 4                                    # W = 96: no padding in either orientation
        assert ib(2, 96) == 2 * per and ib(1000, 96) == 1000 * per and ib(100000, 96) == 100000 * per
        assert ib(64, 99) == 64 * (57344 + 65536 + 99 * 4)                 # 64 x 396 bytes of norms is a multiple of 256
        assert ib(100000, 99) == 100000 * (57344 + 65536) + 39600128      # 39.6 MB of norms rounded up to 256

    def test_negative_codes_outside_the_range(self):
        ib = lambda c, W: _lib.call("dvlp_xattn_caption_index_bytes", c, W)
        qb = lambda Bi, G, W: _lib.call("dvlp_xattn_caption_index_query_workspace_bytes", Bi, G, W)
        gb = lambda Bi, G, K, W: _lib.call("dvlp_xattn_caption_index_ground_workspace_bytes", Bi, G, K, W)
        assert ib(4, 0) < 0 and ib(4, 113) < 0 and ib(0, 99) < 0 and ib(4, 112) > 0
        assert qb(4, 289, 99) < 0 and qb(65536, 240, 99) < 0 and qb(4, 240, 113) < 0 and qb(0, 240, 99) < 0 and qb(4, 0, 99) < 0
        # the per-call prep of the videos: chat [240][256] + chatT [256][256] bf16 per video + the region norms; independent of any capacity
        assert qb(8, 240, 99) == 8 * (240 * 512 + 256 * 256 * 2) + 7680
        assert qb(65535, 288, 112) > 0
        assert gb(8, 240, 5, 99) == qb(8, 240, 99) and gb(8, 289, 5, 99) < 0 and gb(65536, 240, 5, 99) < 0 and gb(8, 240, 0, 99) < 0
        with pytest.raises(DemoVLPHipError):
            ops.xattn_caption_index_bytes(4, 113)


class TestCaptionEntryArgumentChecks:
    def test_index_add_rejects(self):
        for args in [(4, 99, 0, 5, ONE, ONE), (4, 99, -1, 1, ONE, ONE), (4, 99, 3, 2, ONE, ONE), (4, 99, 0, 0, ONE, ONE), (0, 99, 0, 1, ONE, ONE),
                     (4, 113, 0, 1, ONE, ONE), (4, 0, 0, 1, ONE, ONE), (4, 99, 0, 1, None, ONE), (4, 99, 0, 1, ONE, None)]:
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_caption_index_add", *args, None)

    def test_index_pairs_rejects(self):
        ok = dict(cap=4, W=99, index=ONE, mcap=ONE, Bi=2, G=240, d=256, C=ONE, mimg=ONE, K=3, cand=ONE, scores=ONE, ws=ONE)
        bad = [dict(d=128), dict(cap=0), dict(G=0), dict(G=289), dict(W=113), dict(W=0), dict(Bi=0), dict(Bi=65536), dict(K=0), dict(index=None),
               dict(mimg=None), dict(C=None), dict(mcap=None), dict(cand=None), dict(scores=None), dict(ws=None), dict(Bi=65535, K=1 << 20)]
        for b in bad:
            a = {**ok, **b}
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_caption_index_pairs_fwd", a["cap"], a["W"], a["index"], a["mcap"], a["Bi"], a["G"], a["d"], a["C"], a["mimg"],
                          a["K"], a["cand"], 20.0, 1, a["scores"], a["ws"], None)

    def test_index_pairs_ground_rejects(self):
        ok = dict(cap=4, W=99, index=ONE, mcap=ONE, Bi=2, G=240, d=256, C=ONE, mimg=ONE, cand=ONE, K=3, frames=8, score=ONE, ws_=ONE, rs=ONE,
                  wr=ONE, ww=ONE, rw=ONE, fs=ONE, ws=ONE)
        bad = [dict(d=128), dict(cap=0), dict(G=0), dict(G=289), dict(W=113), dict(W=0), dict(Bi=0), dict(Bi=65536), dict(K=0), dict(index=None),
               dict(mimg=None), dict(C=None), dict(mcap=None), dict(cand=None), dict(score=None), dict(ws_=None), dict(rs=None), dict(wr=None),
               dict(ww=None), dict(rw=None), dict(ws=None), dict(frames=7), dict(frames=-1), dict(frames=0), dict(fs=None), dict(frames=480)]
        for b in bad:
            a = {**ok, **b}
            with pytest.raises(DemoVLPHipError, match="SHAPE|shape"):
                _lib.call("dvlp_xattn_caption_index_pairs_ground", a["cap"], a["W"], a["index"], a["mcap"], a["Bi"], a["G"], a["d"], a["C"],
                          a["mimg"], a["cand"], a["K"], a["frames"], 20.0, 1, a["score"], a["ws_"], a["rs"], a["wr"], a["ww"], a["rw"], a["fs"],
                          a["ws"], None)


def _caps(n, W, dtype=torch.bfloat16):
    return torch.zeros(n, 256, dtype=dtype), torch.zeros(n, W, 256, dtype=dtype), torch.ones(n, W + 1, dtype=torch.long)


def _videos(n, F=2, R=15):
    return dict(object=torch.zeros(n, F, R, 2054), object_mask=torch.ones(n, F, R))


class TestCaptionIndexHostChecks:
    def test_route_follows_dtype_and_word_count(self):
        assert search.CaptionIndex(10, 99, torch.bfloat16).fused and search.CaptionIndex(10, 112, "bfloat16").fused
        assert not search.CaptionIndex(10, 99, torch.float32).fused and not search.CaptionIndex(10, 113, torch.bfloat16).fused
        with pytest.raises(ValueError):
            search.CaptionIndex(0, 99)
        with pytest.raises(ValueError):
            search.CaptionIndex(4, 0)
        with pytest.raises(ValueError):
            search.CaptionIndex(4, 99, torch.float16)

    def test_add_checks_then_needs_the_device(self):
        ix = search.CaptionIndex(4, 20, torch.bfloat16, device="cpu")
        assert len(ix) == 0
        with pytest.raises(ValueError, match="W = 20"):
            ix.add(*_caps(2, 21))                                          # another width: no silent padding
        with pytest.raises(ValueError, match="W = 20"):
            ix.add(*_caps(2, 19))
        g, l, a = _caps(2, 20)
        with pytest.raises(ValueError):
            ix.add(g, l, a[:, :-1])                                        # the mask without its CLS position
        with pytest.raises(ValueError, match="capacity"):
            ix.add(*_caps(5, 20))                                          # past the capacity
        with pytest.raises(ValueError, match="bfloat16"):
            ix.add(*_caps(2, 20, torch.float32))
        with pytest.raises(DemoVLPHipError):
            ix.add(*_caps(2, 20))                                          # well-formed, but on the host
        assert len(ix) == 0

    def test_search_checks_then_needs_the_device(self):
        ix = search.CaptionIndex(64, 20, torch.bfloat16, device="cpu")
        data, loss = _videos(2), RWALoss(20, "equal")
        with pytest.raises(ValueError, match="empty"):
            ix.search(None, loss, data)
        ix.n = 50                                                          # (as if filled: the checks below are host logic)
        with pytest.raises(ValueError, match="shortlist"):
            ix.search(None, loss, data, k=11, shortlist=10)
        with pytest.raises(ValueError, match="shortlist"):
            ix.search(None, loss, data, k=51, shortlist=None)
        with pytest.raises(ValueError):
            ix.search(None, loss, data, k=0)
        with pytest.raises(ValueError):
            ix.search(None, loss, data, chunk=0)
        with pytest.raises(ValueError, match="divisor"):
            ix.search(None, loss, data, k=10, shortlist=20, ground=True, frames=7)      # G = 30
        with pytest.raises(DemoVLPHipError):
            ix.search(None, loss, data, k=10, shortlist=20)
        big = search.CaptionIndex(5000, 20, torch.bfloat16, device="cpu")
        big.n = 5000
        with pytest.raises(ValueError, match="1024"):
            big.search(None, loss, data, k=10, shortlist=2000)
        with pytest.raises(ValueError, match="1024"):
            big.search(None, loss, data, k=2000, shortlist=None)

    def test_the_shared_checks_give_video_index_the_same_errors(self):
        v, c = search.VideoIndex(64, 30, device="cpu"), search.CaptionIndex(64, 20, device="cpu")
        text = dict(input_ids=torch.zeros(2, 21, dtype=torch.long), attention_mask=torch.ones(2, 21, dtype=torch.long))
        v.n = c.n = 50
        for kw in (dict(k=11, shortlist=10), dict(k=0), dict(chunk=0)):
            with pytest.raises(ValueError) as ev:
                v.search(None, RWALoss(20, "equal"), text, **kw)
            with pytest.raises(ValueError) as ec:
                c.search(None, RWALoss(20, "equal"), _videos(2), **kw)
            assert str(ev.value) == str(ec.value)

    def test_ground_refuses_the_parity_route(self):
        ids = torch.zeros(2, 3, dtype=torch.long)
        for ix in (search.CaptionIndex(8, 20, torch.float32, device="cpu"), search.CaptionIndex(8, 113, torch.bfloat16, device="cpu")):
            ix.n = 8
            with pytest.raises(DemoVLPHipError, match="fused"):
                ix.ground(None, RWALoss(20, "equal"), _videos(2), ids)
            with pytest.raises(DemoVLPHipError, match="fused"):
                ix.search(None, RWALoss(20, "equal"), _videos(2), k=3, ground=True)
        ix = search.CaptionIndex(8, 20, torch.bfloat16, device="cpu")
        ix.n = 8
        with pytest.raises(ValueError, match="divisor"):
            ix.ground(None, RWALoss(20, "equal"), _videos(2), ids, frames=4)
        with pytest.raises(DemoVLPHipError):
            ix.ground(None, RWALoss(20, "equal"), _videos(2), ids, frames=2)            # well-formed, but on the host

    def test_wrappers_refuse_host_tensors_wrong_dtypes_and_shapes(self):
        W, G, cap = 20, 30, 2
        buf = torch.zeros(ops.xattn_caption_index_bytes(cap, W), dtype=torch.uint8)
        Q = torch.zeros(cap, W, 256, dtype=torch.bfloat16)
        with pytest.raises(DemoVLPHipError, match="bf16"):
            ops.xattn_caption_index_add(buf, cap, W, 0, Q.float())
        with pytest.raises(DemoVLPHipError, match="expected Q"):
            ops.xattn_caption_index_add(buf, cap, W, 0, torch.zeros(cap, W + 1, 256, dtype=torch.bfloat16))
        with pytest.raises(DemoVLPHipError, match="smaller"):
            ops.xattn_caption_index_add(buf[:-1], cap, W, 0, Q)
        with pytest.raises(DemoVLPHipError, match="contiguous"):
            ops.xattn_caption_index_add(buf, cap, W, 0, torch.zeros(cap, 256, W, dtype=torch.bfloat16).transpose(1, 2))
        with pytest.raises(DemoVLPHipError, match="MI355X"):
            ops.xattn_caption_index_add(buf, cap, W, 0, Q)                 # well-formed, but on the host
        C, mi, mc = torch.zeros(3, G, 256, dtype=torch.bfloat16), torch.zeros(3, G), torch.zeros(cap, W)
        cand = torch.zeros(3, 2, dtype=torch.int32)
        for fn in (ops.xattn_caption_index_pairs_fwd, ops.xattn_caption_index_pairs_ground):
            with pytest.raises(DemoVLPHipError, match="bf16"):
                fn(buf, cap, W, mc, C.float(), mi, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="int32"):
                fn(buf, cap, W, mc, C, mi, cand.long(), 20.0, True)
            with pytest.raises(DemoVLPHipError, match="int32"):
                fn(buf, cap, W, mc, C, mi, cand[:2], 20.0, True)
            with pytest.raises(DemoVLPHipError, match="masks"):
                fn(buf, cap, W, mc[:1], C, mi, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="masks"):
                fn(buf, cap, W, mc, C, mi[:, :-1], cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="smaller"):
                fn(buf[:-1], cap, W, mc, C, mi, cand, 20.0, True)
            with pytest.raises(DemoVLPHipError, match="contiguous"):
                fn(buf, cap, W, mc, C, mi, torch.zeros(2, 3, dtype=torch.int32).t(), 20.0, True)
            with pytest.raises(DemoVLPHipError, match="MI355X"):
                fn(buf, cap, W, mc, C, mi, cand, 20.0, True)               # well-formed, but on the host
        with pytest.raises(DemoVLPHipError, match="divisor"):
            ops.xattn_caption_index_pairs_ground(buf, cap, W, mc, C, mi, cand, 20.0, True, frames=4)

    def test_the_autograd_function_exists_beside_its_twin(self):
        from demovlp_amd import functional as Fn
        assert issubclass(Fn.XattnCaptionIndexPairsFn, torch.autograd.Function)
        with pytest.raises(DemoVLPHipError, match="forward only"):
            Fn.XattnCaptionIndexPairsFn.backward(None, None)
