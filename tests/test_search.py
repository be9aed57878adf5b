"""Text-to-video search, host side: the error codes and size helpers of the six C entries behind it (row top-k, resident video index,
query-major pair list), the argument checks of ``search.VideoIndex`` and ``search.two_stage_sims`` (no GPU needed for any of them)."""
import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, metric
from demovlp_amd import search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null pointer value for argument checks that return before anything is launched


class TestEntryArgumentChecks:
    def test_topk_rejects_bad_shapes_and_null_pointers(self):
        ok = dict(M=2, N=100, x=ONE, ld=100, K=10, base=0, val=ONE, idx=ONE, merge=0, ws=ONE)
        bad = [dict(K=0), dict(K=1025), dict(M=0), dict(N=0), dict(N=1 << 31), dict(ld=99), dict(base=-1), dict(base=(1 << 31) - 50),
               dict(merge=2), dict(x=None), dict(val=None), dict(idx=None), dict(ws=None), dict(x=ONE + 2)]
        for b in bad:
            a = {**ok, **b}
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_topk_rows", a["M"], a["N"], a["x"], a["ld"], a["K"], a["base"], a["val"], a["idx"], a["merge"], a["ws"], None)

    def test_topk_workspace_helper(self):
        w = lambda M, N, K: _lib.call("dvlp_topk_workspace_bytes", M, N, K)
        assert w(1, 100, 0) < 0 and w(1, 100, 1025) < 0 and w(0, 100, 10) < 0 and w(1, 0, 10) < 0 and w(1, 1 << 31, 10) < 0
        assert w(1000, 1000, 10) == 1000 * 10 * 8                          # enough rows: one list per row
        assert w(1, 1 << 20, 100) == 256 * 100 * 8                         # one row of 4 MB: 256 column segments
        assert w(1, 1 << 20, 1024) == 32 * 1024 * 8                        # the merge pass bounds segments x K
        assert w(1, 1000, 10) == 10 * 8                                    # short rows are not split
        assert w(2000, 1 << 20, 100) == 2 * w(1000, 1 << 20, 100)

    def test_index_size_helpers_scale_as_stated(self):
        ib = lambda c, G: _lib.call("dvlp_xattn_index_bytes", c, G)
        qb = lambda Bj, W: _lib.call("dvlp_xattn_index_query_workspace_bytes", Bj, W)
        per = 288 * 256 * 2 * 2 + 288 * 4                                 # both orientations in bf16 + the norms
        assert ib(2, 288) == 2 * per and ib(1000, 288) == 1000 * per and ib(100000, 288) == 100000 * per      # linear in the capacity
        assert 290e3 < per < 300e3
        assert ib(2, 240) == 2 * (240 * 512 + 256 * 256 * 2) + 2048      # transposed side padded to 32 regions; sections rounded up to 256 bytes
        assert ib(0, 288) < 0 and ib(4, 0) < 0 and ib(4, 289) == _lib.call("dvlp_xattn_index_bytes", 4, 1152) < 0
        assert qb(8, 99) == 8 * (112 * 512 + 256 * 128 * 2) + 3328         # independent of any capacity: captions only
        assert qb(16, 99) == 16 * (112 * 512 + 256 * 128 * 2) + 6400
        assert qb(0, 99) < 0 and qb(4, 0) < 0 and qb(4, 113) < 0

    def test_index_add_rejects(self):
        for args in [(4, 288, 0, 5, ONE, ONE), (4, 288, -1, 1, ONE, ONE), (4, 288, 3, 2, ONE, ONE), (4, 288, 0, 0, ONE, ONE), (0, 288, 0, 1, ONE, ONE),
                     (4, 289, 0, 1, ONE, ONE), (4, 288, 0, 1, None, ONE), (4, 288, 0, 1, ONE, None)]:
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_index_add", *args, None)

    def test_index_pairs_rejects(self):
        ok = dict(cap=4, G=240, index=ONE, mimg=ONE, Bj=2, W=99, d=256, Q=ONE, mcap=ONE, K=3, cand=ONE, scores=ONE, ws=ONE)
        bad = [dict(d=128), dict(cap=0), dict(G=0), dict(G=289), dict(W=113), dict(W=0), dict(Bj=0), dict(Bj=65536), dict(K=0), dict(index=None),
               dict(mimg=None), dict(Q=None), dict(mcap=None), dict(cand=None), dict(scores=None), dict(ws=None)]
        for b in bad:
            a = {**ok, **b}
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_xattn_index_pairs_fwd", a["cap"], a["G"], a["index"], a["mimg"], a["Bj"], a["W"], a["d"], a["Q"], a["mcap"], a["K"],
                          a["cand"], 20.0, 1, a["scores"], a["ws"], None)


def _out(n, G, dtype=torch.bfloat16):
    return dict(global_object_embeddings=torch.zeros(n, 256, dtype=dtype), local_object_embeddings=torch.zeros(n, G, 256, dtype=dtype),
                object_mask=torch.zeros(n, G))


class TestVideoIndexHostChecks:
    def test_route_follows_dtype_and_region_count(self):
        assert search.VideoIndex(10, 240, torch.bfloat16).fused and search.VideoIndex(10, 288, "bfloat16").fused
        assert not search.VideoIndex(10, 240, torch.float32).fused and not search.VideoIndex(10, 1152, torch.bfloat16).fused
        with pytest.raises(ValueError):
            search.VideoIndex(0, 240)
        with pytest.raises(ValueError):
            search.VideoIndex(4, 240, torch.float16)

    def test_add_checks_then_needs_the_device(self):
        ix = search.VideoIndex(4, 30, torch.bfloat16, device="cpu")
        assert len(ix) == 0
        with pytest.raises(ValueError, match="G = 30"):
            ix.add(_out(2, 31))                                            # wrong G
        with pytest.raises(ValueError, match="capacity"):
            ix.add(_out(5, 30))                                            # past the capacity
        with pytest.raises(ValueError, match="bfloat16"):
            ix.add(_out(2, 30, torch.float32))
        with pytest.raises(DemoVLPHipError):
            ix.add(_out(2, 30))                                            # well-formed, but on the host
        assert len(ix) == 0

    def test_search_checks_then_needs_the_device(self):
        ix = search.VideoIndex(64, 30, torch.bfloat16, device="cpu")
        text = dict(input_ids=torch.zeros(2, 100, dtype=torch.long), attention_mask=torch.ones(2, 100, dtype=torch.long))
        with pytest.raises(ValueError, match="empty"):
            ix.search(None, RWALoss(20, "equal"), text)
        ix.n = 50                                                          # (as if filled: the checks below are host logic)
        with pytest.raises(ValueError, match="shortlist"):
            ix.search(None, RWALoss(20, "equal"), text, k=11, shortlist=10)
        with pytest.raises(ValueError, match="shortlist"):
            ix.search(None, RWALoss(20, "equal"), text, k=51, shortlist=None)
        with pytest.raises(ValueError):
            ix.search(None, RWALoss(20, "equal"), text, k=0)
        with pytest.raises(ValueError):
            ix.search(None, RWALoss(20, "equal"), text, chunk=0)
        with pytest.raises(DemoVLPHipError):
            ix.search(None, RWALoss(20, "equal"), text, k=10, shortlist=20)

    def test_wrappers_refuse_host_tensors_and_wrong_dtypes(self):
        from demovlp_amd import ops
        with pytest.raises(DemoVLPHipError):
            ops.topk_rows(torch.zeros(3, 50), 5)
        with pytest.raises(DemoVLPHipError):
            ops.topk_rows(torch.zeros(3, 50, dtype=torch.bfloat16), 5)
        with pytest.raises(DemoVLPHipError):
            ops.topk_rows(torch.zeros(3, 50), 5, merge=True)
        with pytest.raises(DemoVLPHipError):
            ops.topk_rows(torch.zeros(3, 50), 2000)
        with pytest.raises(DemoVLPHipError):
            ops.xattn_index_add(torch.zeros(ops.xattn_index_bytes(2, 30), dtype=torch.uint8), 2, 30, 0, torch.zeros(2, 30, 256))
        with pytest.raises(DemoVLPHipError):
            ops.xattn_index_add(torch.zeros(ops.xattn_index_bytes(2, 30), dtype=torch.uint8), 2, 30, 0, torch.zeros(2, 30, 256, dtype=torch.bfloat16))


class TestTwoStageSims:
    def test_shortlisted_entries_carry_scores_and_the_rest_keep_global_order_behind_them(self):
        g = np.array([[0.9, 0.1, 0.5, 0.3, -0.2], [0.0, 0.8, 0.7, -0.9, 0.6]])
        ids = np.array([[0, 2], [2, 1]])
        scores = np.array([[-3.0, 1.5], [0.25, 0.125]])
        s = search.two_stage_sims(g, ids, scores)
        assert s.shape == g.shape
        assert s[0, 0] == -3.0 and s[0, 2] == 1.5 and s[1, 2] == 0.25 and s[1, 1] == 0.125
        for q in range(2):
            rest = [v for v in range(5) if v not in ids[q]]
            assert s[q, rest].max() < scores.min()                         # strictly behind every shortlisted video
            assert list(np.argsort(-s[q, rest])) == list(np.argsort(-g[q, rest]))      # in global order
        assert list(np.argsort(-s[0], kind="stable")) == [2, 0, 3, 1, 4]

    def test_fillers_are_skipped_and_shapes_checked(self):
        g = np.zeros((2, 3))
        s = search.two_stage_sims(g, np.array([[1, -1], [-1, -1]]), np.array([[2.0, -np.inf], [-np.inf, -np.inf]]))
        assert s[0, 1] == 2.0 and np.isfinite(s).all() and (np.delete(s.ravel(), 1) < 0).all()
        with pytest.raises(ValueError):
            search.two_stage_sims(g, np.zeros((2, 2), int), np.zeros((2, 3)))
        with pytest.raises(ValueError):
            search.two_stage_sims(g, np.full((2, 1), 3), np.zeros((2, 1)))

    def test_full_shortlist_gives_the_metrics_of_the_plain_matrix(self):
        rng = np.random.default_rng(0)
        n = 40
        full = rng.standard_normal((n, n)) + 2.0 * np.eye(n)
        g = rng.standard_normal((n, n))
        ids = np.stack([rng.permutation(n) for _ in range(n)])
        scores = np.take_along_axis(full, ids, 1)
        assert metric.t2v_metrics(search.two_stage_sims(g, ids, scores)) == metric.t2v_metrics(full)
        # a partial shortlist that misses the ground truth ranks it behind the shortlist, by its global position among the rest
        ids8 = np.stack([(np.arange(8) + q + 1) % n for q in range(n)])
        m = metric.t2v_metrics(search.two_stage_sims(g, ids8, np.take_along_axis(full, ids8, 1)))
        assert m["R1"] == 0.0 and m["R5"] == 0.0 and m["MedR"] > 8
