"""Multiple-choice evaluation, host side (b): the reference's ``evaluate_mc`` metric against
golden G15, the synthetic multiple-choice set, the cross-rank merge of predictions on a gloo world of 2, the host-side argument checks of
``RWALoss.get_sim_pairs`` and the error codes / workspace helper of the pair-list C entries (no GPU needed for any of them)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from demovlp_amd import DemoVLPHipError, metric, synthetic as syn
from demovlp_amd.loss import RWALoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G15 = os.path.join(ROOT, "tests", "golden", "g15_mc.npz")


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(G15))


@pytest.fixture(scope="module")
def sd():
    return syn.retrieval_state_dict(8, 30)


class TestEvaluateMcMetric:
    def test_reference_string_on_g15_predictions(self, g15):
        pred = {int(i): int(p) for i, p in zip(g15["mc_ids"], g15["preds"])}
        gt = {int(i): int(a) for i, a in zip(g15["mc_ids"], g15["answers"])}
        assert metric.evaluate_mc(pred, gt) == {"mc_accuracy": str(g15["mc_accuracy"])}

    def test_scores_the_predicted_ids_and_formats_two_decimals(self):
        gt = {"a": 0, "b": 1, "c": 2, "d": 3}
        assert metric.evaluate_mc({"a": 0, "b": 1, "c": 0}, gt) == {"mc_accuracy": "66.67"}       # shared_ids = pred_ids ('d' unused)
        assert metric.evaluate_mc({"d": 3}, gt) == {"mc_accuracy": "100.00"}
        assert metric.evaluate_mc({"a": 1}, gt) == {"mc_accuracy": "0.00"}


class TestMcQuestions:
    def test_deterministic(self, sd):
        a, b = syn.mc_questions(sd, 8, 30, 16, 12), syn.mc_questions(sd, 8, 30, 16, 12)
        for k in a:
            assert np.array_equal(a[k], b[k]), k

    def test_well_formed(self, sd):
        first, n, K = 40, 24, 5
        mc = syn.mc_questions(sd, 8, 30, first, n, K)
        assert mc["object"].shape == (n, 8, 30, 2054) and mc["object_mask"].shape == (n, 8, 30)
        assert mc["input_ids"].shape == (n * K, 100) and mc["attention_mask"].shape == (n * K, 100)
        assert np.array_equal(mc["mc_ids"], np.arange(first, first + n))
        assert np.array_equal(mc["answers"], np.arange(n) % K)                         # the answer slot rotates
        obj, mask, _, _ = syn.retrieval_batch(sd, 8, 30, first, n)
        assert np.array_equal(mc["object"][mc["object_mask"] > 0], obj[mc["object_mask"] > 0]) and not mc["object"][mc["object_mask"] == 0].any()
        assert np.array_equal(mc["object_mask"].reshape(n, -1).sum(1), np.full(n, syn.MC_VISIBLE)) and (mc["object_mask"] <= mask).all()
        for q in range(n):
            v, opts = first + q, mc["options"][q]
            assert opts[mc["answers"][q]] == v
            d = np.delete(opts, mc["answers"][q])
            assert len(set(d.tolist())) == K - 1 and v not in d
            same = (d // syn.RETR_GROUP == v // syn.RETR_GROUP).sum()
            assert same == syn.MC_SAME and 0 < syn.MC_SAME < K - 1                   # hard negatives from the group, and others
            ids, att = syn.retrieval_captions(int(opts[0]), 1)
            assert np.array_equal(mc["input_ids"][q * K], ids[0]) and np.array_equal(mc["attention_mask"][q * K], att[0])

    def test_golden_g15_was_made_from_this_generator(self, g15):
        mc_opts = syn.mc_questions(syn.retrieval_state_dict(int(g15["F"]), int(g15["R"])), int(g15["F"]), int(g15["R"]), int(g15["first"]),
                                   int(g15["n"]), int(g15["K"]))
        assert int(g15["mc_same"]) == syn.MC_SAME and int(g15["mc_visible"]) == syn.MC_VISIBLE
        assert np.array_equal(mc_opts["options"], g15["options"]) and np.array_equal(mc_opts["answers"], g15["answers"])

    def test_reference_accuracy_is_far_from_chance_and_from_perfect(self, g15):
        acc = float(str(g15["mc_accuracy"]))
        assert 35.0 <= acc <= 90.0, acc

    def test_batches_layout(self, sd):
        mc = syn.mc_questions(sd, 8, 30, 0, 7, 5)
        bs = list(syn.mc_batches(mc, 3))
        assert [len(b["mc_id"]) for b in bs] == [3, 3, 1]
        assert bs[1]["text"]["input_ids"].shape == (15, 100) and bs[1]["object"].shape == (3, 8, 30, 2054)
        assert torch.equal(bs[2]["text"]["attention_mask"], torch.from_numpy(mc["attention_mask"][30:35]))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _merge_worker(rank, world, port, ids, preds, scores, q):
    from demovlp_amd.trainer import gather_mc_results
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        half = len(ids) // 2 + 1                    # uneven halves, as a DistributedSampler's last batch can be
        sl = slice(0, half) if rank == 0 else slice(half, None)
        merged, sc = gather_mc_results(ids[sl], preds[sl], scores[sl])
        q.put((rank, merged, sc))
    finally:
        dist.destroy_process_group()


class TestMergeAcrossRanks:
    def test_gloo_world2_merge_equals_single_process(self):
        from demovlp_amd.trainer import gather_mc_results
        rng = np.random.default_rng(3)
        ids = [int(x) for x in rng.permutation(1000)[:11]]
        preds = [int(x) for x in rng.integers(0, 5, 11)]
        scores = rng.standard_normal((11, 5)).astype(np.float32)
        single, sc1 = gather_mc_results(ids, preds, scores)
        assert single == dict(zip(ids, preds)) and np.array_equal(sc1, scores)
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_merge_worker, args=(r, 2, port, ids, preds, scores, q)) for r in range(2)]
        for p in procs:
            p.start()
        res = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
        for rank, merged, sc in res:
            assert merged == single and list(merged) == ids, rank              # every rank gets the whole result, in rank order
            assert np.array_equal(sc, scores), rank


class TestGetSimPairsHostChecks:
    def setup_method(self):
        self.loss = RWALoss(20, "equal")
        self.im = torch.zeros(3, 6, 256)
        self.s = torch.zeros(7, 4, 256)
        self.im_m = torch.zeros(3, 6)
        self.s_m = torch.zeros(7, 4)

    def call(self, cand, im=None):
        return self.loss.get_sim_pairs(self.im if im is None else im, self.s, self.im_m, None, self.s_m, cand=cand)

    def test_index_out_of_range(self):
        with pytest.raises(ValueError):
            self.call(np.array([[0, 7], [1, 2], [3, 4]]))
        with pytest.raises(ValueError):
            self.call(torch.tensor([[0, 1], [-1, 2], [3, 4]]))

    def test_dtype_and_shape(self):
        with pytest.raises(ValueError):
            self.call(np.zeros((3, 2), np.float32))
        with pytest.raises(ValueError):
            self.call(torch.zeros(3, 2, dtype=torch.float64))
        with pytest.raises(ValueError):
            self.call(np.zeros((2, 2), np.int64))                           # one row per image
        with pytest.raises(ValueError):
            self.call(None)                                                  # 7 captions are no K per image for 3 images

    def test_grad_enabled_on_inputs_that_require_grad(self):
        with pytest.raises(DemoVLPHipError):
            self.call(np.zeros((3, 2), np.int64), im=self.im.clone().requires_grad_(True))

    def test_valid_arguments_reach_the_device_check(self):
        with pytest.raises(DemoVLPHipError):                                 # no CPU fallback
            self.call(np.array([[0, 6], [6, 0], [2, 2]], np.int32))


class TestPairsCAbi:
    @pytest.fixture(scope="class")
    def lib(self):
        import __graft_entry__
        __graft_entry__.build()
        from demovlp_amd import _lib
        return _lib

    def test_workspace_helper_runs_on_host(self, lib):
        fused = lib.call("dvlp_xattn_pairs_workspace_bytes", lib.BF16, 64, 320, 5, 240, 99)
        assert fused == lib.call("dvlp_xattn_workspace_bytes", lib.BF16, 64, 320, 240, 99, 0)        # the fused kernel's prep buffers
        f32 = lib.call("dvlp_xattn_pairs_workspace_bytes", lib.F32, 64, 320, 5, 240, 99)
        assert f32 > 5 * 99 * 256 * 4 and f32 < lib.call("dvlp_xattn_workspace_bytes", lib.F32, 2, 5, 240, 99, 0) + (1 << 20)
        long = lib.call("dvlp_xattn_pairs_workspace_bytes", lib.F32, 4, 20, 5, 1152, 99)
        assert long > 0
        assert lib.call("dvlp_xattn_pairs_workspace_bytes", 7, 64, 320, 5, 240, 99) == -1
        assert lib.call("dvlp_xattn_pairs_workspace_bytes", lib.BF16, 64, 320, 0, 240, 99) == -2
        assert lib.call("dvlp_xattn_pairs_workspace_bytes", lib.BF16, 64, 320, 5, 240, 129) == -2

    def test_bad_shape_or_dtype_returns_an_error_code(self, lib):
        import ctypes
        fn = lib.load().dvlp_xattn_pairs_fwd
        x = ctypes.c_void_p(256)                      # never dereferenced: every case below fails its argument check first
        args = lambda dtype, Bi, Bj, K, G, W, d, cand, ws: (dtype, Bi, Bj, K, G, W, d, x, x, x, x, cand, 20.0, 1, x, ws, None)
        assert fn(*args(7, 2, 10, 5, 240, 99, 256, None, x)) == -1                 # dtype
        assert fn(*args(lib.BF16, 2, 10, 5, 240, 99, 128, None, x)) == -2          # d != 256
        assert fn(*args(lib.BF16, 2, 10, 0, 240, 99, 256, None, x)) == -2          # K = 0
        assert fn(*args(lib.BF16, 0, 10, 5, 240, 99, 256, None, x)) == -2          # Bi = 0
        assert fn(*args(lib.BF16, 2, 9, 5, 240, 99, 256, None, x)) == -2           # cand = NULL needs Bj >= Bi K
        assert fn(*args(lib.F32, 2, 10, 5, 240, 200, 256, None, x)) == -2          # W beyond every path
        assert fn(*args(lib.BF16, 2, 10, 5, 240, 99, 256, None, None)) == -2       # no workspace
        with pytest.raises(lib.DemoVLPHipError):
            lib.call("dvlp_xattn_pairs_fwd", 7, 2, 10, 5, 240, 99, 256, x, x, x, x, None, 20.0, 1, x, x, None)
