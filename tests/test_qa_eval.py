"""Video question answering, host side: ``metric.evaluate_qa`` against golden G16 and hand cases, the
synthetic QA set, the cross-rank merge of question ids and logits on a gloo world of 2, the ``impl`` switch of ``BUTDQAHead`` /
``CrossEntropy`` (the default is today's code bit for bit; the HIP path refuses CPU tensors) and the error codes of the new C entries (no GPU
needed for any of them)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from demovlp_amd import DemoVLPHipError, metric, synthetic as syn
from demovlp_amd.loss import CrossEntropy
from demovlp_amd.video_qa_model import BUTDQAHead

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16_qa_finetune.npz")


@pytest.fixture(scope="module")
def g16():
    return dict(np.load(G16))


@pytest.fixture(scope="module")
def sd():
    return syn.retrieval_state_dict(8, 30)


class TestEvaluateQaMetric:
    def test_reference_dict_on_g16_predictions(self, g16, sd):
        val = syn.qa_questions(sd, int(g16["F"]), int(g16["R"]), int(g16["val_first"]), int(g16["val_n"]), int(g16["num_label"]))
        assert np.array_equal(val["label"], g16["val_label"])
        results = [dict(question_id=int(q), answer=int(a)) for q, a in zip(val["question_id"], g16["val_preds"])]
        res = metric.evaluate_qa(results, val["label2ans"], val["qid2data"])
        assert set(res) == {"overall_acc", "ratios"} | {f"{t}_acc" for t in metric.QA_ANSWER_TYPES}
        assert res["overall_acc"] == float(g16["overall_acc"])
        for i, t in enumerate(metric.QA_ANSWER_TYPES):
            assert res[f"{t}_acc"] == g16["type_acc"][i], t
            assert res["ratios"][f"{t}_ratio"] == [float(g16["type_ratio"][i]), int(g16["type_count"][i])], t

    def test_hand_cases(self):
        label2ans = ["cat", "dog", "two"]
        qid2data = {1: {"answer": "cat", "answer_type": "what"}, 2: {"answer": "dog", "answer_type": "what"}, 3: {"answer": "two", "answer_type": "number"}}
        res = metric.evaluate_qa([dict(question_id=1, answer=0), dict(question_id=2, answer=0), dict(question_id=3, answer=2)], label2ans, qid2data)
        assert res["overall_acc"] == 2 / 3 and res["what_acc"] == 0.5 and res["number_acc"] == 1.0
        assert res["who_acc"] == 0 and res["ratios"]["who_ratio"] == [0.0, 0]                  # a type without questions scores 0
        assert res["ratios"]["what_ratio"] == [2 / 3, 2] and res["ratios"]["number_ratio"] == [1 / 3, 1]
        # a repeated question id: the later entry wins, and the question counts once
        res = metric.evaluate_qa([dict(question_id=1, answer=1), dict(question_id=3, answer=2), dict(question_id=1, answer=0)], label2ans, qid2data)
        assert res["overall_acc"] == 1.0 and res["ratios"]["what_ratio"] == [0.5, 1]


class TestQaQuestions:
    def test_deterministic(self, sd):
        a, b = syn.qa_questions(sd, 8, 30, 16, 12, 50), syn.qa_questions(sd, 8, 30, 16, 12, 50)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k

    def test_well_formed(self, sd):
        first, n, NL = 40, 27, 50
        qa = syn.qa_questions(sd, 8, 30, first, n, NL)
        assert qa["object"].shape == (n, 8, 30, 2054) and qa["object_mask"].shape == (n, 8, 30)
        assert qa["input_ids"].shape == (n, 100) and qa["attention_mask"].shape == (n, 100) and qa["input_ids"].dtype == np.int64
        assert qa["label"].dtype == np.int64 and qa["label"].min() >= 0 and qa["label"].max() < NL
        assert np.array_equal(qa["question_id"], np.arange(first, first + n))
        assert qa["answer_type"] == [metric.QA_ANSWER_TYPES[(first + i) % 9] for i in range(n)]
        assert len(qa["label2ans"]) == NL and len(set(qa["label2ans"])) == NL
        obj, mask, cap_ids, _ = syn.retrieval_batch(sd, 8, 30, first, n)
        assert np.array_equal(qa["object"], obj) and np.array_equal(qa["object_mask"], mask)
        for i in range(n):
            m = syn.QA_WORDS + 2
            assert qa["input_ids"][i, 0] == 101 and qa["input_ids"][i, m - 1] == 102 and qa["attention_mask"][i].sum() == m
            body = qa["input_ids"][i, 1:m - 1]
            assert np.isin(body, cap_ids[i]).sum() >= syn.QA_WORDS - 1                       # the clip's own words, one replaced by the query word
            d = qa["qid2data"][first + i]
            assert d["answer"] == qa["label2ans"][qa["label"][i]] and d["answer_type"] == qa["answer_type"][i]

    def test_answer_depends_on_clip_and_question(self, sd):
        qa = syn.qa_questions(sd, 8, 30, 0, 64, 50)
        pool = set(np.random.default_rng(606060).choice(np.arange(1000, syn.VOCAB), syn.QA_QUERY_POOL, replace=False).tolist())
        query = np.array([[w for w in row if w in pool][0] for row in qa["input_ids"]])
        group = np.arange(64) // syn.RETR_GROUP
        same_query = [(i, j) for i in range(64) for j in range(i) if query[i] == query[j] and group[i] != group[j]]
        same_group = [(i, j) for i in range(64) for j in range(i) if query[i] != query[j] and group[i] == group[j]]
        assert same_query and same_group
        assert all(qa["label"][i] != qa["label"][j] for i, j in same_query)                  # the query word alone does not fix the answer
        assert all(qa["label"][i] != qa["label"][j] for i, j in same_group)                  # nor does the clip alone

    def test_batches_layout(self, sd):
        qa = syn.qa_questions(sd, 8, 30, 0, 7, 50)
        bs = list(syn.qa_batches(qa, 3))
        assert [len(b["label"]) for b in bs] == [3, 3, 1]
        assert bs[1]["text"]["input_ids"].shape == (3, 100) and bs[1]["object"].shape == (3, 8, 30, 2054) and bs[2]["question_id"].tolist() == [6]

    def test_golden_g16_was_made_from_this_generator(self, g16, sd):
        tr = syn.qa_questions(sd, int(g16["F"]), int(g16["R"]), 0, int(g16["steps"]) * int(g16["B"]), int(g16["num_label"]))
        assert np.array_equal(tr["label"], g16["train_label"])
        thr = 10 * 1e-4 * float(np.abs(g16["val_logits"]).max())
        assert int((g16["val_margin"] <= thr).sum()) <= 3                                     # the cap of tests/test_gpu_qa.py is met by the fixture


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _merge_worker(rank, world, port, qids, logits, q):
    from demovlp_amd.trainer import gather_qa_results
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        half = len(qids) // 2 + 1                    # uneven halves, as a DistributedSampler's last batch can be
        sl = slice(0, half) if rank == 0 else slice(half, None)
        a, b = gather_qa_results(torch.from_numpy(qids[sl]), torch.from_numpy(logits[sl]))
        q.put((rank, a.numpy(), b.numpy()))
    finally:
        dist.destroy_process_group()


class TestMergeAcrossRanks:
    def test_gloo_world2_merge_equals_single_process(self):
        from demovlp_amd.trainer import gather_qa_results
        rng = np.random.default_rng(3)
        qids = rng.permutation(1000)[:11].astype(np.int64)
        logits = rng.standard_normal((11, 50)).astype(np.float32)
        a, b = gather_qa_results(torch.from_numpy(qids), torch.from_numpy(logits))
        assert np.array_equal(a.numpy(), qids) and np.array_equal(b.numpy(), logits)
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_merge_worker, args=(r, 2, port, qids, logits, q)) for r in range(2)]
        for p in procs:
            p.start()
        got = [q.get(timeout=120) for _ in range(2)]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        for _, a2, b2 in got:
            assert np.array_equal(a2, qids) and np.array_equal(b2, logits)


def _literal_stock_head(head, q, v, mask):
    """BUTDQAHead.forward as it stood before the ``impl`` switch, written out on the module's own sub-modules."""
    a = head.v_att
    logits = a.linear(a.drop(a.v_proj(v) * a.q_proj(q).unsqueeze(1)))
    logits = logits * mask.unsqueeze(-1)
    att = torch.softmax(logits, 1)
    c = head.classifier
    return c.main(c.q_net(q) * c.v_net((att * v).sum(1)))


class TestImplSwitch:
    def test_stock_is_todays_head(self):
        torch.manual_seed(0)
        head = BUTDQAHead(256, 256, 256, 50).eval()
        assert head.impl == "stock" and set(head.state_dict()) == {k[5:] for k in syn.qa_head_schema(50)}
        assert set(BUTDQAHead(256, 256, 256, 50, impl="hip").state_dict()) == set(head.state_dict())
        q, v, mask = torch.randn(3, 256), torch.randn(3, 17, 256), (torch.rand(3, 17) > 0.3).float()
        assert torch.equal(head(q, v, mask), _literal_stock_head(head, q, v, mask))
        head.train()
        torch.manual_seed(5)
        a = head(q, v, mask)
        torch.manual_seed(5)
        assert torch.equal(a, _literal_stock_head(head, q, v, mask))                          # train mode: the same dropout draw

    def test_hip_refuses_cpu_tensors_and_bad_impl_raises(self):
        head = BUTDQAHead(256, 256, 256, 50, impl="hip")
        with pytest.raises(DemoVLPHipError):
            head(torch.zeros(2, 256), torch.zeros(2, 5, 256), torch.ones(2, 5))
        with pytest.raises(ValueError):
            BUTDQAHead(256, 256, 256, 50, impl="triton")
        with pytest.raises(ValueError):
            CrossEntropy(impl="fast")
        with pytest.raises(DemoVLPHipError):
            CrossEntropy(impl="hip")(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
        x, y = torch.randn(4, 7), torch.tensor([1, 0, 6, 3])
        assert torch.equal(CrossEntropy()(x, y), torch.nn.CrossEntropyLoss()(x, y))


class TestNewEntriesReportBadArguments:
    """Error codes without a launch (and without a GPU), as tests/test_abi.py::test_bad_arguments_are_reported_not_launched."""

    @pytest.fixture(scope="class")
    def lib(self):
        from demovlp_amd import _lib
        _lib.load()
        return _lib

    def test_null_pointers_bad_sizes_bad_dtype(self, lib):
        bad = [("dvlp_wn_fold_fwd", (0, None, None, None, None, None, None, None)),
               ("dvlp_wn_fold_fwd", (9, None, None, None, None, None, None, None)),
               ("dvlp_wn_fold_bwd", (5, None, None, None, None, None, None, None, None)),
               ("dvlp_token_max_fwd", (7, 4, 100, 256, None, None, None, None)),
               ("dvlp_token_max_fwd", (lib.F32, 4, 100, 256, None, None, None, None)),
               ("dvlp_token_max_bwd", (lib.BF16, 0, 100, 256, None, None, None, None)),
               ("dvlp_qa_attend_fwd", (5, 4, 240, None, 240 * 256, 256) + (None,) * 9 + (240, 0.0, None, 0, None, None, None, None, None)),
               ("dvlp_qa_attend_fwd", (lib.BF16, 4, 240, None, 240 * 256, 256) + (None,) * 9 + (240, 0.0, None, 0, None, None, None, None, None)),
               ("dvlp_qa_attend_bwd", (lib.F32, 4, 0, None, 0, 256) + (None,) * 7 + (0, 0.0, None, 0) + (None,) * 15),
               ("dvlp_softmax_xent", (4, 0, None, None, None, None, None, None, None)),
               ("dvlp_softmax_xent", (4, 50, None, None, None, None, None, None, None))]
        for name, args in bad:
            with pytest.raises(DemoVLPHipError):
                lib.call(name, *args)

    def test_size_helpers_on_host(self, lib):
        assert lib.call("dvlp_qa_attend_workspace_floats", 64, 240) == 64 * 240 + 64 + 2 * 64 * 4 * 256 + 64 * 256
        assert lib.call("dvlp_qa_attend_workspace_floats", 0, 240) == 0
        assert lib.call("dvlp_qa_attend_fused", lib.BF16, 240) == 1 and lib.call("dvlp_qa_attend_fused", lib.BF16, 288) == 1
        assert lib.call("dvlp_qa_attend_fused", lib.BF16, 289) == 0 and lib.call("dvlp_qa_attend_fused", lib.F32, 240) == 0
