"""Text-to-video search on a real MI355X: the row top-k kernel against numpy's stable argsort, the resident-index pair kernel against the
fused full grid (bit for bit), and ``search.VideoIndex.search`` against ``trainer.evaluate`` on the retrieval set with signal (golden G11's
inputs), in the search orientation ``global_sims + local_sims.T``."""
import numpy as np
import pytest
import torch

from demovlp_amd import ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss, RWALoss
from demovlp_amd.model import ObjectRelation
from demovlp_amd.trainer import evaluate
from helpers import load_golden
from oracle import restatement as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"

# fp32 rounding of a 256-term dot product of unit vectors summed in another order: 256 x 2^-24 = 1.5e-5 (the local addend is bit-equal)
SCORE_TOL = 2e-5
RANK_GAP = 4e-5               # a rank is compared only where the score gaps to both neighbours exceed twice that


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. top-k against numpy
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows(M, N, variant, seed):
    """Row r is of kind (r + variant) % 4: random normal | rounded to 1/64 (mostly ties, and -0.0) | the same with +inf, -inf, NaN | constant."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, N), dtype=np.float32)
    for r in range(M):
        kind = (r + variant) % 4
        if kind in (1, 2):
            x[r] = np.round(x[r] * 64) / 64
        if kind == 2:
            pos = rng.integers(0, N, (3, max(1, N // 50)))
            x[r, pos[0]] = np.inf
            x[r, pos[1]] = -np.inf
            x[r, pos[2]] = np.nan
            x[r, pos[2][:1]] = np.float32(np.uint32(0xffc00123).view(np.float32)) if N > 1 else np.nan      # a NaN with sign and payload
        if kind == 3:
            x[r] = np.float32(0.375)
    return x


def _expect(x, order, K, base):
    M, N = x.shape
    k = min(K, N)
    idx = np.full((M, K), -1, np.int64)
    val = np.full((M, K), -np.inf, np.float32)
    idx[:, :k] = order[:, :k] + base
    val[:, :k] = np.take_along_axis(x, order[:, :k], 1)
    return val, idx


def _padded(x, pad):
    """x on the device inside a wider matrix (ld = N + pad, so rows start at every 4-byte phase); the padding holds +inf: a read past N shows"""
    M, N = x.shape
    buf = torch.full((M, N + pad), float("inf"), device=DEV, dtype=torch.float32)
    buf[:, :N] = torch.from_numpy(x).to(DEV)
    return buf


def _check(got, want, tag):
    val, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(idx, want[1]), (tag, "indices")
    assert np.array_equal(val.view(np.uint32), want[0].view(np.uint32)), (tag, "values, bit for bit")


class TestTopkAgainstNumpy:
    @pytest.mark.parametrize("M", [1, 3, 300])
    @pytest.mark.parametrize("N", ["1", "K-1", "1000", "65537", "2^20"])
    def test_stable_descending_order_values_and_indices(self, M, N):
        Ks = (1, 10, 100, 1024)
        sizes = {"1": [1], "K-1": [9, 99, 1023], "1000": [1000], "65537": [65537], "2^20": [1 << 20]}[N]      # (K - 1 = 0 is no matrix)
        for n in sizes:
            for variant in ([0] if M >= 4 else range(0, 4, M)):
                x = _rows(M, n, variant, 7 * M + n % 1000 + variant)
                order = np.argsort(-x, axis=1, kind="stable")
                xd = _padded(x, 3 if variant == 0 else 5)
                for K in (Ks if N != "K-1" else [n + 1]):
                    base = 0 if K == 10 else 12345
                    got = ops.topk_rows(xd, K, N=n, index_base=base)
                    _check(got, _expect(x, order, K, base), (M, n, K, variant))
                    again = ops.topk_rows(xd, K, N=n, index_base=base)
                    assert torch.equal(again[1], got[1]) and torch.equal(again[0].view(torch.int32), got[0].view(torch.int32))

    @pytest.mark.parametrize("M,N,chunks", [(3, 1000, (250, 300)), (1, 65537, (16384, 7777)), (300, 65537, (30000,)), (3, 1 << 20, (1 << 18, 300000))])
    @pytest.mark.parametrize("K", [10, 100, 1024])
    def test_chunked_calls_with_merge_equal_the_one_shot_call(self, M, N, chunks, K):
        x = _rows(M, N, 1, N + K)
        xd = _padded(x, 3)
        one = ops.topk_rows(xd, K, N=N)
        _check(one, _expect(x, np.argsort(-x, axis=1, kind="stable"), K, 0), (M, N, K))
        for chunk in chunks:
            out = (torch.empty((M, K), device=DEV), torch.empty((M, K), device=DEV, dtype=torch.int32))
            for c0 in range(0, N, chunk):
                ops.topk_rows(xd[:, c0:], K, N=min(chunk, N - c0), index_base=c0, out=out, merge=c0 > 0)
            assert torch.equal(out[1], one[1]), (chunk, "indices")
            assert torch.equal(out[0].view(torch.int32), one[0].view(torch.int32)), (chunk, "values")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. index pairs against the full grid, bf16
# ---------------------------------------------------------------------------------------------------------------------------------------
def _inputs(Bi, Bj, G, W, seed, dtype):
    rng = np.random.default_rng(seed)
    im = rng.standard_normal((Bi, G, 256), dtype=np.float32)
    cap = rng.standard_normal((Bj, W, 256), dtype=np.float32)
    n = min(G, W)
    for b in range(min(Bi, Bj)):
        cap[b, :n, :64] += 0.5 * im[b, :n, :64]
    m_img = np.zeros((Bi, G), np.float32)
    if G > 4:
        m_img[-1, G - 4:] = -100.0
    m_cap = np.full((Bj, W), -100.0, np.float32)
    for b in range(Bj):
        m_cap[b, : max(1, min(W, 3 + 5 * b))] = 0.0
    t = lambda a: torch.from_numpy(a).to(DEV)
    return t(im).to(dtype), t(cap).to(dtype), t(m_img), t(m_cap)


def _cand(Bj, Bi, K, seed):
    """video rows per caption [Bj, K], with a repeat and an unordered row"""
    c = np.random.default_rng(seed).integers(0, Bi, (Bj, K))
    if K > 1:
        c[0, -1] = c[0, 0]
        c[-1] = np.sort(c[-1])[::-1]
    return c.astype(np.int32)


def _filled(C, capacity, splits):
    G = C.shape[1]
    index = torch.zeros(ops.xattn_index_bytes(capacity, G), device=DEV, dtype=torch.uint8)
    r0 = 0
    for n in splits:
        ops.xattn_index_add(index, capacity, G, r0, C[r0:r0 + n].contiguous())
        r0 += n
    return index


class TestIndexPairsBf16BitEqualToFullGrid:
    @pytest.mark.parametrize("Bi,Bj,G,W,K", [(4, 9, 240, 99, 5), (3, 7, 288, 112, 4), (3, 5, 1, 99, 3), (3, 6, 240, 1, 5), (4, 6, 288, 99, 1),
                                             (1, 8, 240, 99, 6), (1, 1, 30, 99, 1)])
    @pytest.mark.parametrize("focal", ["equal", "prob"])
    def test_equals_get_sim_entries(self, Bi, Bj, G, W, K, focal):
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 11 + G + W, torch.bfloat16)
        cand = torch.from_numpy(_cand(Bj, Bi, K, G + K)).to(DEV)
        index = _filled(C, Bi, [Bi])
        with torch.no_grad():
            full = RWALoss(20, focal).get_sim(C, Q, mi, None, mc)                       # [Bi, Bj]
            got = ops.xattn_index_pairs_fwd(index, Bi, G, mi, Q, mc, cand, 20.0, focal == "equal")
        want = full[cand.long(), torch.arange(Bj, device=DEV)[:, None]]
        assert got.shape == (Bj, K) and got.dtype == torch.float32 and torch.isfinite(got).all()
        assert torch.equal(got, want), float((got - want).abs().max())

    def test_three_adds_are_byte_equal_to_one_and_spare_rows_stay_untouched(self):
        C, Q, mi, mc = _inputs(7, 3, 240, 99, 3, torch.bfloat16)
        one, three = _filled(C, 9, [7]), _filled(C, 9, [2, 4, 1])
        assert torch.equal(one, three)
        assert one.any() and not torch.equal(one, _filled(C.flip(0), 9, [7]))

    def test_out_of_range_candidate_scores_nan_and_leaves_the_others(self):
        Bi, Bj, G, W, K = 4, 5, 240, 99, 4
        C, Q, mi, mc = _inputs(Bi, Bj, G, W, 5, torch.bfloat16)
        index = _filled(C, 6, [Bi])                                                     # capacity 6: rows 4, 5 were never added
        mi6 = torch.cat([mi, torch.zeros(2, G, device=DEV)])
        cand = _cand(Bj, Bi, K, 1)
        good = ops.xattn_index_pairs_fwd(index, 6, G, mi6, Q, mc, torch.from_numpy(cand).to(DEV), 20.0, True)
        bad = cand.copy()
        bad[1, 2], bad[3, 0], bad[4, 3] = -1, 6, 2 ** 31 - 1
        got = ops.xattn_index_pairs_fwd(index, 6, G, mi6, Q, mc, torch.from_numpy(bad).to(DEV), 20.0, True)
        hole = torch.from_numpy(bad != cand).to(DEV)
        assert torch.isnan(got[hole]).all() and torch.equal(got[~hole], good[~hole]) and torch.isfinite(good).all()

    def test_forward_only(self):
        from demovlp_amd import DemoVLPHipError, functional as Fn
        C, Q, mi, mc = _inputs(2, 3, 30, 20, 1, torch.bfloat16)
        Q.requires_grad_(True)
        s = Fn.XattnIndexPairsFn.apply(_filled(C, 2, [2]), 2, 30, mi, Q, mc, torch.zeros(3, 2, device=DEV, dtype=torch.int32), 20.0, True)
        with pytest.raises(DemoVLPHipError):
            s.sum().backward()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3, 4, 6. search against trainer.evaluate on the retrieval set with signal (bf16, fused route)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _retrieval_model(F, R, sd, dtype):
    m = ObjectRelation({"model": "", "input_objects": False, "object_num": R, "num_frames": F, "time_module": None},
                       {"model": "pretrained/distilbert-base-uncased", "pretrained": True, "input": "text", "two_outputs": True}, pretrained_init=False, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.set_text_dropout(0.0)
    return m.to(DEV)


def _retrieval_batches(sd, F, R, BS, NB):
    for b in range(NB):
        obj, mask, ids, att = syn.retrieval_batch(sd, F, R, b * BS, BS)
        yield {"text": {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(att).to(DEV)},
               "object": torch.from_numpy(obj).to(DEV), "object_mask": torch.from_numpy(mask).to(DEV)}


LOSS = dict(use_local=True, use_global=True, coef=1.0, focal_type="equal")


@pytest.fixture(scope="module")
def g11():
    g = load_golden("g11_retrieval.npz")
    F, R, BS, NB = int(g["F"]), int(g["R"]), int(g["batch"]), int(g["batches"])
    sd = syn.retrieval_state_dict(F, R)
    model = _retrieval_model(F, R, sd, "bfloat16")
    loss = GlobalLocalLoss(**LOSS)
    batches = list(_retrieval_batches(sd, F, R, BS, NB))
    res = evaluate(model, loss, batches)
    index = search.VideoIndex(BS * NB, F * R, torch.bfloat16, DEV).add_batches(model, batches)
    text = {k: torch.cat([b["text"][k] for b in batches]) for k in ("input_ids", "attention_mask")}
    full = res["global_sims"].astype(np.float64) + res["local_sims"].T.astype(np.float64)       # the search orientation: [query, video]
    return dict(model=model, loss=loss, batches=batches, res=res, index=index, text=text, full=full, n=BS * NB)


def _search(g11, index=None, **kw):
    """Every caption of the set, searched batch by batch as ``trainer.evaluate`` runs the text tower (a tower's bf16 output depends on the
    batch it was computed in: the GEMM dispatch follows the row count), results concatenated."""
    parts = [(index or g11["index"]).search(g11["model"], g11["loss"], b["text"], **kw) for b in g11["batches"]]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _ordered(ids, scores):
    """best first, equal scores by smaller id"""
    s, i = scores[:, :-1], ids[:, :-1]
    return bool(((s > scores[:, 1:]) | ((s == scores[:, 1:]) & (i < ids[:, 1:]))).all())


class TestSearchOnTheRetrievalSet:
    def test_exact_search_equals_the_full_grid_in_the_search_orientation(self, g11):
        ix, full, n = g11["index"], g11["full"], g11["n"]
        assert len(ix) == n and ix.fused
        ids, scores = _search(g11, k=10, shortlist=None)
        assert ids.shape == (n, 10) and ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.is_cuda
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        dev = np.abs(scores - np.take_along_axis(full, ids, 1)).max()
        order = np.argsort(-full, axis=1, kind="stable")
        srt = np.take_along_axis(full, order, 1)
        gap = srt[:, :-1] - srt[:, 1:]                                                    # gap[p] = between positions p and p + 1
        clear = np.concatenate([np.ones((n, 1), bool), gap[:, :9] > RANK_GAP], 1) & (gap[:, :10] > RANK_GAP)
        print("\nexact search: max |score - (global + local.T)| %.2e; %d of %d positions clear of ties" % (dev, clear.sum(), clear.size))
        assert dev < SCORE_TOL, dev
        assert np.array_equal(ids[clear], order[:, :10][clear])
        assert _ordered(ids, scores) and clear.mean() > 0.9
        # the quirk orientation of trainer.evaluate is a different matrix (its metrics are not comparable)
        assert np.abs(g11["res"]["o2t_sims"] - full).max() > 1e-2

    def test_partial_shortlist_is_exact_on_the_shortlist(self, g11):
        ix, full, n, S = g11["index"], g11["full"], g11["n"], 32
        model, text = g11["model"], g11["text"]
        with torch.no_grad():
            gt = torch.cat([model.eval().compute_text(b["text"])[0] for b in g11["batches"]])
        sl, cos = ix.shortlist_by_cosine(gt, S)
        sl = sl.cpu().numpy()
        glob = g11["res"]["global_sims"].astype(np.float64)
        order = np.argsort(-glob, axis=1, kind="stable")
        srt = np.take_along_axis(glob, order, 1)
        decided = (srt[:, S - 1] - srt[:, S]) > RANK_GAP                                  # rows whose 32nd / 33rd are not within rounding
        print("\nshortlist 32: %d of %d rows have a clear cut" % (decided.sum(), n))
        assert decided.sum() > n // 2 and (np.diff(sl, axis=1) > 0).all()
        assert np.array_equal(sl[decided], np.sort(order[:, :S], axis=1)[decided])
        # every row, clear cut or not: no video left out beats a shortlisted one by more than rounding
        inside = np.zeros((n, n), bool)
        np.put_along_axis(inside, sl, True, 1)
        assert inside.sum(1).min() == S
        assert (np.where(inside, -np.inf, glob).max(1) <= np.where(inside, glob, np.inf).min(1) + RANK_GAP).all()
        assert np.abs(cos.cpu().numpy() - np.take_along_axis(glob, sl, 1)).max() < SCORE_TOL
        ids, scores = _search(g11, k=10, shortlist=S)
        all_ids, all_scores = _search(g11, k=S, shortlist=S)
        assert torch.equal(ids, all_ids[:, :10]) and torch.equal(scores, all_scores[:, :10])
        ids, scores, all_ids = ids.cpu().numpy(), scores.cpu().numpy(), all_ids.cpu().numpy()
        assert np.array_equal(np.sort(all_ids, axis=1), sl)                               # the re-ranked set IS the cosine shortlist
        assert np.abs(scores - np.take_along_axis(full, ids, 1)).max() < SCORE_TOL
        assert _ordered(ids, scores) and _ordered(all_ids, all_scores.cpu().numpy())

    def test_state_dict_round_trip_modes_and_chunks(self, g11, tmp_path):
        ix, model, loss, text = g11["index"], g11["model"], g11["loss"], g11["text"]
        ref = _search(g11, k=10, shortlist=32)
        torch.save(ix.state_dict(), tmp_path / "index.pt")
        back = search.VideoIndex(ix.capacity, ix.G, torch.bfloat16, DEV).load_state_dict(torch.load(tmp_path / "index.pt"))
        assert len(back) == len(ix)
        got = _search(g11, back, k=10, shortlist=32)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
        for chunk in (100, 64):                                                           # does not / does divide the 256 rows
            got = _search(g11, k=10, shortlist=32, chunk=chunk)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), chunk
        model.train()
        try:
            got = _search(g11, k=10, shortlist=32)
            assert model.training and not got[1].requires_grad and got[1].grad_fn is None
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
            model.eval()
            ix.search(model, loss, text, k=3, shortlist=8)
            assert not model.training
        finally:
            model.eval()

    def test_evaluate_t2v_with_a_full_shortlist_equals_the_metrics_of_the_full_grid(self, g11):
        from demovlp_amd import metric
        r = search.evaluate_t2v(g11["model"], g11["loss"], g11["batches"], shortlist=None)
        assert np.abs(r["sims"] - g11["full"]).max() < SCORE_TOL
        want = metric.t2v_metrics(g11["full"])
        print("\nsearch orientation t2v:", {k: r["t2v_metrics"][k] for k in ("R1", "R10", "MedR")}, "| full grid:", {k: want[k] for k in ("R1", "R10", "MedR")})
        assert abs(r["t2v_metrics"]["R1"] - want["R1"]) <= 100.0 * 3 / g11["n"]           # (a 2e-5 deviation can move a tied rank or two)
        part = search.evaluate_t2v(g11["model"], g11["loss"], g11["batches"], shortlist=64)
        print("shortlist 64 t2v:", {k: part["t2v_metrics"][k] for k in ("R1", "R10", "MedR")})       # recall here is a property of the synthetic weights: printed only


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. parity route (fp32): against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
class TestParityRoute:
    def test_fp32_scores_within_1e5_of_the_fp64_oracle(self):
        F, R, N, NQ, S, K = 8, 30, 12, 6, 5, 3
        sd = syn.retrieval_state_dict(F, R)
        model = _retrieval_model(F, R, sd, "float32")
        loss = GlobalLocalLoss(**LOSS)
        batches = list(_retrieval_batches(sd, F, R, 6, N // 6))
        ix = search.VideoIndex(N + 2, F * R, torch.float32, DEV)
        assert not ix.fused
        ix.add_batches(model, batches[:1])
        with torch.no_grad():
            out = model.eval()(batches[1], return_embeds=True)
        ix.add(out)                                                                       # the dict route
        assert len(ix) == N
        with pytest.raises(ValueError):
            ix.add_batches(model, batches[:1])                                            # 12 + 6 > 14
        text = {k: v[:NQ] for k, v in batches[0]["text"].items()}
        ids, scores = ix.search(model, loss, text, k=K, shortlist=S)
        with torch.no_grad():
            embeds = [model(b, return_embeds=True) for b in batches]
        go = torch.cat([e["global_object_embeddings"] for e in embeds]).cpu().double()
        lo = torch.cat([e["local_object_embeddings"] for e in embeds]).cpu().double()
        om = torch.cat([e["object_mask"] for e in embeds]).cpu().double()
        gt = embeds[0]["global_text_embeddings"][:NQ].cpu().double()
        lt = embeds[0]["local_text_embeddings"][:NQ].cpu().double()
        tm = ((text["attention_mask"][:, 1:] - 1.0) * 100.0).cpu().double()
        unit = lambda a: a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)
        cos = unit(gt) @ unit(go).T
        err = 0.0
        for j in range(NQ):
            for p in range(K):
                i = int(ids[j, p])
                want = float(orc.xattn_pair(lo[i], lt[j], om[i], tm[j], 20.0, True)) + float(cos[j, i])
                err = max(err, abs(float(scores[j, p]) - want))
        print("\nparity route: max |score - fp64 oracle| %.2e" % err)
        assert err < 1e-5, err
        assert _ordered(ids.cpu().numpy(), scores.cpu().numpy())
