"""Filtered search and row removal on a real MI355X: ``dvlp_topk_rows_masked`` against the numpy reference of
``tests/test_filtered_search.py`` (delete the disallowed columns, stable argsort, pad; exact equality of the indices and of the raw value
bits), ``search(allow=...)`` against a fresh index that holds only the allowed rows (ids exactly, scores bit for bit: the per-pair code
is the same, and the rows of the fresh index keep their order, so even a tie would be cut the same way), and ``remove`` / ``replace`` /
the state dict.

The search cases run on synthetic tower outputs (``_text_side`` / ``_video_side`` replaced, as ``tests/test_gpu_caption_moments.py``
does): what is under test is the path from the filter to the result, not a tower."""
import numpy as np
import pytest
import torch

from demovlp_amd import ops, search
from demovlp_amd.loss import RWALoss
from test_filtered_search import DENSITIES, allow_mask, masked_topk_ref, special_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                    # words of 0xFFFFFFFF on either side of the words the header says the kernel may load
LOSS = RWALoss(20, "equal")
MODEL = torch.nn.Identity()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the masked top-k against numpy
# ---------------------------------------------------------------------------------------------------------------------------------------
def _padded(x, pad=3):
    """x on the device inside a wider matrix (ld = N + pad: rows start at every 4-byte phase); the padding holds +inf: a read past N shows"""
    M, N = x.shape
    buf = torch.full((M, N + pad), float("inf"), device=DEV, dtype=torch.float32)
    buf[:, :N] = torch.from_numpy(x).to(DEV)
    return buf


def _guarded(allow, N, base):
    """The mask words of ``allow`` (bool [N] or [M, N], columns base .. base + N - 1) with EVERY other bit set: the bits below ``base`` and at
    or beyond ``base + N`` in the words that hold columns, the words below ``base >> 5``, and GUARD words of ones before and after each
    mask row.  -> a view [words] / [M, words] into the guarded buffer (word 0 = global columns 0 .. 31)."""
    words = (base + N + 31) // 32
    bits = np.ones(allow.shape[:-1] + (words * 32,), bool)
    bits[..., base:base + N] = allow
    packed = ops.pack_allow_bits(torch.from_numpy(bits).to(DEV)).view(torch.int32)
    buf = torch.full(allow.shape[:-1] + (GUARD + words + GUARD,), -1, device=DEV, dtype=torch.int32)
    buf[..., GUARD:GUARD + words] = packed
    return buf[..., GUARD:GUARD + words].view(torch.uint32)


def _check(got, want, tag):
    val, idx = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(idx, want[1]), (tag, "indices")
    assert np.array_equal(val.view(np.uint32), want[0].view(np.uint32)), (tag, "values, bit for bit")


def _with_base(ref, base):
    return ref[0], np.where(ref[1] >= 0, ref[1] + base, -1)


class TestMaskedTopkAgainstNumpy:
    @pytest.mark.parametrize("K", [1, 7, 1024])
    @pytest.mark.parametrize("N", [1, 5, 1023, 1024, 1025, 4099])          # a round is 1024 columns, a load 4
    @pytest.mark.parametrize("M", [3, 600])                                # rows split into column segments | one workgroup per row
    def test_masked_topk_equals_the_numpy_reference_bit_for_bit(self, M, N, K):
        x = special_rows(M, N, 11 * N + K + M)
        xd = _padded(x)
        plain = {base: ops.topk_rows(xd, K, N=N, index_base=base) for base in (0, 37, 64)}
        for density in DENSITIES:
            for per_row in (False, True):
                a = allow_mask(M, N, K, density, per_row, N + K + M)
                ref = masked_topk_ref(x, a, K)
                for base in (0, 37, 64):
                    words = _guarded(a, N, base)
                    assert words.dim() == (2 if per_row else 1) and (not per_row or words.stride(0) > words.shape[1])
                    got = ops.topk_rows_masked(xd, K, words, N=N, index_base=base)
                    _check(got, _with_base(ref, base), (M, N, K, density, per_row, base))
                    if density == "all":                               # nothing deleted: dvlp_topk_rows, bit for bit
                        assert torch.equal(got[1], plain[base][1]) and torch.equal(got[0].view(torch.int32), plain[base][0].view(torch.int32))
                    if density == "none":
                        assert (got[1] == -1).all() and torch.isneginf(got[0]).all()
                again = ops.topk_rows_masked(xd, K, words, N=N, index_base=64)      # two runs: equal bytes
                assert torch.equal(again[1], got[1]) and torch.equal(again[0].view(torch.int32), got[0].view(torch.int32))

    def test_masked_topk_special_values_on_both_sides_of_the_mask(self):
        """the largest value of every row (+inf) is disallowed and never listed; the allowed NaN and -inf are listed, after every number, with
        their indices and their bits; a duplicated value is cut by the index"""
        M, N, K = 3, 1025, 1024
        x = special_rows(M, N, 5)
        a = allow_mask(M, N, K, "half", True, 6)
        assert a[:, 1].all() and a[:, 2].all() and not a[:, N - 1].any() and np.isposinf(x[:, N - 1]).all()
        val, idx = ops.topk_rows_masked(_padded(x), K, _guarded(a, N, 0), N=N)
        _check((val, idx), masked_topk_ref(x, a, K), "specials")
        val, idx = val.cpu().numpy(), idx.cpu().numpy()
        for m in range(M):
            n = int(a[m].sum())
            assert n < K and (idx[m, n:] == -1).all() and np.isneginf(val[m, n:]).all()
            assert N - 1 not in idx[m] and not np.isposinf(val[m]).any()
            assert idx[m, n - 1] == 1 and val[m, n - 1:n].view(np.uint32)[0] == 0xffc00123      # the NaN, last, payload and sign intact
            assert 2 in idx[m, :n - 1] and np.isneginf(val[m, list(idx[m]).index(2)])

    @pytest.mark.parametrize("M,N,K", [(3, 1025, 7), (3, 4099, 1024), (600, 1025, 7)])
    @pytest.mark.parametrize("density", ["few", "half"])
    def test_masked_topk_streamed_in_chunks_of_100_equals_the_one_shot_call(self, M, N, K, density):
        x = special_rows(M, N, N + K)
        xd = _padded(x)
        for base in (0, 37):                                           # chunk bases 100, 200, ... / 137, 237, ...: no multiple of 32
            for per_row in (False, True):
                a = allow_mask(M, N, K, density, per_row, 2 * N + K)
                words = _guarded(a, N, base)
                one = ops.topk_rows_masked(xd, K, words, N=N, index_base=base)
                _check(one, _with_base(masked_topk_ref(x, a, K), base), (M, N, K, density, per_row, base))
                out = (torch.empty((M, K), device=DEV), torch.empty((M, K), device=DEV, dtype=torch.int32))
                for c0 in range(0, N, 100):
                    ops.topk_rows_masked(xd[:, c0:], K, words, N=min(100, N - c0), index_base=base + c0, out=out, merge=c0 > 0)
                assert torch.equal(out[1], one[1]), (base, per_row, "indices")
                assert torch.equal(out[0].view(torch.int32), one[0].view(torch.int32)), (base, per_row, "values")

    def test_masked_topk_reads_neither_the_guard_words_nor_the_padding(self):
        """All columns disallowed, every bit around them set (``_guarded``: the neighbouring bits of the first and last word, the words below
        ``index_base >> 5``, 64 words of ones on either side of each mask row) and +inf in x beyond N: a single bit or value read from outside
        would be listed."""
        for M, N, base in [(3, 1025, 37), (600, 33, 64), (3, 4099, 0), (3, 5, 91)]:
            x = special_rows(M, N, N)
            for per_row in (False, True):
                a = np.zeros((M, N) if per_row else (N,), bool)
                val, idx = ops.topk_rows_masked(_padded(x, 5), 7, _guarded(a, N, base), N=N, index_base=base)
                assert (idx == -1).all() and torch.isneginf(val).all(), (M, N, base, per_row)
                a[..., N - 1] = True                                   # the last column alone: the bit next to the first one never read
                val, idx = ops.topk_rows_masked(_padded(x, 5), 7, _guarded(a, N, base), N=N, index_base=base)
                assert (idx[:, 0] == base + N - 1).all() and (idx[:, 1:] == -1).all() and torch.isneginf(val[:, 1:]).all(), (M, N, base, per_row)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. search on small indexes (synthetic tower outputs)
# ---------------------------------------------------------------------------------------------------------------------------------------
N_ROWS, NQ, W_WORDS = 40, 5, 12


def _videos(n, G, seed, dtype=torch.bfloat16):
    rng = np.random.default_rng(seed)
    om = np.zeros((n, G), np.float32)
    om[1::3, G - 3:] = -100.0                                      # some masked tails
    t = lambda a: torch.from_numpy(a).to(DEV)
    return (t(rng.standard_normal((n, 256), dtype=np.float32)).to(dtype), t(rng.standard_normal((n, G, 256), dtype=np.float32)).to(dtype), t(om))


def _captions(n, W, seed, dtype=torch.bfloat16):
    """-> (global [n, 256], local [n, W, 256], attention mask [n, W + 1] with ragged lengths)"""
    rng = np.random.default_rng(seed)
    att = np.zeros((n, W + 1), np.float32)
    for j in range(n):
        att[j, :2 + (5 * j + 3) % W] = 1.0
    t = lambda a: torch.from_numpy(a).to(DEV)
    return (t(rng.standard_normal((n, 256), dtype=np.float32)).to(dtype), t(rng.standard_normal((n, W, 256), dtype=np.float32)).to(dtype), t(att))


def _video_index(vid, rows=None, tiled=False, capacity=None):
    go, lo, om = (t if rows is None else t[rows] for t in vid)
    ix = search.VideoIndex(capacity or go.shape[0], lo.shape[1], lo.dtype, DEV, tiled=tiled)
    ix.add(dict(global_object_embeddings=go, local_object_embeddings=lo, object_mask=om))
    return ix


def _caption_index(cap, rows=None, tiled=False, capacity=None):
    gt, lt, att = (t if rows is None else t[rows] for t in cap)
    ix = search.CaptionIndex(capacity or gt.shape[0], lt.shape[1], lt.dtype, DEV, tiled=tiled)
    ix.add(gt, lt, att)
    return ix


class _T2V:
    """text-to-video: a VideoIndex of N_ROWS videos of G regions searched by NQ synthetic captions of W_WORDS words"""

    def __init__(self, G, tiled=False, dtype=torch.bfloat16, n=N_ROWS):
        self.rows_data = _videos(n, G, 100 + G, dtype)
        gt, lt, att = _captions(NQ, W_WORDS, 200 + G, dtype)
        self.side = (gt, lt.contiguous(), (att[:, 1:].contiguous() - 1.0) * 100.0)
        self.query = dict(input_ids=torch.zeros(NQ, W_WORDS + 1, device=DEV, dtype=torch.long), attention_mask=att)
        self.tiled, self.n, self.global_query = tiled, n, gt
        self.index = self.make()

    def make(self, rows=None, capacity=None):
        ix = _video_index(self.rows_data, rows, self.tiled, capacity)
        ix._text_side = lambda model, block: self.side
        return ix


class _V2T:
    """video-to-text: a CaptionIndex of N_ROWS captions of W_WORDS words searched by NQ synthetic videos of G regions (F = 4 frames)"""

    def __init__(self, G, tiled=False):
        self.rows_data = _captions(N_ROWS, W_WORDS, 300 + G)
        go, lo, om = _videos(NQ, G, 400 + G)
        self.side = (go, lo.contiguous(), om)
        self.query = dict(object=torch.zeros(NQ, 4, G // 4, 1, device=DEV), object_mask=torch.ones(NQ, 4, G // 4, device=DEV))
        self.tiled, self.n, self.global_query = tiled, N_ROWS, go
        self.index = self.make()

    def make(self, rows=None, capacity=None):
        ix = _caption_index(self.rows_data, rows, self.tiled, capacity)
        ix._video_side = lambda model, block: self.side
        return ix


@pytest.fixture(scope="module", params=["t2v fused G=36", "t2v tiled G=160", "v2t fused", "v2t tiled"])
def case(request):
    return {"t2v fused G=36": lambda: _T2V(36), "t2v tiled G=160": lambda: _T2V(160, tiled=True), "v2t fused": lambda: _V2T(36),
            "v2t tiled": lambda: _V2T(36, tiled=True)}[request.param]()


def _find(c, index=None, **kw):
    return (index or c.index).search(MODEL, LOSS, c.query, **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _shared_mask(n, seed=0):
    m = torch.from_numpy(np.random.default_rng(seed).random(n) < 0.5).to(DEV)
    m[:2] = torch.tensor([False, True], device=DEV)
    return m


def _against_fresh(c, mask_row, got_ids, got_scores, k, shortlist, q=None):
    """(ids, scores) of a filtered search == those of a fresh index holding only the allowed rows, ids mapped back"""
    rows = torch.nonzero(mask_row)[:, 0]
    ids, scores = _find(c, c.make(rows), k=k, shortlist=shortlist)
    sel = slice(None) if q is None else slice(q, q + 1)
    assert torch.equal(got_ids[sel], rows[ids][sel]), (q, "ids")
    assert torch.equal(_bits(got_scores[sel]), _bits(scores[sel])), (q, "scores, bit for bit")


class TestFilteredSearch:
    @pytest.mark.parametrize("shortlist", [8, None])                       # the masked cut | the exact branch (S == n)
    def test_search_with_a_filter_equals_search_on_a_fresh_index_of_the_allowed_rows(self, case, shortlist):
        mask = _shared_mask(case.n)
        assert 10 <= int(mask.sum()) <= 30
        ids, scores = _find(case, k=5, shortlist=shortlist, allow=mask)
        assert ids.dtype == torch.int64 and tuple(ids.shape) == (NQ, 5) and mask[ids].all() and torch.isfinite(scores).all()
        assert (scores[:, :-1] > scores[:, 1:]).all()                   # separated scores: no comparison rests on a tie
        _against_fresh(case, mask, ids, scores, 5, shortlist)
        # one mask per query
        per = torch.from_numpy(np.random.default_rng(1).random((NQ, case.n)) < 0.5).to(DEV)
        per[0] = mask
        ids, scores = _find(case, k=5, shortlist=shortlist, allow=per)
        assert torch.gather(per, 1, ids).all()
        for q in range(NQ):
            _against_fresh(case, per[q], ids, scores, 5, shortlist, q)
        assert not torch.equal(ids[1:], _find(case, k=5, shortlist=shortlist, allow=mask)[0][1:])      # (the rows of the mask matter)

    def test_fewer_allowed_rows_than_asked_for_end_in_holes(self, case):
        mask = torch.zeros(case.n, device=DEV, dtype=torch.bool)
        mask[[4, 20, 33]] = True
        for shortlist in (8, None):
            ids, scores = _find(case, k=5, shortlist=shortlist, allow=mask)
            assert (ids[:, 3:] == -1).all() and torch.isneginf(scores[:, 3:]).all() and torch.isfinite(scores[:, :3]).all()
            assert (ids[:, :3].sort(dim=1)[0] == torch.tensor([4, 20, 33], device=DEV)).all()
            _against_fresh(case, mask, ids[:, :3], scores[:, :3], 3, None)
        sl, cos = case.index.shortlist_by_cosine(case.global_query, 8, allow=mask)
        assert sl.tolist() == [[-1] * 5 + [4, 20, 33]] * NQ and torch.isneginf(cos[:, :5]).all() and torch.isfinite(cos[:, 5:]).all()
        # the k winners with grounding: a hole answers as an id outside the index does
        out = _find(case, k=5, shortlist=8, allow=mask, ground=True, frames=4)
        assert torch.equal(out[0], ids) and torch.isnan(out[2]["score"][:, 3:]).all() and torch.isfinite(out[2]["score"][:, :3]).all()
        none = torch.zeros(case.n, device=DEV, dtype=torch.bool)
        ids, scores = _find(case, k=2, shortlist=8, allow=none)
        assert (ids == -1).all() and torch.isneginf(scores).all()

    def test_a_filter_of_all_ones_changes_nothing(self, case):
        for shortlist in (8, None):
            ref = _find(case, k=5, shortlist=shortlist)
            for allow in (torch.ones(case.n, device=DEV, dtype=torch.bool), torch.ones(NQ, case.n, device=DEV, dtype=torch.bool)):
                got = _find(case, k=5, shortlist=shortlist, allow=allow)
                assert torch.equal(got[0], ref[0]) and torch.equal(_bits(got[1]), _bits(ref[1]))
        a, b = case.index.shortlist_by_cosine(case.global_query, 8), case.index.shortlist_by_cosine(case.global_query, 8, allow=allow)
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))

    def test_a_narrow_filter_finds_rows_a_host_side_post_filter_loses(self, case):
        """the reason for the kernel: allow only the rows the cosine shortlist of query 0 leaves out"""
        sl, _ = case.index.shortlist_by_cosine(case.global_query, 8)
        mask = torch.ones(case.n, device=DEV, dtype=torch.bool)
        mask[sl[0]] = False
        ids, _ = _find(case, k=8, shortlist=8)                          # search, then filter on the host: nothing survives for query 0
        assert not mask[ids[0]].any()
        ids, scores = _find(case, k=8, shortlist=8, allow=mask)
        assert mask[ids[0]].all() and torch.isfinite(scores[0]).all()

    def test_timeline_with_a_filter_lists_no_disallowed_caption(self):
        c = _V2T(36, tiled=True)
        mask = _shared_mask(c.n, 3)
        tl = c.index.timeline(MODEL, LOSS, c.query, 4, 2, k=3, shortlist=8, allow=mask)
        assert tuple(tl["ids"].shape) == (NQ, 3, 3) and mask[tl["ids"]].all() and torch.isfinite(tl["scores"]).all()
        rows = torch.nonzero(mask)[:, 0]
        want = c.make(rows).timeline(MODEL, LOSS, c.query, 4, 2, k=3, shortlist=8)
        assert torch.equal(tl["ids"], rows[want["ids"]]) and torch.equal(_bits(tl["scores"]), _bits(want["scores"]))
        assert torch.equal(_bits(tl["cosine"]), _bits(want["cosine"]))
        few = torch.zeros(c.n, device=DEV, dtype=torch.bool)
        few[[7, 8]] = True
        tl = c.index.timeline(MODEL, LOSS, c.query, 4, 2, k=3, shortlist=8, allow=few)
        assert (tl["ids"][..., :2].sort(dim=-1)[0] == torch.tensor([7, 8], device=DEV)).all() and (tl["ids"][..., 2] == -1).all()
        assert torch.isneginf(tl["scores"][..., 2]).all() and torch.isnan(tl["cosine"][..., 2]).all() and torch.isfinite(tl["cosine"][..., :2]).all()

    def test_the_fp32_route_drops_the_holes_of_a_query_before_it_gathers(self):
        c = _T2V(20, dtype=torch.float32, n=12)
        assert not c.index.fused
        mask = torch.zeros(12, device=DEV, dtype=torch.bool)
        mask[[1, 5, 6, 10]] = True
        for shortlist in (6, None):
            ids, scores = _find(c, k=5, shortlist=shortlist, allow=mask)
            assert (ids[:, 4] == -1).all() and torch.isneginf(scores[:, 4]).all() and mask[ids[:, :4]].all()
            _against_fresh(c, mask, ids[:, :4], scores[:, :4], 4, None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. removal and replacement
# ---------------------------------------------------------------------------------------------------------------------------------------
GONE = [3, 17]


def _same_index(a, b):
    for name in ("gn", "local") + (("om",) if hasattr(a, "om") else ("tm",)):
        assert torch.equal(getattr(a, name).view(torch.uint8), getattr(b, name).view(torch.uint8)), name


class TestRemovalAndReplacement:
    def test_removed_rows_are_in_no_result_and_answer_as_holes(self, case):
        ix = case.make()
        without = torch.ones(case.n, device=DEV, dtype=torch.bool)
        without[GONE] = False
        assert ix.alive is None and ix.live == case.n and "alive" not in ix.state_dict()
        assert ix.remove(torch.tensor(GONE)) is ix
        assert len(ix) == case.n and ix.live == case.n - 2 and ix.removed().tolist() == GONE and ix.removed().dtype == torch.int64
        assert not ix.gn[GONE].any() and ix.gn[4].any()                                    # a saved index does not carry the embeddings
        assert ix.alive.dtype == torch.uint32 and ix.alive.cpu().tolist() == [0xFFFFFFFF & ~(1 << 3 | 1 << 17), 0xFF]
        words = ix.alive.clone()
        ix.remove([17])                                                                    # twice: a no-op
        assert torch.equal(ix.alive.view(torch.int32), words.view(torch.int32)) and ix.live == case.n - 2
        for shortlist in (8, None):
            ids, scores = _find(case, ix, k=8, shortlist=shortlist)
            assert not torch.isin(ids, torch.tensor(GONE, device=DEV)).any() and (ids >= 0).all()
            ref = _find(case, k=8, shortlist=shortlist, allow=without)                     # == filtering them out of an untouched index
            assert torch.equal(ids, ref[0]) and torch.equal(_bits(scores), _bits(ref[1]))
        k_all = _find(case, ix, k=case.n, shortlist=None)                                  # every row asked for: the two holes come last
        assert (k_all[0][:, -2:] == -1).all() and torch.isneginf(k_all[1][:, -2:]).all() and (k_all[0][:, :-2] >= 0).all()
        sl, _ = ix.shortlist_by_cosine(case.global_query, 8)
        assert not torch.isin(sl, torch.tensor(GONE, device=DEV)).any() and (sl >= 0).all()
        # a filter on top of the removal: ANDed
        only = torch.zeros(case.n, device=DEV, dtype=torch.bool)
        only[[3, 4, 17, 20]] = True
        ids, _ = _find(case, ix, k=3, shortlist=8, allow=only)
        assert (ids[:, :2].sort(dim=1)[0] == torch.tensor([4, 20], device=DEV)).all() and (ids[:, 2] == -1).all()
        # explicit ids: a removed row is a hole, the others are what they were
        ask = torch.tensor([[3, 5, 17]] * NQ, device=DEV)
        g, ref = ix.ground(MODEL, LOSS, case.query, ask, frames=4), case.index.ground(MODEL, LOSS, case.query, ask, frames=4)
        hole = case.index.ground(MODEL, LOSS, case.query, torch.full_like(ask, -1), frames=4)
        for name in ("score", "word_scores", "region_scores", "frame_scores", "word_region", "region_word"):
            assert torch.equal(g[name][:, 1].contiguous().view(torch.uint8), ref[name][:, 1].contiguous().view(torch.uint8)), name
            assert torch.equal(g[name][:, ::2].contiguous().view(torch.uint8), hole[name][:, ::2].contiguous().view(torch.uint8)), name
        assert torch.isnan(g["score"][:, ::2]).all() and torch.isfinite(g["score"][:, 1]).all()
        if case.tiled:
            m = ix.moments(MODEL, LOSS, case.query, ask, 4, 2)
            assert torch.isnan(m["scores"][:, ::2]).all() and (m["best"][:, ::2] == -1).all() and torch.isnan(m["best_score"][:, ::2]).all()
            assert torch.isfinite(m["scores"][:, 1]).all() and (m["best"][:, 1] >= 0).all()
        if case.tiled and isinstance(ix, search.CaptionIndex):
            tl = ix.timeline(MODEL, LOSS, case.query, 4, 2, k=5, shortlist=None)
            assert not torch.isin(tl["ids"], torch.tensor(GONE, device=DEV)).any() and (tl["ids"] >= 0).all()

    def test_replace_writes_the_bytes_of_a_fresh_index_and_revives_the_row(self, case):
        other = tuple(t[:1] for t in (_videos if isinstance(case, _T2V) else _captions)(2, case.rows_data[1].shape[1], 999))
        ix = case.make().remove(GONE)
        if isinstance(case, _T2V):
            ix.replace([3], dict(global_object_embeddings=other[0], local_object_embeddings=other[1], object_mask=other[2]))
        else:
            ix.replace([3], *other)
        assert ix.removed().tolist() == [17] and ix.live == case.n - 1 and len(ix) == case.n
        # the fresh index: the same rows with ``other`` in place of row 3, added in one call; row 17 is compared after its removal there too
        data = tuple(torch.cat([t[:3], o, t[4:]]) for t, o in zip(case.rows_data, other))
        fresh = (_video_index if isinstance(case, _T2V) else _caption_index)(data, tiled=case.tiled)
        fresh._text_side = fresh._video_side = lambda model, block: case.side
        fresh.remove([17])
        _same_index(ix, fresh)
        assert torch.equal(ix.alive.view(torch.int32), fresh.alive.view(torch.int32))
        got, want = _find(case, ix, k=case.n - 1, shortlist=None), _find(case, fresh, k=case.n - 1, shortlist=None)
        assert torch.equal(got[0], want[0]) and torch.equal(_bits(got[1]), _bits(want[1])) and (got[0] == 3).any(1).all() and (got[0] >= 0).all()
        # replacing a live row in place changes that row alone
        before = case.make()
        again = case.make()
        again.replace([5, 6], *((dict(global_object_embeddings=case.rows_data[0][5:7], local_object_embeddings=case.rows_data[1][5:7],
                                      object_mask=case.rows_data[2][5:7]),) if isinstance(case, _T2V) else tuple(t[5:7] for t in case.rows_data)))
        _same_index(again, before)
        assert again.alive is None

    def test_state_dict_round_trips_alive_and_an_untouched_index_saves_none(self, case, tmp_path):
        ix = case.make()
        keys = set(ix.state_dict())
        assert "alive" not in keys and keys == {"capacity", "dtype", "n", "fused", "gn", "local"} | ({"tiled"} if case.tiled else set()) \
            | ({"G", "om"} if isinstance(case, _T2V) else {"W", "tm"})
        ix.remove(GONE)
        torch.save(ix.state_dict(), tmp_path / "index.pt")
        state = torch.load(tmp_path / "index.pt")
        assert set(state) == keys | {"alive"} and not state["gn"][GONE].any()
        back = case.make(rows=torch.arange(2, device=DEV), capacity=case.n).load_state_dict(state)      # (an index that held something else)
        assert back.removed().tolist() == GONE and back.live == case.n - 2 and len(back) == case.n
        _same_index(back, ix)
        a, b = _find(case, ix, k=8, shortlist=8), _find(case, back, k=8, shortlist=8)
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1]))
        # loading a state without the key clears the mask
        assert back.load_state_dict(case.index.state_dict()).alive is None and back.live == case.n
