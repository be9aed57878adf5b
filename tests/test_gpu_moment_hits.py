"""Moment retrieval on a real MI355X (product library): ``dvlp_moment_select`` (``csrc/moments.hip``) held to the numpy
restatement ``tests/moment_select_ref.py`` bit for bit -- values as raw bits, positions exactly -- its mechanics, ``moments(..., top=...)`` on
both index classes, and ``VideoIndex.search_moments`` against a composition of the public pieces it is made of, on a planted moment and
through the holes of a filter and a removal.  Nothing here has a tolerance: the selection copies bits and compares integers, and the one
float operation of ``search_moments`` beyond its parts (cosine + window score) is repeated on the device by the composition."""
import numpy as np
import pytest
import torch

from demovlp_amd import _lib, ops, search, synthetic as syn
from demovlp_amd.loss import GlobalLocalLoss
from moment_select_ref import moment_select_ref, overlap, suppresses
from test_gpu_long_search import _retrieval_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
#          P     M     T     what it stresses
SHAPES = [(1, 1, 1),          # smallest shape
          (3, 5, 4),          # more picks asked than selectable
          (7, 63, 3),         # just under one lane-width
          (5, 64, 8),         # exactly one lane-width
          (4, 65, 8),         # just over one lane-width
          (9, 257, 16),
          (2, 1024, 32),
          (2, 1025, 5),
          (3, 4096, 32),      # largest M and T
          (1001, 37, 3)]      # many workgroups, a ragged last one
IOUS = [0.0, 0.3, 0.5, 1.0]
PAD = 3                       # ld = M + 3, NaN in the padding columns


def _bits(t):
    return t.contiguous().view(torch.int32)


def _window_sets(M):
    """two window lists of M windows: four lengths at stride 1 (cut or tiled to M), and one single length"""
    out = []
    for F, lengths in ((16, (1, 2, 4, 8)), (min(M + 2, 1000), 3)):
        s, l = search.moment_windows(F, lengths, 1)
        out.append((np.resize(s.numpy(), M), np.resize(l.numpy(), M)))
    return out


def _score_sets(P, M, seed):
    """the score matrices [P, M] of one shape: N(0, 1); multiples of 0.25 (many ties, some -0.0); scattered -inf; scattered NaN; one all -inf row;
    one all-NaN row"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((P, M)).astype(np.float32)
    q = (np.round(x * 2) / 4).astype(np.float32)
    holes = q.copy()
    holes[rng.random((P, M)) < 0.4] = -np.inf
    nans = x.copy()
    nans[rng.random((P, M)) < 0.3] = np.nan
    empty, lost = q.copy(), x.copy()
    empty[P // 2] = -np.inf
    lost[P // 2] = np.nan
    return dict(normal=x, quantised=q, scattered_neg_inf=holes, scattered_nan=nans, an_all_neg_inf_row=empty, an_all_nan_row=lost)


def _padded(x):
    """x [P, M] -> a device matrix [P, M + PAD] with NaN in the padding columns"""
    buf = np.full((x.shape[0], x.shape[1] + PAD), np.nan, np.float32)
    buf[:, :x.shape[1]] = x
    return torch.from_numpy(buf).to(DEV)


class TestKernelAgainstTheRestatement:
    @pytest.mark.parametrize("P,M,T", SHAPES)
    @pytest.mark.parametrize("iou", IOUS)
    def test_values_as_bits_and_positions_exactly(self, P, M, T, iou):
        for w, (start, length) in enumerate(_window_sets(M)):
            ds, dl = torch.from_numpy(start).to(DEV).int(), torch.from_numpy(length).to(DEV).int()
            for name, x in _score_sets(P, M, 100 * M + P + w).items():
                val, pos = ops.moment_select(_padded(x), ds, dl, T, iou, M=M)
                assert val.shape == (P, T) and pos.shape == (P, T) and val.dtype == torch.float32 and pos.dtype == torch.int32
                want_val, want_pos = moment_select_ref(x, start, length, T, iou)
                tag = (name, "windows %d" % w)
                assert np.array_equal(pos.cpu().numpy(), want_pos), tag
                assert np.array_equal(_bits(val).cpu().numpy(), want_val.view(np.int32)), tag

    def test_windows_given_on_the_host_are_uploaded(self):
        start, length = search.moment_windows(16, (2, 4), 1)
        x = torch.from_numpy(_score_sets(6, start.numel(), 1)["quantised"]).to(DEV)
        val, pos = ops.moment_select(x.view(2, 3, -1), start, length, 3, 0.5)
        assert val.shape == (2, 3, 3) and pos.shape == (2, 3, 3)
        want_val, want_pos = moment_select_ref(x.cpu().numpy(), start.numpy(), length.numpy(), 3, 0.5)
        assert np.array_equal(pos.view(6, 3).cpu().numpy(), want_pos) and np.array_equal(_bits(val).view(6, 3).cpu().numpy(), want_val.view(np.int32))


class TestKernelMechanics:
    @pytest.mark.parametrize("P,M,T", [(5, 64, 8), (1001, 37, 3), (3, 4096, 32)])
    def test_nothing_outside_the_outputs_is_written_and_two_calls_agree(self, P, M, T):
        start, length = _window_sets(M)[0]
        ds, dl = torch.from_numpy(start).to(DEV).int(), torch.from_numpy(length).to(DEV).int()
        x = _padded(_score_sets(P, M, 9)["scattered_neg_inf"])
        val, pos = ops.moment_select(x, ds, dl, T, 0.5, M=M)
        again = ops.moment_select(x, ds, dl, T, 0.5, M=M)
        assert torch.equal(_bits(val), _bits(again[0])) and torch.equal(pos, again[1])
        guard, n = 64, P * T
        vbuf = torch.full((n + 2 * guard,), -12345.0, device=DEV, dtype=torch.float32)
        pbuf = torch.full((n + 2 * guard,), -777, device=DEV, dtype=torch.int32)
        v, q = vbuf[guard:guard + n], pbuf[guard:guard + n]
        _lib.call("dvlp_moment_select", P, M, ops.p(x), M + PAD, ops.p(ds), ops.p(dl), T, 0.5, ops.p(v), ops.p(q), ops.stream())
        torch.cuda.synchronize()
        assert torch.equal(_bits(v), _bits(val).view(-1)) and torch.equal(q, pos.view(-1))
        for buf, fill in ((vbuf, -12345.0), (pbuf, -777)):
            assert (buf[:guard] == fill).all() and (buf[guard + n:] == fill).all()

    @pytest.mark.parametrize("P,M,T", [(4, 65, 8), (9, 257, 16), (1001, 37, 3)])
    def test_iou_one_on_finite_rows_is_the_row_top_k(self, P, M, T):
        start, length = _window_sets(M)[0]
        for name in ("normal", "quantised"):
            x = torch.from_numpy(_score_sets(P, M, 4)[name]).to(DEV)
            val, pos = ops.moment_select(x, torch.from_numpy(start), torch.from_numpy(length), T, 1.0)
            tval, tidx = ops.topk_rows(x, T)
            assert torch.equal(pos, tidx) and torch.equal(_bits(val), _bits(tval)), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# index level: a small tiled index in the style of tests/test_gpu_moments.py's e2e fixture (F = 8, R = 4, 12 videos, 6 queries)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _videos(b):
    return {"object": b["object"], "object_mask": b["object_mask"]}


@pytest.fixture(scope="module")
def e2e():
    F, R, N = 8, 4, 12
    sd = syn.retrieval_state_dict(F, R)
    model = _retrieval_model(F, R, sd, "bfloat16").eval()
    loss = GlobalLocalLoss(use_local=True, use_global=True, coef=1.0, focal_type="equal")
    batches = []
    for b in range(N // 6):
        obj, mask, ids, att = syn.retrieval_batch(sd, F, R, b * 6, 6)
        batches.append({"text": {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(att).to(DEV)},
                        "object": torch.from_numpy(obj).to(DEV), "object_mask": torch.from_numpy(mask).to(DEV)})
    W = batches[0]["text"]["input_ids"].shape[1] - 1
    vix = search.VideoIndex(N, F * R, torch.bfloat16, DEV, tiled=True).add_batches(model, batches)
    cix = search.CaptionIndex(N, W, torch.bfloat16, DEV, tiled=True).add_batches(model, batches)
    return dict(model=model, loss=loss, batches=batches, text=batches[0]["text"], vix=vix, cix=cix, F=F, R=R, N=N)


OLD_KEYS = {"scores", "start", "length", "best", "best_start", "best_length", "best_score"}
TOP_KEYS = {"top", "top_start", "top_length", "top_score"}


def _check_top(mo, old, m, iou):
    """the ``top*`` keys of a moments dict against the restatement on its own ``scores``; column 0 against ``best*``; the rest against ``old``"""
    assert set(mo) == OLD_KEYS | TOP_KEYS and set(old) == OLD_KEYS
    for name in OLD_KEYS:
        assert old[name].dtype == mo[name].dtype and torch.equal(old[name].contiguous().view(torch.uint8), mo[name].contiguous().view(torch.uint8)), name
    N, k, M = mo["scores"].shape
    start, length = mo["start"].cpu().numpy(), mo["length"].cpu().numpy()
    val, pos = moment_select_ref(mo["scores"].cpu().numpy().reshape(N * k, M), start, length, m, iou)
    pos = pos.reshape(N, k, m).astype(np.int64)
    assert (pos >= 0).all() and (pos[..., 0] != pos[..., 1]).all()                 # (the fixture has no hole and more than one free window per pair)
    assert mo["top"].dtype == torch.int64 and mo["top_start"].dtype == torch.int64 and mo["top_length"].dtype == torch.int64
    assert np.array_equal(mo["top"].cpu().numpy(), pos)
    assert np.array_equal(mo["top_start"].cpu().numpy(), start[pos]) and np.array_equal(mo["top_length"].cpu().numpy(), length[pos])
    assert mo["top_score"].dtype == torch.float32 and np.array_equal(_bits(mo["top_score"]).cpu().numpy(), val.view(np.int32).reshape(N, k, m))
    for name in ("", "_start", "_length"):
        assert torch.equal(mo["top" + name][..., 0], mo["best" + name]), name
    assert torch.equal(_bits(mo["top_score"][..., 0]), _bits(mo["best_score"]))


class TestMomentsWithTop:
    def test_video_index(self, e2e):
        vix, model, loss, text, F, N = e2e["vix"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"], e2e["N"]
        ids = torch.arange(N, device=DEV).expand(6, -1).contiguous()
        old = vix.moments(model, loss, text, ids, F, (2, 4))
        _check_top(vix.moments(model, loss, text, ids, F, (2, 4), top=3, iou=0.5), old, 3, 0.5)

    def test_a_hole_is_minus_one_and_nan(self, e2e):
        vix, model, loss, text, F = e2e["vix"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"]
        ids = torch.tensor([[0, -1, 3]], device=DEV).expand(6, -1).contiguous()
        mo = vix.moments(model, loss, text, ids, F, (2, 4), top=2)
        for name in ("top", "top_start", "top_length"):
            assert (mo[name][:, 1] == -1).all() and (mo[name][:, 0] >= 0).all() and (mo[name][:, 2] >= 0).all(), name
        assert torch.isnan(mo["top_score"][:, 1]).all() and torch.isfinite(mo["top_score"][:, 0]).all()

    def test_caption_index(self, e2e):
        cix, model, loss, F, N = e2e["cix"], e2e["model"], e2e["loss"], e2e["F"], e2e["N"]
        data = _videos(e2e["batches"][1])
        ids = torch.arange(N, device=DEV).expand(6, -1).contiguous()
        old = cix.moments(model, loss, data, ids, F, (2, 4))
        _check_top(cix.moments(model, loss, data, ids, F, (2, 4), top=3, iou=0.5), old, 3, 0.5)

    def test_search_passes_top_through(self, e2e):
        vix, cix, model, loss, text, F = e2e["vix"], e2e["cix"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"]
        ids, scores, mo = vix.search(model, loss, text, k=3, shortlist=5, frames=F, moments=(2, 4), moment_top=2, moment_iou=0.3)
        ids0, scores0, old = vix.search(model, loss, text, k=3, shortlist=5, frames=F, moments=(2, 4))
        assert torch.equal(ids, ids0) and torch.equal(_bits(scores), _bits(scores0))
        _check_top(mo, old, 2, 0.3)
        data = _videos(e2e["batches"][0])
        cids, _, cmo = cix.search(model, loss, data, k=3, shortlist=5, frames=F, moments=(2, 4), moment_top=2, moment_iou=0.3)
        _check_top(cmo, cix.moments(model, loss, data, cids, F, (2, 4)), 2, 0.3)


def _composed(ix, model, loss, text, k, F, windows, stride, per_video, iou, shortlist, allow=None):
    """``search_moments`` out of public pieces: ``shortlist_by_cosine``, ``moments`` on the whole shortlist, the numpy restatement, the fp32 add
    on the device, a stable sort -> (ids, start, length int64 [Nq, k], scores fp32 [Nq, k]) on the host"""
    with torch.no_grad():
        gt, _ = model.compute_text(text)
    ids, cos = ix.shortlist_by_cosine(gt, shortlist, allow=allow)
    mo = ix.moments(model, loss, text, ids, F, windows, stride)
    Nq, S, M = mo["scores"].shape
    start, length = mo["start"].cpu().numpy(), mo["length"].cpu().numpy()
    val, pos = moment_select_ref(mo["scores"].cpu().numpy().reshape(Nq * S, M), start, length, per_video, iou)
    total = (torch.from_numpy(val).to(DEV).view(Nq, S, per_video) + cos[:, :, None]).view(Nq, S * per_video).cpu().numpy()
    key = np.where(np.isnan(total), -np.inf, total)                             # NaN last; a NaN and a -inf entry are both padding: reported alike
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    window = np.take_along_axis(pos.reshape(Nq, S * per_video).astype(np.int64), order, 1)
    video = np.take_along_axis(ids.cpu().numpy(), order // per_video, 1)
    none, at = window < 0, np.clip(window, 0, M - 1)
    score = np.where(none, np.float32(-np.inf), np.take_along_axis(total, order, 1)).astype(np.float32)
    return np.where(none, -1, video), np.where(none, -1, start[at]), np.where(none, -1, length[at]), score


def _same_hits(got, want):
    assert set(got) == {"ids", "start", "length", "scores"}
    for name, ref in zip(("ids", "start", "length"), want[:3]):
        assert got[name].dtype == torch.int64 and np.array_equal(got[name].cpu().numpy(), ref), name
    assert got["scores"].dtype == torch.float32 and np.array_equal(_bits(got["scores"]).cpu().numpy(), want[3].view(np.int32))


class TestSearchMoments:
    @pytest.mark.parametrize("shortlist", [5, None])
    @pytest.mark.parametrize("per_video,iou", [(1, 0.5), (3, 0.3)])
    def test_against_a_composition_of_the_public_pieces(self, e2e, shortlist, per_video, iou):
        vix, model, loss, text, F = e2e["vix"], e2e["model"], e2e["loss"], e2e["text"], e2e["F"]
        k = 5 if per_video == 1 else 9
        model.train()
        got = vix.search_moments(model, loss, text, k=k, frames=F, windows=(2, 4), stride=1, per_video=per_video, iou=iou, shortlist=shortlist)
        assert model.training                                                # the training flag is restored
        model.eval()
        assert got["ids"].shape == (6, k) and (got["ids"] >= 0).all() and torch.isfinite(got["scores"]).all()
        assert (got["scores"][:, :-1] >= got["scores"][:, 1:]).all()
        _same_hits(got, _composed(vix, model, loss, text, k, F, (2, 4), 1, per_video, iou, shortlist))

    def test_holes_of_a_filter_and_of_a_removal(self, e2e):
        model, loss, text, F, N = e2e["model"], e2e["loss"], e2e["text"], e2e["F"], e2e["N"]
        vix = search.VideoIndex(N, e2e["vix"].G, torch.bfloat16, DEV, tiled=True).load_state_dict(e2e["vix"].state_dict())      # (remove changes the index)
        allow = torch.zeros(N, dtype=torch.bool, device=DEV)
        allow[[2, 7, 9]] = True
        kw = dict(k=8, frames=F, windows=(2, 4), stride=1, per_video=2, iou=0.5)
        for shortlist in (6, None):
            got = vix.search_moments(model, loss, text, shortlist=shortlist, allow=allow, **kw)      # 3 videos x 2 hits < k = 8
            assert (got["ids"][:, :6] >= 0).all() and torch.isin(got["ids"][:, :6], torch.tensor([2, 7, 9], device=DEV)).all()
            for name in ("ids", "start", "length"):
                assert (got[name][:, 6:] == -1).all(), name
            assert torch.isneginf(got["scores"][:, 6:]).all() and torch.isfinite(got["scores"][:, :6]).all()
            _same_hits(got, _composed(vix, model, loss, text, 8, F, (2, 4), 1, 2, 0.5, shortlist, allow))
        vix.remove([7])
        for shortlist in (6, None):
            got = vix.search_moments(model, loss, text, shortlist=shortlist, allow=allow, **kw)
            assert not (got["ids"] == 7).any() and (got["ids"][:, :4] >= 0).all() and (got["ids"][:, 4:] == -1).all()
            assert (got["start"][:, 4:] == -1).all() and (got["length"][:, 4:] == -1).all() and torch.isneginf(got["scores"][:, 4:]).all()
            _same_hits(got, _composed(vix, model, loss, text, 8, F, (2, 4), 1, 2, 0.5, shortlist, allow))
        got = vix.search_moments(model, loss, text, shortlist=None, **{**kw, "k": 24})               # no filter: 11 live videos x 2 hits, then padding
        assert not (got["ids"] == 7).any() and (got["ids"][:, :22] >= 0).all() and (got["ids"][:, 22:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# a planted moment: videos of 16 frames x 4 regions put into the index as embeddings; video 3 carries the words of query 0 in the frames
# [2, 6) (exact copies) and [10, 14) (copies under noise); every other frame of every video is noise, and all videos share one global
# embedding, so the cosine is the same for all and the ranking is the windows'.
# ---------------------------------------------------------------------------------------------------------------------------------------
PF, PR, F0, F1, WIN, PLANTED = 16, 4, 2, 10, 4, 3


@pytest.fixture(scope="module")
def planted(e2e):
    model, text = e2e["model"], e2e["text"]
    with torch.no_grad():
        _, lt = model.compute_text(text)
    words = lt[0][text["attention_mask"][0, 1:] > 0].float()                  # the unpadded words of query 0
    words = words / words.norm(dim=1, keepdim=True)
    gen = torch.Generator(device="cpu").manual_seed(5)
    N, G = 6, PF * PR
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    local = unit(torch.randn(N, G, 256, generator=gen)).to(DEV)
    copies = words[torch.arange(WIN * PR, device=DEV) % words.shape[0]]
    local[PLANTED, F0 * PR:(F0 + WIN) * PR] = copies
    local[PLANTED, F1 * PR:(F1 + WIN) * PR] = copies + 0.3 * local[PLANTED, F1 * PR:(F1 + WIN) * PR]
    ix = search.VideoIndex(N, G, torch.bfloat16, DEV, tiled=True)
    ix.add(dict(global_object_embeddings=torch.ones(N, 256, device=DEV, dtype=torch.bfloat16), local_object_embeddings=local.bfloat16(),
                object_mask=torch.zeros(N, G, device=DEV)))
    return ix


class TestPlantedMoment:
    def test_the_planted_window_is_the_first_hit(self, e2e, planted):
        model, loss, text = e2e["model"], e2e["loss"], e2e["text"]
        got = planted.search_moments(model, loss, text, k=3, frames=PF, windows=(WIN,), stride=1, per_video=1, iou=0.5, shortlist=None)
        assert (int(got["ids"][0, 0]), int(got["start"][0, 0]), int(got["length"][0, 0])) == (PLANTED, F0, WIN)
        assert float(got["scores"][0, 0]) > float(got["scores"][0, 1])
        assert len(set(got["ids"][0].tolist())) == 3                          # per_video = 1: one hit per video

    def test_a_second_occurrence_in_the_same_video_is_its_second_hit(self, e2e, planted):
        model, loss, text = e2e["model"], e2e["loss"], e2e["text"]
        iou = 0.25
        got = planted.search_moments(model, loss, text, k=4, frames=PF, windows=(WIN,), stride=1, per_video=2, iou=iou, shortlist=None)
        hits = [(int(i), int(s), int(l)) for i, s, l in zip(got["ids"][0], got["start"][0], got["length"][0])]
        assert hits[0] == (PLANTED, F0, WIN) and hits[1] == (PLANTED, F1, WIN), hits
        mine = [(s, l) for i, s, l in hits if i == PLANTED]
        assert len(mine) == 2
        inter, union = overlap(np.array([mine[0][0], mine[1][0]]), np.array([mine[0][1], mine[1][1]]), 0)
        assert not suppresses(inter, union, iou)[1]
