"""Text-to-video search (not in the reference, whose every use of the trained model ends in a metric): hand the model a sentence, get back
the best videos of a collection.

``VideoIndex`` keeps the collection prepared on the device: the normalised global embeddings, the object masks and the video side of the
fused local-similarity kernel exactly as that kernel reads it (``dvlp_xattn_index_add``: ~296 KB per video at G = 288), so a query never
touches the object tower or re-prepares a video.  ``VideoIndex.search`` is two stages:

  global   cosine of every query against every video -- one exact-fp32 ``dvlp_gemm`` per index chunk -- reduced on the device to the
           ``shortlist`` best videos per query by ``dvlp_topk_rows`` (merged over the chunks);
  local    the (region x word) similarity of each query against its shortlisted videos only (``dvlp_xattn_index_pairs_fwd``: the per-pair
           code of the full-grid kernel, bit-equal to its entries), added to the cosine, and a last ``dvlp_topk_rows`` for the ``k`` best.

``VideoIndex.ground`` / ``search(..., ground=True)`` say where a result matched: for the k winners one more launch
(``dvlp_xattn_index_pairs_ground``, the pair kernel's own arithmetic) returns the per-word and per-region cosines the local score is the
mean of, each word's strongest region (and frame) with its attention weight, each region's strongest word and per-frame means.  Fused route
only.

Orientation.  The score of (caption j, video i) is ``cos(text_j, video_i) + local(video_i, caption_j)``.  ``trainer.evaluate`` reproduces
the reference's quirk of adding the global [text, video] and local [video, text] matrices element-wise without a transpose
(trainer/trainer_dist.py:369-399); search does not.  In ``evaluate``'s terms the search score is ``global_sims + local_sims.T``, and metrics
computed from search results (``evaluate_t2v``) are NOT comparable with the reference's evaluation numbers.

fp32 models, and region counts beyond the fused kernel's range (G > 288), take the parity route: the raw local embeddings are kept and each
query's shortlist is gathered and scored by the multi-kernel ``RWALoss.get_sim`` -- slow and exact, as fp32 is everywhere in this package.
"""
from __future__ import annotations

import numpy as np
import torch

from . import functional as Fn
from . import ops
from ._lib import DemoVLPHipError, call

_DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, torch.float32: torch.float32, torch.bfloat16: torch.bfloat16}
TOPK_MAX = 1024               # dvlp_topk_rows: 1 <= K <= 1024
QUERY_BLOCK = 1024            # queries per pass of the pipeline (bounds the text tower's and the pair kernel's scratch)


class VideoIndex:
    """A collection of videos prepared for search.  ``capacity`` videos of ``G`` regions (frames x regions per frame) in the model's compute
    ``dtype``; device memory is allocated at the first ``add``."""

    def __init__(self, capacity, G, dtype=torch.bfloat16, device="cuda"):
        if int(capacity) < 1 or int(G) < 1:
            raise ValueError(f"capacity and G must be positive, got {capacity} and {G}")
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be float32 or bfloat16, got {dtype!r}")
        self.capacity, self.G, self.dtype, self.device = int(capacity), int(G), _DTYPES[dtype], torch.device(device)
        self.n = 0
        # fused route: bf16 within the fused kernel's range (host arithmetic; a negative size is "not supported")
        self.fused = self.dtype == torch.bfloat16 and call("dvlp_xattn_index_bytes", self.capacity, self.G) > 0
        self.gn = self.om = self.local = None

    def __len__(self):
        return self.n

    def _alloc(self):
        if self.gn is not None:
            return
        if self.device.type != "cuda":
            raise DemoVLPHipError("VideoIndex lives on an MI355X device only (no CPU fallback)")
        dev = self.device
        self.gn = torch.zeros((self.capacity, 256), device=dev, dtype=torch.float32)
        self.om = torch.zeros((self.capacity, self.G), device=dev, dtype=torch.float32)
        if self.fused:      # zeroed: the alignment gaps between its sections are never written, and the buffer is compared / saved as bytes
            self.local = torch.zeros(ops.xattn_index_bytes(self.capacity, self.G), device=dev, dtype=torch.uint8)
        else:
            self.local = torch.zeros((self.capacity, self.G, 256), device=dev, dtype=self.dtype)

    # ---- filling ------------------------------------------------------------------------------------------------------
    def add(self, out):
        """Append the videos of ``out``, the dict ``ObjectRelation.forward(..., return_embeds=True)`` returns (its ``global_object_embeddings``
        [n, 256], ``local_object_embeddings`` [n, G, 256] and ``object_mask`` [n, G] are read).  Returns the index rows they took."""
        go, lo, om = out["global_object_embeddings"], out["local_object_embeddings"], out["object_mask"]
        n = go.shape[0]
        if lo.dim() != 3 or lo.shape[1] != self.G or lo.shape[2] != 256:
            raise ValueError(f"this index holds videos of G = {self.G} regions: expected local embeddings [n, {self.G}, 256], got {tuple(lo.shape)}")
        if tuple(go.shape) != (n, 256) or lo.shape[0] != n or tuple(om.shape) != (n, self.G):
            raise ValueError(f"expected [n, 256], [n, {self.G}, 256], [n, {self.G}], got {tuple(go.shape)}, {tuple(lo.shape)}, {tuple(om.shape)}")
        if lo.dtype != self.dtype:
            raise ValueError(f"this index holds {self.dtype} embeddings, got {lo.dtype}")
        if self.n + n > self.capacity:
            raise ValueError(f"adding {n} videos to {self.n} exceeds the capacity {self.capacity}")
        if not (go.is_cuda and lo.is_cuda and om.is_cuda):
            raise DemoVLPHipError("VideoIndex lives on an MI355X device only (no CPU fallback): embeddings must be on the device")
        self._alloc()
        r0 = self.n
        with torch.no_grad():
            self.gn[r0:r0 + n] = ops.rownorm_fwd(go.detach().contiguous())[0]
            self.om[r0:r0 + n] = om.detach().float()
            if self.fused:
                ops.xattn_index_add(self.local, self.capacity, self.G, r0, lo.detach().contiguous())
            else:
                self.local[r0:r0 + n] = lo.detach()
        self.n += n
        return range(r0, r0 + n)

    def add_batches(self, model, batches):
        """Run the object tower only (``model.compute_object``) on every batch ``{'object', 'object_mask', ...}`` and add its videos."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                for data in batches:
                    go, lo, add_mask = model.compute_object(data["object"], data["object_mask"])
                    self.add(dict(global_object_embeddings=go, local_object_embeddings=lo, object_mask=add_mask[:, 1:, ...]))
        finally:
            if was_training:
                model.train()
        return self

    # ---- persistence --------------------------------------------------------------------------------------------------
    def state_dict(self):
        self._alloc()
        return dict(capacity=self.capacity, G=self.G, dtype=str(self.dtype).replace("torch.", ""), n=self.n, fused=self.fused,
                    gn=self.gn.cpu(), om=self.om.cpu(), local=self.local.cpu())

    def load_state_dict(self, state):
        if (state["capacity"], state["G"], _DTYPES[state["dtype"]], bool(state["fused"])) != (self.capacity, self.G, self.dtype, self.fused):
            raise ValueError("state_dict belongs to an index of another capacity / G / dtype")
        self._alloc()
        for name in ("gn", "om", "local"):
            getattr(self, name).copy_(state[name])
        self.n = int(state["n"])
        return self

    # ---- search -------------------------------------------------------------------------------------------------------
    def _shortlist_size(self, shortlist):
        return self.n if shortlist is None or shortlist >= self.n else int(shortlist)

    def shortlist_by_cosine(self, global_text_embeddings, shortlist, chunk=65536):
        """The global stage alone: (ids int64 [Nq, S] ascending per row, cosines fp32 [Nq, S]) of the ``shortlist`` best videos per query
        embedding [Nq, 256] by cosine (ties by smaller id)."""
        if not global_text_embeddings.is_cuda or self.n == 0:
            raise DemoVLPHipError("shortlist_by_cosine needs a filled index and embeddings on an MI355X device")
        with torch.no_grad():
            ids, cos = self._global_stage(ops.rownorm_fwd(global_text_embeddings.detach().contiguous())[0], self._shortlist_size(shortlist), int(chunk))
        return ids.long(), cos

    def _global_stage(self, qn, S, chunk):
        """-> (ids int32 [Nq, S] ascending per row, cosines fp32 [Nq, S]) of the S best videos per query by cosine."""
        Nq, dev = qn.shape[0], qn.device
        if S == self.n:                                            # every video: nothing to select
            cos = torch.empty((Nq, self.n), device=dev, dtype=torch.float32)
            for c0 in range(0, self.n, chunk):
                cn = min(chunk, self.n - c0)
                ops.gemm(qn, self.gn[c0:], Nq, cn, 256, dtype=ops.F32, out=cos[:, c0:], ldc=self.n)
            return torch.arange(self.n, device=dev, dtype=torch.int32).expand(Nq, -1).contiguous(), cos
        out = (torch.empty((Nq, S), device=dev, dtype=torch.float32), torch.empty((Nq, S), device=dev, dtype=torch.int32))
        for c0 in range(0, self.n, chunk):
            cn = min(chunk, self.n - c0)
            sims = ops.gemm(qn, self.gn[c0:], Nq, cn, 256, dtype=ops.F32)
            ops.topk_rows(sims, S, index_base=c0, out=out, merge=c0 > 0)
        # by id: the final cut breaks score ties by position in the shortlist, which must then mean "smaller id first"
        ids, order = torch.sort(out[1], dim=1)
        return ids.contiguous(), torch.gather(out[0], 1, order).contiguous()

    def _local_stage(self, local_loss, lt, text_mask, ids):
        lam, gate = float(local_loss.lambda_softmax), local_loss.focal_type == "equal"
        if self.fused:
            return Fn.XattnIndexPairsFn.apply(self.local, self.capacity, self.G, self.om, lt, text_mask, ids, lam, gate)
        out = torch.empty(ids.shape, device=ids.device, dtype=torch.float32)
        for j in range(ids.shape[0]):                              # parity route: the query's videos gathered, multi-kernel grid [S, 1]
            rows = ids[j].long()
            out[j] = local_loss.get_sim(self.local[rows], lt[j:j + 1], self.om[rows], None, text_mask[j:j + 1])[:, 0]
        return out

    def _text_side(self, model, text):
        """One block of queries through the text tower -> (global [Nq, 256], local [Nq, W, 256], additive word mask [Nq, W])."""
        att = text["attention_mask"]
        text_mask = (att[:, 1:].contiguous() - 1.0) * 100.0        # as trainer.evaluate (trainer/trainer_dist.py:156-159)
        gt, lt = model.compute_text(text)
        if lt.dtype != self.dtype:
            raise ValueError(f"this index holds {self.dtype} embeddings, the model computes {lt.dtype}")
        if self.fused and call("dvlp_xattn_index_query_workspace_bytes", lt.shape[0], lt.shape[1]) < 0:
            raise DemoVLPHipError(f"captions of {lt.shape[1]} words are beyond the fused kernel's range (W <= 112)")
        return gt, lt.contiguous(), text_mask

    def _score(self, model, loss_fn, text, S, chunk, side=None):
        """One block of queries through the text tower (or its outputs ``side``) and both stages -> (qn, ids int32 [Nq, S], cos, local)."""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        gt, lt, text_mask = side if side is not None else self._text_side(model, text)
        qn = ops.rownorm_fwd(gt.contiguous())[0]
        ids, cos = self._global_stage(qn, S, chunk)
        return qn, ids, cos, self._local_stage(local_loss, lt, text_mask, ids)

    def _ground_block(self, loss_fn, side, att, ids, frames):
        """Grounding of one block's pairs (query j, index row ids[j, p]) from its text-tower outputs."""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        _, lt, text_mask = side
        out = ops.xattn_index_pairs_ground(self.local, self.capacity, self.G, self.om, lt, text_mask, ids.to(torch.int32).contiguous(),
                                           float(local_loss.lambda_softmax), local_loss.focal_type == "equal", frames)
        out["word_valid"] = att[:, 1:] > 0
        if frames is not None:
            out["word_frame"] = torch.div(out["word_region"], self.G // int(frames), rounding_mode="floor")
        return out

    def _ground_checks(self, frames):
        if not self.fused:
            raise DemoVLPHipError("grounding needs the fused route (a bf16 index with G <= 288, captions of W <= 112 words): this index is "
                                  f"{self.dtype} with G = {self.G}; there is no fp32 / long-video grounding")
        if frames is not None and (int(frames) < 1 or self.G % int(frames) != 0):
            raise ValueError(f"frames = {frames} must be a positive divisor of G = {self.G}")

    def ground(self, model, loss_fn, text, ids, frames=None):
        """Where the local similarity of (query j, index row ``ids[j, p]``) comes from; ``ids`` int [Nq, k], typically what ``search``
        returned.  -> a dict on the device (``ops.xattn_index_pairs_ground``): ``score`` [Nq, k] (the local addend of the search score, bit
        for bit), ``word_scores`` / ``word_region`` / ``word_region_weight`` [Nq, k, W], ``region_scores`` / ``region_word`` [Nq, k, G],
        ``word_valid`` bool [Nq, W] (words of the query that are not padding) and, with ``frames`` (a divisor of G: regions are frame-major),
        ``frame_scores`` [Nq, k, frames] and ``word_frame`` = ``word_region // (G // frames)``.  Fused route only; no gradient flows."""
        self._ground_checks(frames)
        ids_in = text["input_ids"]
        if not (ids_in.is_cuda and ids.is_cuda):
            raise DemoVLPHipError("VideoIndex.ground runs on an MI355X device only (no CPU fallback): move the queries and ids to cuda")
        if ids.dim() != 2 or ids.shape[0] != ids_in.shape[0] or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"ids must be int [Nq = {ids_in.shape[0]}, k], got {ids.dtype} {tuple(ids.shape)}")
        if self.n == 0:
            raise ValueError("the index is empty")
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for q0 in range(0, ids_in.shape[0], QUERY_BLOCK):
                    block = {name: t[q0:q0 + QUERY_BLOCK] for name, t in text.items() if isinstance(t, torch.Tensor)}
                    res.append(self._ground_block(loss_fn, self._text_side(model, block), block["attention_mask"], ids[q0:q0 + QUERY_BLOCK], frames))
        finally:
            if was_training:
                model.train()
        return {name: torch.cat([r[name] for r in res]) for name in res[0]}

    def search(self, model, loss_fn, text, k=10, shortlist=100, chunk=65536, ground=False, frames=None):
        """The ``k`` best videos for every query of ``text`` (``{'input_ids', 'attention_mask'}`` [Nq, L] on the device) ->
        ``(ids int64 [Nq, k], scores fp32 [Nq, k])`` on the device, best first, equal scores by smaller id; ids are index rows.
        With ``ground=True``: ``(ids, scores, grounding)``, the dict of ``VideoIndex.ground`` for the k winners (one more launch over them,
        on the text-tower outputs the search used; ``frames`` as there).

        ``loss_fn`` supplies ``lambda_softmax`` / ``focal_type`` (a ``GlobalLocalLoss`` or its ``RWALoss``).  ``shortlist``: videos per query
        that reach the local stage, chosen by cosine (at most 1024); ``None`` or ``>= len(index)`` scores every video (exact search).
        ``chunk``: index rows per global-stage product.  The score is ``cos(text_j, video_i) + local(video_i, caption_j)``: in
        ``trainer.evaluate``'s terms ``global_sims + local_sims.T``, NOT its ``o2t_sims`` (which keeps the reference's transposed-addend
        quirk), so metrics of search results are not comparable with the reference's evaluation numbers.  No gradient flows."""
        k, chunk = int(k), int(chunk)
        if self.n == 0:
            raise ValueError("the index is empty")
        S = self._shortlist_size(shortlist)
        if k < 1 or k > S:
            raise ValueError(f"k = {k} must lie in [1, shortlist = {S}]")
        if k > TOPK_MAX or (S < self.n and S > TOPK_MAX):
            raise ValueError(f"k and a partial shortlist are limited to {TOPK_MAX} (dvlp_topk_rows)")
        if chunk < 1:
            raise ValueError(f"chunk must be positive, got {chunk}")
        if ground:
            self._ground_checks(frames)
        ids_in = text["input_ids"]
        if not ids_in.is_cuda:
            raise DemoVLPHipError("VideoIndex.search runs on an MI355X device only (no CPU fallback): move the queries to cuda")
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for q0 in range(0, ids_in.shape[0], QUERY_BLOCK):
                    block = {name: t[q0:q0 + QUERY_BLOCK] for name, t in text.items() if isinstance(t, torch.Tensor)}
                    side = self._text_side(model, block)
                    _, ids, cos, local = self._score(model, loss_fn, block, S, chunk, side)
                    val, pos = ops.topk_rows(cos + local, k)
                    top = torch.gather(ids, 1, pos.long()).long()
                    res.append((top, val, self._ground_block(loss_fn, side, block["attention_mask"], top, frames) if ground else None))
        finally:
            if was_training:
                model.train()
        ids, scores = torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res])
        if not ground:
            return ids, scores
        return ids, scores, {name: torch.cat([r[2][name] for r in res]) for name in res[0][2]}


def two_stage_sims(global_sims, ids, scores):
    """Search results as a matrix ``metric.t2v_metrics`` accepts (host, numpy): [Nq, N] holding ``scores[q, s]`` at column ``ids[q, s]`` and
    ``global_sims - C`` elsewhere, C large enough that every video outside a query's shortlist ranks behind all of its shortlist, in global
    order -- what a two-stage search returns when asked for more than it re-ranked.  ids < 0 (fillers) are skipped."""
    g = np.asarray(global_sims, dtype=np.float64)
    ids, scores = np.asarray(ids), np.asarray(scores, dtype=np.float64)
    if g.ndim != 2 or ids.shape != scores.shape or ids.ndim != 2 or ids.shape[0] != g.shape[0]:
        raise ValueError(f"expected global_sims [Nq, N] and ids / scores [Nq, S], got {g.shape}, {ids.shape}, {scores.shape}")
    if ids.size and ids.max() >= g.shape[1]:
        raise ValueError(f"ids must be below N = {g.shape[1]}, got {ids.max()}")
    ok = ids >= 0
    finite = scores[ok & np.isfinite(scores)]
    C = (g.max() - (finite.min() if finite.size else 0.0)) + 1.0 if g.size else 0.0
    sims = g - max(C, 1.0)
    rows = np.broadcast_to(np.arange(ids.shape[0])[:, None], ids.shape)
    sims[rows[ok], ids[ok]] = scores[ok]
    return sims


def evaluate_t2v(model, loss_fn, batches, shortlist=None, chunk=65536):
    """Text-to-video metrics of two-stage search on one loader (a re-iterable of tokenised batches ``{'text', 'object', 'object_mask'}``, query
    b of a batch belonging to its video b): every video goes into one ``VideoIndex``, every caption is searched with ``shortlist``, and
    ``metric.t2v_metrics`` is taken of ``two_stage_sims``.  Comparing ``shortlist=None`` with a partial one measures what the shortlist
    costs in recall.  Search orientation (see the module docstring): not comparable with ``trainer.evaluate``.
    -> ``{'t2v_metrics': dict, 'sims': numpy [N, N]}``."""
    from . import metric as M
    batches = list(batches)
    N = sum(int(b["object"].shape[0]) for b in batches)
    obj = batches[0]["object"]
    index = VideoIndex(N, int(obj.shape[1] * obj.shape[2]), model.compute_dtype, obj.device).add_batches(model, batches)
    S = index._shortlist_size(shortlist)
    if S < N and S > TOPK_MAX:
        raise ValueError(f"a partial shortlist is limited to {TOPK_MAX} (dvlp_topk_rows)")
    was_training = model.training
    model.eval()
    g, ids, scores = [], [], []
    try:
        with torch.no_grad():
            for data in batches:
                qn, i, cos, local = index._score(model, loss_fn, data["text"], S, int(chunk))
                g.append(ops.gemm(qn, index.gn, qn.shape[0], N, 256, dtype=ops.F32).cpu().numpy())
                ids.append(i.cpu().numpy())
                scores.append((cos + local).cpu().numpy())
    finally:
        if was_training:
            model.train()
    sims = two_stage_sims(np.concatenate(g), np.concatenate(ids), np.concatenate(scores))
    return dict(t2v_metrics=M.t2v_metrics(sims), sims=sims)
