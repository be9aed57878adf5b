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

Video-to-text search is the same pipeline with the roles swapped.  ``CaptionIndex`` keeps a collection of captions (tags, descriptions)
resident -- normalised global text embeddings, additive word masks and the caption side of the fused kernel (``dvlp_xattn_caption_index_add``:
123 392 bytes per caption at W = 99) -- and ``CaptionIndex.search`` answers "which captions fit this clip": object tower, cosine shortlist,
``dvlp_xattn_caption_index_pairs_fwd`` over the shortlist, final top-k; ``CaptionIndex.ground`` grounds the winners.  The pair score is the
one above, ``cos(video_i, text_j) + local(video_i, caption_j)``, so an exact v2t search is the transpose of an exact t2v search: in
``evaluate``'s terms ``global_sims.T + local_sims``, again not the quirk matrix, and ``evaluate_v2t`` is no more comparable with the
reference's numbers than ``evaluate_t2v``.

Long videos.  The fused kernel keeps both attention matrices of a pair on chip, which stops it at G = 288 regions (8 frames x 36).
``VideoIndex(..., tiled=True)`` (bf16, G <= 1152: 32 frames x 36) keeps the same resident layout (~1.18 MB per video at G = 1152) and runs
the local stage and the grounding on the region-tiled pair kernel (``dvlp_xattn_long_index_pairs_fwd`` / ``_pairs_ground``: two sweeps over
128-region tiles); ``search``, ``ground``, ``search(ground=True, frames=F)`` and the state dict work as above.  Its scores
agree with the fused kernel's to rounding (2e-3), not bit for bit.  ``CaptionIndex(..., tiled=True)`` (bf16, W <= 112) is the same route for
long QUERY videos: the resident caption side is byte for byte that of a fused index, and the local stage and the grounding run the tiled
pair kernel on the video-major grid (``dvlp_xattn_long_caption_index_pairs_fwd`` / ``_pairs_ground``), bit-equal per pair to
``VideoIndex(..., tiled=True)``.

Moments.  ``VideoIndex.moments`` / ``search(..., frames=F, moments=(4, 8))`` say WHEN a long video matched: every window of that many
consecutive frames of a result is scored as a video of its own -- the local similarity of its regions alone, not a mean of whole-video
cosines -- by ``dvlp_xattn_long_index_moments_fwd``, which reads the window out of the resident index in place (one launch
per window length over all windows of all pairs), and the best window per result is picked on the device.  ``tiled=True`` indexes only.
``CaptionIndex.moments`` / ``search(..., frames=F, moments=(4, 8))`` are the same question for a long QUERY video against resident
captions -- the same windows, the same scores bit for bit -- on ``dvlp_xattn_long_caption_index_moments_fwd``, where a
workgroup stages its caption once and walks the windows of its pair.  ``CaptionIndex.timeline`` turns it round: for every window of a query
video the ``k`` best captions of the video's shortlist by that window's local similarity (the kernel's window-major output, one
``dvlp_topk_rows`` over all windows) -- which captions apply when.

Moment retrieval.  The second best window of a pair is almost always the best one shifted by a frame, so ranking windows
needs a selection that knows they overlap in time: ``dvlp_moment_select``, greedy temporal non-maximum suppression per pair on the device
(best first in the order of ``dvlp_topk_rows``; a pick kills every window whose intersection over union with it exceeds ``iou``).
``moments(..., top=m, iou=0.5)`` / ``search(..., moment_top=m)`` report up to ``m`` such windows per result -- a second occurrence in the
same video -- and ``VideoIndex.search_moments`` answers "where, in which video, does this happen": every window of every shortlisted
video is scored, up to ``per_video`` windows per video survive the suppression, and the hits ``cos(text, video) + local(window)`` of all
videos are ranked together, so a long video with one matching window is not diluted by its other frames.

fp32 models, and region counts beyond the fused kernel's range (G > 288) without ``tiled=True``, take the parity route: the raw local
embeddings are kept and each query's shortlist is gathered and scored by the multi-kernel ``RWALoss.get_sim`` -- slow and exact, as fp32 is
everywhere in this package.

Filters and removal.  ``search`` / ``shortlist_by_cosine`` / ``timeline`` take ``allow``, a bool tensor over the index rows
(one for all queries or one per query): the global stage runs ``dvlp_topk_rows_masked``, which never lists a disallowed row, so the cut to
``shortlist`` is made among the allowed rows -- filtering a larger result on the host would cut first and could leave nothing.  A query
with fewer allowed rows than asked for is padded with id -1, the hole every later stage already knows (the pair kernels score it NaN, the
final top-k sorts it last) and comes back as (-1, -inf).  ``index.remove(ids)`` clears the rows' bits in a resident ``alive`` mask (one bit
per row, allocated at the first removal, ANDed into every filter) and zeroes their global embeddings; rows keep their numbers.
``index.replace(rows, ...)`` overwrites rows in place through the ``*_index_add`` entries and revives them; ``index.live`` and
``index.removed()`` count and list.  Compaction (renumbering rows) is not offered.
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
VIDEO_BLOCK = 256             # query videos per pass of CaptionIndex's pipeline (the object tower runs G + 1 tokens per video, not 100)


def moment_windows(frames, windows, stride=1):
    """The windows ``VideoIndex.moments`` scores, on the host: (starts, lengths), int64 tensors [M_total] in frames.  ``windows``: a window
    length or a sequence of them; lengths come in the order given, starts 0, ``stride``, 2 ``stride``, ... ascending within a length
    (``dvlp_xattn_long_index_moments_count`` windows each).  ValueError for what that entry refuses: a length outside [1, frames],
    ``stride < 1``, no length at all."""
    frames, stride = int(frames), int(stride)
    lengths = [int(windows)] if isinstance(windows, (int, np.integer)) else [int(w) for w in windows]
    if frames < 1 or stride < 1 or not lengths:
        raise ValueError(f"frames and stride must be positive and windows not empty, got frames = {frames}, stride = {stride}, windows = {windows!r}")
    starts, lens = [], []
    for win in lengths:
        M = call("dvlp_xattn_long_index_moments_count", frames, frames, win, stride)       # (G = frames: one region per frame)
        if M < 0:
            raise ValueError(f"a window of {win} frames does not fit a video of {frames} frames (1 <= window <= frames)")
        starts += [m * stride for m in range(M)]
        lens += [win] * M
    return torch.tensor(starts, dtype=torch.int64), torch.tensor(lens, dtype=torch.int64)


class _ResidentIndex:
    """What both directions share: the row count, the search-argument checks and the global (cosine) stage over ``self.gn`` [capacity, 256],
    the normalised global embeddings of the ``self.n`` resident rows."""

    alive = None              # uint32 words [ceil(capacity / 32)], bit r = row r is live; allocated by the first ``remove`` (None: nothing was ever removed)

    def __len__(self):
        return self.n

    # ---- filters and removal ------------------------------------------------------------------------------------------------
    def _filter(self, allow, Nq):
        """The packed allow mask of one call -> uint32 words [words] (every query) or [Nq, words] (per query), or None when no row is
        left out: ``allow`` (bool [len(index)] or [Nq, len(index)] on the index's device, or None) ANDed with the live rows."""
        if allow is None:
            return self.alive
        if not isinstance(allow, torch.Tensor) or allow.dtype != torch.bool or tuple(allow.shape) not in ((self.n,), (Nq, self.n)) \
                or allow.device.type != self.device.type:
            got = f"{allow.dtype} {tuple(allow.shape)} on {allow.device}" if isinstance(allow, torch.Tensor) else repr(type(allow))
            raise ValueError(f"allow must be a bool tensor [{self.n}] (every query) or [{Nq}, {self.n}] (per query) on {self.device.type}: one entry "
                             f"per index row; got {got}")
        words = ops.pack_allow_bits(allow)
        if self.alive is not None:
            words = (words.view(torch.int32) & self.alive.view(torch.int32)[:words.shape[-1]]).view(torch.uint32)
        return words

    @staticmethod
    def _rows_of(mask, q0, q1):
        return mask if mask is None or mask.dim() == 1 else mask[q0:q1]

    @classmethod
    def _mask_arg(cls, mask, q0, q1):
        """the ``mask`` keyword of ``_score`` for the queries [q0, q1); no keyword at all without a mask: that call is what it was"""
        return {} if mask is None else {"mask": cls._rows_of(mask, q0, q1)}

    def _row_list(self, rows, what):
        """-> the rows of a ``remove`` / ``replace`` call as a list of ints, or the ValueError that names the one outside [0, len(index))"""
        rows = [int(r) for r in (rows.tolist() if isinstance(rows, torch.Tensor) else rows)]
        bad = [r for r in rows if r < 0 or r >= self.n]
        if bad:
            raise ValueError(f"{what}: row {bad[0]} is outside [0, len(index) = {self.n})")
        return rows

    def _set_alive(self, rows, on):
        if self.alive is None:
            if on:
                return
            full = torch.ones(self.capacity, device=self.gn.device, dtype=torch.bool)      # rows not yet in use are live: ``add`` needs no mask
        else:
            full = _unpack_bits(self.alive, self.capacity)
        full[torch.tensor(rows, device=full.device, dtype=torch.int64)] = bool(on)
        self.alive = ops.pack_allow_bits(full)

    def remove(self, ids):
        """Take the rows ``ids`` (ints in [0, len(index)); a list or a tensor) out of every later result: ``search``, ``shortlist_by_cosine``
        and ``timeline`` never list them, ``ground`` / ``moments`` answer for them as for a hole (id -1).  Rows keep their numbers and
        ``len(index)`` its value; a removed row's bytes stay where they are (``replace`` reuses the slot) but its global embedding is
        zeroed, so a saved index does not carry it.  Removing a row twice is a no-op; an id outside the index is a ``ValueError``."""
        rows = self._row_list(ids, "remove")
        if not rows:
            return self
        with torch.no_grad():
            self._set_alive(rows, False)
            self.gn[torch.tensor(rows, device=self.gn.device, dtype=torch.int64)] = 0.0
        return self

    def removed(self):
        """The removed rows, int64 ascending, on the index's device: the slots ``replace`` can reuse."""
        if self.alive is None:
            return torch.empty(0, device=self.device, dtype=torch.int64)
        return torch.nonzero(~_unpack_bits(self.alive, self.n))[:, 0]

    @property
    def live(self):
        """rows in use that were not removed (``len(index)`` counts the removed ones too)"""
        return self.n - int(self.removed().numel())

    def _live_ids(self, ids):
        """explicit ids of ``ground`` / ``moments``: a removed row becomes -1, the hole every pair kernel answers NaN for"""
        if self.alive is None:
            return ids
        inside = (ids >= 0) & (ids < self.capacity)
        live = _unpack_bits(self.alive, self.capacity)[ids.long().clamp(0, self.capacity - 1)]
        return torch.where(inside & ~live, torch.full_like(ids, -1), ids)

    def _shortlist_size(self, shortlist):
        return self.n if shortlist is None or shortlist >= self.n else int(shortlist)

    def _search_checks(self, k, shortlist, chunk):
        """-> (k, S, chunk) of a search call, or the ValueError that names what is wrong with them"""
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
        return k, S, chunk

    def _global_stage(self, qn, S, chunk, mask=None):
        """-> (ids int32 [Nq, S] ascending per row, cosines fp32 [Nq, S]) of the S best index rows per query by cosine.  ``mask`` (``_filter``):
        the S best ALLOWED rows (``dvlp_topk_rows_masked``: a disallowed row is never scored against the cut); a query with fewer than S
        of them is padded with id -1 (cosine -inf; in the exact branch S == n the cosine of a left-out row stays, its id is -1), the hole
        the later stages score NaN."""
        Nq, dev = qn.shape[0], qn.device
        if S == self.n:                                            # every row: nothing to select
            cos = torch.empty((Nq, self.n), device=dev, dtype=torch.float32)
            for c0 in range(0, self.n, chunk):
                cn = min(chunk, self.n - c0)
                ops.gemm(qn, self.gn[c0:], Nq, cn, 256, dtype=ops.F32, out=cos[:, c0:], ldc=self.n)
            ids = torch.arange(self.n, device=dev, dtype=torch.int32).expand(Nq, -1)
            if mask is not None:
                ids = torch.where(_unpack_bits(mask, self.n).expand(Nq, -1), ids, torch.full_like(ids, -1))
            return ids.contiguous(), cos
        out = (torch.empty((Nq, S), device=dev, dtype=torch.float32), torch.empty((Nq, S), device=dev, dtype=torch.int32))
        for c0 in range(0, self.n, chunk):
            cn = min(chunk, self.n - c0)
            sims = ops.gemm(qn, self.gn[c0:], Nq, cn, 256, dtype=ops.F32)
            if mask is None:
                ops.topk_rows(sims, S, index_base=c0, out=out, merge=c0 > 0)
            else:
                ops.topk_rows_masked(sims, S, mask, index_base=c0, out=out, merge=c0 > 0)
        # by id: the final cut breaks score ties by position in the shortlist, which must then mean "smaller id first"
        ids, order = torch.sort(out[1], dim=1)
        return ids.contiguous(), torch.gather(out[0], 1, order).contiguous()


def _unpack_bits(words, n):
    """uint32 words [..., >= ceil(n / 32)] (``ops.pack_allow_bits``) -> bool [..., n]"""
    c = torch.arange(n, device=words.device, dtype=torch.int64)
    return ((words.view(torch.int32)[..., c >> 5] >> (c & 31).to(torch.int32)) & 1).bool()


def _holes(top, val):
    """the final cut of a filtered search: a hole (id -1, NaN score, sorted last) reads (-1, -inf)"""
    return torch.where(top < 0, torch.full_like(val, float("-inf")), val)


def _top_arg(top, iou):
    """the ``top`` / ``iou`` keywords of ``_moments_block``; no keyword at all without ``top``: that call is what it was"""
    return {} if top is None else {"top": top, "iou": iou}


def _select_checks(tiled, top, iou, M_total, what):
    """-> (top, iou) of a moment selection (``dvlp_moment_select``), or the ValueError that names the number outside its limits"""
    if not tiled:
        raise ValueError(f"{what} selects among the windows of a bf16 index built with tiled=True: this index is not tiled")
    top, iou = int(top), float(iou)
    if top < 1 or top > ops.MOMENT_MAX_T:
        raise ValueError(f"{what} = {top} must lie in [1, {ops.MOMENT_MAX_T}] (dvlp_moment_select)")
    if not 0.0 <= iou <= 1.0:
        raise ValueError(f"iou = {iou} must lie in [0, 1]")
    if M_total > ops.MOMENT_MAX_M:
        raise ValueError(f"{M_total} windows per pair exceed the {ops.MOMENT_MAX_M} dvlp_moment_select takes: fewer window lengths or a larger stride")
    return top, iou


class VideoIndex(_ResidentIndex):
    """A collection of videos prepared for search.  ``capacity`` videos of ``G`` regions (frames x regions per frame) in the model's compute
    ``dtype``; device memory is allocated at the first ``add``.  ``tiled=True`` (bf16, G <= 1152) selects the region-tiled pair kernel for the
    local stage and the grounding: the route for long videos (G > 288), allowed at any G in its range."""

    def __init__(self, capacity, G, dtype=torch.bfloat16, device="cuda", tiled=False):
        if int(capacity) < 1 or int(G) < 1:
            raise ValueError(f"capacity and G must be positive, got {capacity} and {G}")
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be float32 or bfloat16, got {dtype!r}")
        self.capacity, self.G, self.dtype, self.device = int(capacity), int(G), _DTYPES[dtype], torch.device(device)
        self.n = 0
        # fused route: bf16 within the fused kernel's range (host arithmetic; a negative size is "not supported")
        self.fused = self.dtype == torch.bfloat16 and call("dvlp_xattn_index_bytes", self.capacity, self.G) > 0
        self.tiled = bool(tiled)
        if self.tiled and (self.dtype != torch.bfloat16 or call("dvlp_xattn_long_index_bytes", self.capacity, self.G) < 0):
            raise ValueError(f"tiled=True needs a bfloat16 index with G <= 1152 regions, got {self.dtype} with G = {self.G}")
        self.gn = self.om = self.local = None

    def _alloc(self):
        if self.gn is not None:
            return
        if self.device.type != "cuda":
            raise DemoVLPHipError("VideoIndex lives on an MI355X device only (no CPU fallback)")
        dev = self.device
        self.gn = torch.zeros((self.capacity, 256), device=dev, dtype=torch.float32)
        self.om = torch.zeros((self.capacity, self.G), device=dev, dtype=torch.float32)
        if self.tiled:      # zeroed: the alignment gaps between its sections are never written, and the buffer is compared / saved as bytes
            self.local = torch.zeros(ops.xattn_long_index_bytes(self.capacity, self.G), device=dev, dtype=torch.uint8)
        elif self.fused:
            self.local = torch.zeros(ops.xattn_index_bytes(self.capacity, self.G), device=dev, dtype=torch.uint8)
        else:
            self.local = torch.zeros((self.capacity, self.G, 256), device=dev, dtype=self.dtype)

    # ---- filling ------------------------------------------------------------------------------------------------------
    def _checked(self, out, rows=None):
        """the tensors of an ``add`` / ``replace`` (``rows``) call, checked -> (global, local, mask, n); allocates the device memory"""
        go, lo, om = out["global_object_embeddings"], out["local_object_embeddings"], out["object_mask"]
        n = go.shape[0]
        if lo.dim() != 3 or lo.shape[1] != self.G or lo.shape[2] != 256:
            raise ValueError(f"this index holds videos of G = {self.G} regions: expected local embeddings [n, {self.G}, 256], got {tuple(lo.shape)}")
        if tuple(go.shape) != (n, 256) or lo.shape[0] != n or tuple(om.shape) != (n, self.G):
            raise ValueError(f"expected [n, 256], [n, {self.G}, 256], [n, {self.G}], got {tuple(go.shape)}, {tuple(lo.shape)}, {tuple(om.shape)}")
        if lo.dtype != self.dtype:
            raise ValueError(f"this index holds {self.dtype} embeddings, got {lo.dtype}")
        if rows is None and self.n + n > self.capacity:
            raise ValueError(f"adding {n} videos to {self.n} exceeds the capacity {self.capacity}")
        if rows is not None and len(rows) != n:
            raise ValueError(f"replace: {len(rows)} rows for {n} videos")
        if not (go.is_cuda and lo.is_cuda and om.is_cuda):
            raise DemoVLPHipError("VideoIndex lives on an MI355X device only (no CPU fallback): embeddings must be on the device")
        self._alloc()
        return go, lo, om, n

    def _write(self, r0, go, lo, om):
        n = go.shape[0]
        self.gn[r0:r0 + n] = ops.rownorm_fwd(go.detach().contiguous())[0]
        self.om[r0:r0 + n] = om.detach().float()
        if self.tiled:
            ops.xattn_long_index_add(self.local, self.capacity, self.G, r0, lo.detach().contiguous())
        elif self.fused:
            ops.xattn_index_add(self.local, self.capacity, self.G, r0, lo.detach().contiguous())
        else:
            self.local[r0:r0 + n] = lo.detach()

    def add(self, out):
        """Append the videos of ``out``, the dict ``ObjectRelation.forward(..., return_embeds=True)`` returns (its ``global_object_embeddings``
        [n, 256], ``local_object_embeddings`` [n, G, 256] and ``object_mask`` [n, G] are read).  Returns the index rows they took."""
        go, lo, om, n = self._checked(out)
        r0 = self.n
        with torch.no_grad():
            self._write(r0, go, lo, om)
        self.n += n
        return range(r0, r0 + n)

    def replace(self, rows, out):
        """Overwrite the index rows ``rows`` (ints in [0, len(index)), one per video of ``out``, the dict ``add`` takes) in place: a
        re-encoded video, or a new one in a slot ``removed()`` lists.  The rows are written by the entry ``add`` uses
        (``dvlp_xattn_index_add`` at ``row0 = r``), so a replaced row's bytes are those of a fresh index holding the same video; a removed
        row is live again.  Returns ``self``."""
        rows = self._row_list(rows, "replace")
        go, lo, om, _ = self._checked(out, rows)
        with torch.no_grad():
            for i, r in enumerate(rows):
                self._write(r, go[i:i + 1], lo[i:i + 1], om[i:i + 1])
            if rows:
                self._set_alive(rows, True)
        return self

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
        state = dict(capacity=self.capacity, G=self.G, dtype=str(self.dtype).replace("torch.", ""), n=self.n, fused=self.fused,
                     gn=self.gn.cpu(), om=self.om.cpu(), local=self.local.cpu())
        if self.tiled:      # (only tiled indexes write the key: every other state dict is what it was)
            state["tiled"] = True
        if self.alive is not None:      # (the same pattern: written once something has been removed)
            state["alive"] = self.alive.cpu()
        return state

    def load_state_dict(self, state):
        if (state["capacity"], state["G"], _DTYPES[state["dtype"]], bool(state["fused"]), bool(state.get("tiled", False))) != \
                (self.capacity, self.G, self.dtype, self.fused, self.tiled):
            raise ValueError("state_dict belongs to an index of another capacity / G / dtype / route")
        self._alloc()
        for name in ("gn", "om", "local"):
            getattr(self, name).copy_(state[name])
        self.n = int(state["n"])
        self.alive = state["alive"].to(self.gn.device) if "alive" in state else None
        return self

    # ---- search -------------------------------------------------------------------------------------------------------
    def shortlist_by_cosine(self, global_text_embeddings, shortlist, chunk=65536, allow=None):
        """The global stage alone: (ids int64 [Nq, S] ascending per row, cosines fp32 [Nq, S]) of the ``shortlist`` best videos per query
        embedding [Nq, 256] by cosine (ties by smaller id).  ``allow`` (bool [len(index)] or [Nq, len(index)] on the device; ``ValueError``
        otherwise): only allowed rows, and never a removed one; a query with fewer than S of them starts with ids -1 (cosine -inf)."""
        mask = self._filter(allow, global_text_embeddings.shape[0])
        if not global_text_embeddings.is_cuda or self.n == 0:
            raise DemoVLPHipError("shortlist_by_cosine needs a filled index and embeddings on an MI355X device")
        with torch.no_grad():
            ids, cos = self._global_stage(ops.rownorm_fwd(global_text_embeddings.detach().contiguous())[0], self._shortlist_size(shortlist), int(chunk),
                                          mask)
        return ids.long(), cos

    def _local_stage(self, local_loss, lt, text_mask, ids, holes=False):
        lam, gate = float(local_loss.lambda_softmax), local_loss.focal_type == "equal"
        if self.tiled:
            return Fn.XattnLongIndexPairsFn.apply(self.local, self.capacity, self.G, self.om, lt, text_mask, ids, lam, gate)
        if self.fused:
            return Fn.XattnIndexPairsFn.apply(self.local, self.capacity, self.G, self.om, lt, text_mask, ids, lam, gate)
        out = torch.empty(ids.shape, device=ids.device, dtype=torch.float32)
        for j in range(ids.shape[0]):                              # parity route: the query's videos gathered, multi-kernel grid [S, 1]
            rows = ids[j].long()
            if holes:                                              # a filtered search: the -1s of the query are dropped before the gather, NaN in their place
                keep = rows >= 0
                out[j] = float("nan")
                if bool(keep.any()):
                    rows = rows[keep]
                    out[j, keep] = local_loss.get_sim(self.local[rows], lt[j:j + 1], self.om[rows], None, text_mask[j:j + 1])[:, 0]
                continue
            out[j] = local_loss.get_sim(self.local[rows], lt[j:j + 1], self.om[rows], None, text_mask[j:j + 1])[:, 0]
        return out

    def _text_side(self, model, text):
        """One block of queries through the text tower -> (global [Nq, 256], local [Nq, W, 256], additive word mask [Nq, W])."""
        att = text["attention_mask"]
        text_mask = (att[:, 1:].contiguous() - 1.0) * 100.0        # as trainer.evaluate (trainer/trainer_dist.py:156-159)
        gt, lt = model.compute_text(text)
        if lt.dtype != self.dtype:
            raise ValueError(f"this index holds {self.dtype} embeddings, the model computes {lt.dtype}")
        if (self.fused or self.tiled) and call("dvlp_xattn_index_query_workspace_bytes", lt.shape[0], lt.shape[1]) < 0:
            raise DemoVLPHipError(f"captions of {lt.shape[1]} words are beyond the fused kernel's range (W <= 112)")
        return gt, lt.contiguous(), text_mask

    def _score(self, model, loss_fn, text, S, chunk, side=None, mask=None):
        """One block of queries through the text tower (or its outputs ``side``) and both stages -> (qn, ids int32 [Nq, S], cos, local);
        ``mask``: the block's rows of ``_filter``."""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        gt, lt, text_mask = side if side is not None else self._text_side(model, text)
        qn = ops.rownorm_fwd(gt.contiguous())[0]
        ids, cos = self._global_stage(qn, S, chunk, mask)
        return qn, ids, cos, self._local_stage(local_loss, lt, text_mask, ids, mask is not None)

    def _ground_block(self, loss_fn, side, att, ids, frames):
        """Grounding of one block's pairs (query j, index row ids[j, p]) from its text-tower outputs."""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        _, lt, text_mask = side
        ground = ops.xattn_long_index_pairs_ground if self.tiled else ops.xattn_index_pairs_ground
        out = ground(self.local, self.capacity, self.G, self.om, lt, text_mask, ids.to(torch.int32).contiguous(),
                     float(local_loss.lambda_softmax), local_loss.focal_type == "equal", frames)
        out["word_valid"] = att[:, 1:] > 0
        if frames is not None:
            out["word_frame"] = torch.div(out["word_region"], self.G // int(frames), rounding_mode="floor")
        return out

    def _ground_checks(self, frames):
        if not (self.fused or self.tiled):
            raise DemoVLPHipError("grounding needs the fused route (a bf16 index with G <= 288, captions of W <= 112 words) or, for long videos, "
                                  f"a bf16 index built with tiled=True (G <= 1152): this index is {self.dtype} with G = {self.G}; there is no "
                                  "fp32 grounding")
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
                    res.append(self._ground_block(loss_fn, self._text_side(model, block), block["attention_mask"],
                                                  self._live_ids(ids[q0:q0 + QUERY_BLOCK]), frames))
        finally:
            if was_training:
                model.train()
        return {name: torch.cat([r[name] for r in res]) for name in res[0]}

    # ---- moments ------------------------------------------------------------------------------------------------------
    def _moment_checks(self, frames, windows, stride):
        """-> (starts, lengths, the window lengths as a list) on the host, or the error that names what is wrong"""
        if not self.tiled:
            raise DemoVLPHipError("moments need a bf16 index built with tiled=True (G <= 1152): the region-range pair kernel "
                                  f"(dvlp_xattn_long_index_moments_fwd) is the tiled kernel's; this index is {self.dtype} with G = {self.G}")
        if frames is None or int(frames) < 1 or self.G % int(frames) != 0:
            raise ValueError(f"frames = {frames} must be a positive divisor of G = {self.G}")
        starts, lengths = moment_windows(frames, windows, stride)
        return starts, lengths, [int(windows)] if isinstance(windows, (int, np.integer)) else [int(w) for w in windows]

    def _window_scores(self, loss_fn, side, ids, frames, wins, stride):
        """one launch per window length over all windows of the pairs (query j, index row ids[j, p]), concatenated along the window axis"""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        _, lt, text_mask = side
        lam, gate = float(local_loss.lambda_softmax), local_loss.focal_type == "equal"
        cand = ids.to(torch.int32).contiguous()
        return torch.cat([ops.xattn_long_index_moments_fwd(self.local, self.capacity, self.G, self.om, lt, text_mask, cand, int(frames), w,
                                                           int(stride), lam, gate) for w in wins], dim=2)

    def _moments_block(self, loss_fn, side, ids, frames, windows, stride, top=None, iou=0.5):
        """Moments of one block's pairs (query j, index row ids[j, p]) from its text-tower outputs: one launch per window length, then the
        best window per pair by ``dvlp_topk_rows`` (ties: the smaller position -- the earlier length, then the earlier start) and, with
        ``top``, that many non-overlapping ones by ``dvlp_moment_select``."""
        starts, lengths, wins = windows
        return _best_moments(self._window_scores(loss_fn, side, ids, frames, wins, stride), starts, lengths, top, iou)

    def moments(self, model, loss_fn, text, ids, frames, windows, stride=1, top=None, iou=0.5):
        """WHEN (query j, index row ``ids[j, p]``) matched: every window of ``windows`` (a length or a sequence of lengths, in frames) at
        starts 0, ``stride``, ... of a video of ``frames`` frames (a divisor of G: regions are frame-major) scored as a video of its own --
        the local similarity of its regions alone; the global cosine, which does not depend on the window, is not added.  ``ids`` int
        [Nq, k], typically what ``search`` returned.  -> a dict on the device: ``scores`` fp32 [Nq, k, M_total] (-inf for a window without
        an unmasked region), ``start`` / ``length`` int64 [M_total] (``moment_windows``), ``best`` int64 [Nq, k] (position of the best
        window; equal scores: the earlier length, then the earlier start) and ``best_start`` / ``best_length`` / ``best_score`` [Nq, k].
        An id outside the index gives NaN scores, NaN ``best_score`` and -1 in ``best`` / ``best_start`` / ``best_length``.  A window of
        all ``frames`` frames scores what ``ground`` reports as ``score``, bit for bit.  ``tiled=True`` indexes only; no gradient flows.

        ``top = m`` (1 <= m <= 32, at most 4096 windows per pair; ``ValueError`` otherwise) adds the ``m`` best windows of each pair that
        do not overlap one another by more than ``iou`` (temporal intersection over union in frames, 0 <= iou <= 1; greedy, best first:
        ``dvlp_moment_select``): ``top`` int64 [Nq, k, m] (positions), ``top_start`` / ``top_length`` and ``top_score``.  A
        pair with fewer such windows ends in -1 / -1 / -1 / -inf, a hole is -1 / -1 / -1 / NaN throughout.  Column 0 equals ``best`` /
        ``best_start`` / ``best_length`` / ``best_score`` bit for bit (but for a pair whose every window is empty: ``best`` names window 0
        with its -inf, ``top`` selects nothing).  With ``top=None`` the dict and every launch are what they were."""
        if top is not None and not self.tiled:
            _select_checks(False, top, iou, 0, "top")
        win = self._moment_checks(frames, windows, stride)
        if top is not None:
            top, iou = _select_checks(True, top, iou, int(win[0].numel()), "top")
        ids_in = text["input_ids"]
        if not (ids_in.is_cuda and ids.is_cuda):
            raise DemoVLPHipError("VideoIndex.moments runs on an MI355X device only (no CPU fallback): move the queries and ids to cuda")
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
                    res.append(self._moments_block(loss_fn, self._text_side(model, block), self._live_ids(ids[q0:q0 + QUERY_BLOCK]), frames, win,
                                                   stride, **_top_arg(top, iou)))
        finally:
            if was_training:
                model.train()
        return _cat_moments(res)

    def search(self, model, loss_fn, text, k=10, shortlist=100, chunk=65536, ground=False, frames=None, moments=None, moment_stride=1, allow=None,
               moment_top=None, moment_iou=0.5):
        """The ``k`` best videos for every query of ``text`` (``{'input_ids', 'attention_mask'}`` [Nq, L] on the device) ->
        ``(ids int64 [Nq, k], scores fp32 [Nq, k])`` on the device, best first, equal scores by smaller id; ids are index rows.
        With ``ground=True``: ``(ids, scores, grounding)``, the dict of ``VideoIndex.ground`` for the k winners (one more launch over them,
        on the text-tower outputs the search used; ``frames`` as there).  With ``moments`` (window lengths in frames; needs ``frames`` and
        a ``tiled=True`` index): the dict of ``VideoIndex.moments`` for the k winners at stride ``moment_stride``, computed on the same
        text-tower outputs, is appended as the last element of the tuple; ``moment_top`` / ``moment_iou`` are its ``top`` / ``iou`` (several
        non-overlapping windows per winner; they need ``moments``).

        ``loss_fn`` supplies ``lambda_softmax`` / ``focal_type`` (a ``GlobalLocalLoss`` or its ``RWALoss``).  ``shortlist``: videos per query
        that reach the local stage, chosen by cosine (at most 1024); ``None`` or ``>= len(index)`` scores every video (exact search).
        ``chunk``: index rows per global-stage product.  The score is ``cos(text_j, video_i) + local(video_i, caption_j)``: in
        ``trainer.evaluate``'s terms ``global_sims + local_sims.T``, NOT its ``o2t_sims`` (which keeps the reference's transposed-addend
        quirk), so metrics of search results are not comparable with the reference's evaluation numbers.  No gradient flows.

        ``allow``: a filter, bool on the device, [len(index)] (every query) or [Nq, len(index)] (per query); anything else is a
        ``ValueError``.  Only allowed rows are shortlisted and scored (the cut to ``shortlist`` is made among them, so a narrow filter loses
        nothing), and a removed row (``remove``) is never allowed.  ``k`` is still checked against ``shortlist`` / ``len(index)``, not
        against the filter, which lives on the device: a query with fewer than ``k`` allowed rows ends in ids -1 with scores -inf, and the
        ``ground`` / ``moments`` dicts carry for those what they document for an id outside the index.  With ``allow=None`` and nothing
        removed every launch and result is what it was."""
        k, S, chunk = self._search_checks(k, shortlist, chunk)
        if ground:
            self._ground_checks(frames)
        if moment_top is not None and moments is None:
            raise ValueError(f"moment_top = {moment_top} selects among the windows of moments=...: give the window lengths")
        if moment_top is not None and not self.tiled:
            _select_checks(False, moment_top, moment_iou, 0, "moment_top")
        win = self._moment_checks(frames, moments, moment_stride) if moments is not None else None
        if moment_top is not None:
            moment_top, moment_iou = _select_checks(True, moment_top, moment_iou, int(win[0].numel()), "moment_top")
        ids_in = text["input_ids"]
        mask = self._filter(allow, ids_in.shape[0])
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
                    _, ids, cos, local = self._score(model, loss_fn, block, S, chunk, side, **self._mask_arg(mask, q0, q0 + QUERY_BLOCK))
                    val, pos = ops.topk_rows(cos + local, k)
                    top = torch.gather(ids, 1, pos.long()).long()
                    if mask is not None:
                        val = _holes(top, val)
                    res.append((top, val, self._ground_block(loss_fn, side, block["attention_mask"], top, frames) if ground else None,
                                self._moments_block(loss_fn, side, top, frames, win, moment_stride, **_top_arg(moment_top, moment_iou))
                                if win is not None else None))
        finally:
            if was_training:
                model.train()
        out = (torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res]))
        if ground:
            out += ({name: torch.cat([r[2][name] for r in res]) for name in res[0][2]},)
        if win is not None:
            out += (_cat_moments([r[3] for r in res]),)
        return out

    def search_moments(self, model, loss_fn, text, k=10, frames=None, windows=(4,), stride=1, per_video=1, iou=0.5, shortlist=100, chunk=65536,
                       allow=None):
        """WHERE, IN WHICH VIDEO: the ``k`` best (video, window) hits for every query of ``text`` -> a dict on the device, best first:
        ``ids`` int64 [Nq, k] (index rows), ``start`` / ``length`` int64 [Nq, k] (frames) and ``scores`` fp32 [Nq, k], the score of a hit
        being ``cos(text, video) + local(window)``: the video's global cosine plus the local similarity of the window's regions alone.
        ``search(..., moments=...)`` ranks videos by their whole-video score and looks for windows inside the winners only, so a long video
        whose short window matches is diluted by its other frames and its moment is never reported; here every window of every
        shortlisted video competes.

        Per query block, all on the device and without a host synchronisation: the global stage (the ``shortlist`` best videos by cosine,
        at most 1024; ``None`` or ``>= len(index)``: every video; ``allow`` and removed rows as in ``search``), one launch of
        ``dvlp_xattn_long_index_moments_fwd`` per window length over ALL shortlisted videos (``frames``, ``windows``, ``stride`` as in
        ``moments``), ``dvlp_moment_select`` with ``T = per_video`` over the [Nq S, M_total] window scores -- up to ``per_video`` hits per
        video, none overlapping an earlier one of that video by more than ``iou`` -- the cosine added, and one
        ``dvlp_topk_rows`` over the [Nq, S per_video] hits.  Equal scores go to the smaller index row, then to the video's better hit.
        A query with fewer than ``k`` hits (a narrow ``allow``, removed rows, videos with fewer selectable windows than ``per_video``) ends
        in ``ids = start = length = -1`` with score -inf.

        Checked before anything is launched, each a ``ValueError`` naming the number: the rules of ``moments`` and ``search`` on ``frames``,
        ``windows``, ``stride``, ``shortlist`` and ``chunk``; ``1 <= per_video <= 32``; ``0 <= iou <= 1``;
        ``1 <= k <= min(1024, S per_video)``; at most 4096 windows per video.  ``tiled=True`` indexes only; no gradient flows."""
        if not self.tiled:
            _select_checks(False, per_video, iou, 0, "search_moments")
        _, S, chunk = self._search_checks(1, shortlist, chunk)
        starts, lengths, wins = self._moment_checks(frames, windows, stride)
        M = int(starts.numel())
        T, iou = _select_checks(True, per_video, iou, M, "per_video")
        k = int(k)
        if k < 1 or k > min(TOPK_MAX, S * T):
            raise ValueError(f"k = {k} must lie in [1, min({TOPK_MAX}, shortlist x per_video = {S * T})]")
        ids_in = text["input_ids"]
        mask = self._filter(allow, ids_in.shape[0])
        if not ids_in.is_cuda:
            raise DemoVLPHipError("VideoIndex.search_moments runs on an MI355X device only (no CPU fallback): move the queries to cuda")
        dev = ids_in.device
        start, length = starts.to(dev), lengths.to(dev)
        start32, length32 = start.to(torch.int32), length.to(torch.int32)
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for q0 in range(0, ids_in.shape[0], QUERY_BLOCK):
                    block = {name: t[q0:q0 + QUERY_BLOCK] for name, t in text.items() if isinstance(t, torch.Tensor)}
                    side = self._text_side(model, block)
                    ids, cos = self._global_stage(ops.rownorm_fwd(side[0].contiguous())[0], S, chunk, self._rows_of(mask, q0, q0 + QUERY_BLOCK))
                    Nq = ids.shape[0]
                    val, pos = ops.moment_select(self._window_scores(loss_fn, side, ids, frames, wins, stride), start32, length32, T, iou)
                    hit_val, hit = ops.topk_rows((val + cos[:, :, None]).view(Nq, S * T), k)      # hit: video s = hit // T, its pick hit % T
                    hit = hit.long()
                    window = torch.gather(pos.view(Nq, S * T).long(), 1, hit)
                    video = torch.gather(ids.long(), 1, torch.div(hit, T, rounding_mode="floor"))
                    none, at, minus = window < 0, window.clamp(0, M - 1), torch.full_like(window, -1)
                    res.append((torch.where(none, minus, video), torch.where(none, minus, start[at]), torch.where(none, minus, length[at]),
                                torch.where(none, torch.full_like(hit_val, float("-inf")), hit_val)))
        finally:
            if was_training:
                model.train()
        return dict(ids=torch.cat([r[0] for r in res]), start=torch.cat([r[1] for r in res]), length=torch.cat([r[2] for r in res]),
                    scores=torch.cat([r[3] for r in res]))


def _best_moments(scores, starts, lengths, top=None, iou=0.5):
    """the moments dict of window scores [N, k, M_total]: the best window per pair by ``dvlp_topk_rows`` (K = 1; a hole's NaN row: -1 / NaN)
    and, with ``top``, the ``top`` best that do not overlap by more than ``iou`` by ``dvlp_moment_select`` (padding: -1 / -inf; a hole: -1 / NaN)"""
    Nq, k, M = scores.shape
    val, pos = ops.topk_rows(scores.view(Nq * k, M), 1)
    val, pos = val.view(Nq, k), pos.view(Nq, k).long()
    hole = torch.isnan(val)
    start, length = starts.to(scores.device), lengths.to(scores.device)
    minus = torch.full_like(pos, -1)
    at = pos.clamp(0, M - 1)
    out = dict(scores=scores, start=start, length=length, best=torch.where(hole, minus, pos), best_start=torch.where(hole, minus, start[at]),
               best_length=torch.where(hole, minus, length[at]), best_score=val)
    if top is not None:
        tval, tpos = ops.moment_select(scores, start.to(torch.int32), length.to(torch.int32), top, iou)
        tpos = tpos.long()
        none, at, minus = tpos < 0, tpos.clamp(0, M - 1), torch.full_like(tpos, -1)
        out.update(top=tpos, top_start=torch.where(none, minus, start[at]), top_length=torch.where(none, minus, length[at]), top_score=tval)
    return out


def _cat_moments(res):
    """the moments dicts of consecutive query blocks as one (``start`` / ``length`` describe the windows, not the queries)"""
    return {name: res[0][name] if name in ("start", "length") else torch.cat([r[name] for r in res]) for name in res[0]}


class CaptionIndex(_ResidentIndex):
    """A collection of captions (tags, descriptions) prepared for video-to-text search.  ``capacity`` captions of exactly ``W`` words (the
    tokenised length minus the CLS position) in the model's compute ``dtype``; device memory is allocated at the first ``add``.

    Resident: the normalised global text embeddings ``gn`` [capacity, 256], the additive word masks ``tm`` [capacity, W] and the caption side
    of the fused local-similarity kernel exactly as that kernel reads it (``dvlp_xattn_caption_index_add``: 123 392 bytes per caption at
    W = 99).  bf16 with W <= 112 is the ``fused`` route; anything else keeps the raw embeddings [capacity, W, 256] and scores each query
    video's shortlist with ``RWALoss.get_sim`` on a [1, S] grid (the parity route: exact and slow).  ``tiled=True`` (bf16, W <= 112) keeps
    the same resident bytes and selects the region-tiled pair kernel for the local stage and the grounding: the route for long query
    videos (288 < G <= 1152), allowed at any G in its range."""

    def __init__(self, capacity, W, dtype=torch.bfloat16, device="cuda", tiled=False):
        if int(capacity) < 1 or int(W) < 1:
            raise ValueError(f"capacity and W must be positive, got {capacity} and {W}")
        if dtype not in _DTYPES:
            raise ValueError(f"dtype must be float32 or bfloat16, got {dtype!r}")
        self.capacity, self.W, self.dtype, self.device = int(capacity), int(W), _DTYPES[dtype], torch.device(device)
        self.n = 0
        # fused route: bf16 within the fused kernel's range (host arithmetic; a negative size is "not supported")
        self.fused = self.dtype == torch.bfloat16 and call("dvlp_xattn_caption_index_bytes", self.capacity, self.W) > 0
        self.tiled = bool(tiled)
        if self.tiled and not self.fused:      # (one resident layout: a tiled index is a fused index with another pair kernel)
            raise ValueError(f"tiled=True needs a bfloat16 index of captions with W <= 112 words, got {self.dtype} with W = {self.W}")
        self.gn = self.tm = self.local = None

    def _alloc(self):
        if self.gn is not None:
            return
        if self.device.type != "cuda":
            raise DemoVLPHipError("CaptionIndex lives on an MI355X device only (no CPU fallback)")
        dev = self.device
        self.gn = torch.zeros((self.capacity, 256), device=dev, dtype=torch.float32)
        self.tm = torch.zeros((self.capacity, self.W), device=dev, dtype=torch.float32)
        if self.fused:      # zeroed: the alignment gaps between its sections are never written, and the buffer is compared / saved as bytes
            self.local = torch.zeros(ops.xattn_caption_index_bytes(self.capacity, self.W), device=dev, dtype=torch.uint8)
        else:
            self.local = torch.zeros((self.capacity, self.W, 256), device=dev, dtype=self.dtype)

    # ---- filling ------------------------------------------------------------------------------------------------------
    def _checked(self, global_text, local_text, attention_mask, rows=None):
        """the tensors of an ``add`` / ``replace`` (``rows``) call, checked -> (global, local, attention mask, n); allocates the device memory"""
        gt, lt, att = global_text, local_text, attention_mask
        n = gt.shape[0]
        if lt.dim() != 3 or lt.shape[1] != self.W or lt.shape[2] != 256:
            raise ValueError(f"this index holds captions of W = {self.W} words: expected local embeddings [n, {self.W}, 256], got {tuple(lt.shape)}")
        if tuple(gt.shape) != (n, 256) or lt.shape[0] != n or tuple(att.shape) != (n, self.W + 1):
            raise ValueError(f"expected [n, 256], [n, {self.W}, 256], [n, {self.W + 1}], got {tuple(gt.shape)}, {tuple(lt.shape)}, {tuple(att.shape)}")
        if lt.dtype != self.dtype:
            raise ValueError(f"this index holds {self.dtype} embeddings, got {lt.dtype}")
        if rows is None and self.n + n > self.capacity:
            raise ValueError(f"adding {n} captions to {self.n} exceeds the capacity {self.capacity}")
        if rows is not None and len(rows) != n:
            raise ValueError(f"replace: {len(rows)} rows for {n} captions")
        if not (gt.is_cuda and lt.is_cuda and att.is_cuda):
            raise DemoVLPHipError("CaptionIndex lives on an MI355X device only (no CPU fallback): embeddings must be on the device")
        self._alloc()
        return gt, lt, att, n

    def _write(self, r0, gt, lt, att):
        n = gt.shape[0]
        self.gn[r0:r0 + n] = ops.rownorm_fwd(gt.detach().contiguous())[0]
        self.tm[r0:r0 + n] = ((att[:, 1:].contiguous() - 1.0) * 100.0).float()      # as trainer.evaluate (trainer/trainer_dist.py:156-159)
        if self.fused:
            ops.xattn_caption_index_add(self.local, self.capacity, self.W, r0, lt.detach().contiguous())
        else:
            self.local[r0:r0 + n] = lt.detach()

    def add(self, global_text, local_text, attention_mask):
        """Append captions from the text tower's outputs (``model.compute_text``): ``global_text`` [n, 256], ``local_text`` [n, W, 256] and
        the tokeniser's ``attention_mask`` [n, W + 1] (CLS position first).  Exactly ``W`` words: another width raises ``ValueError`` -- the
        text tower's bf16 output depends on the shape it ran at, so padding here would break bit-equality with the full grid.  Returns the
        index rows they took."""
        gt, lt, att, n = self._checked(global_text, local_text, attention_mask)
        r0 = self.n
        with torch.no_grad():
            self._write(r0, gt, lt, att)
        self.n += n
        return range(r0, r0 + n)

    def replace(self, rows, global_text, local_text, attention_mask):
        """Overwrite the index rows ``rows`` (ints in [0, len(index)), one per caption; the three tensors ``add`` takes) in place: a
        re-worded caption, or a new one in a slot ``removed()`` lists.  The rows are written by the entry ``add`` uses
        (``dvlp_xattn_caption_index_add`` at ``row0 = r``), so a replaced row's bytes are those of a fresh index holding the same caption;
        a removed row is live again.  Returns ``self``."""
        rows = self._row_list(rows, "replace")
        gt, lt, att, _ = self._checked(global_text, local_text, attention_mask, rows)
        with torch.no_grad():
            for i, r in enumerate(rows):
                self._write(r, gt[i:i + 1], lt[i:i + 1], att[i:i + 1])
            if rows:
                self._set_alive(rows, True)
        return self

    def add_batches(self, model, batches):
        """Run the text tower only (``model.compute_text``) on every batch (``{'text': {'input_ids', 'attention_mask'}, ...}`` or the text
        dict itself) in eval mode and add its captions; the model's training flag is restored."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                for data in batches:
                    text = data["text"] if "text" in data else data
                    gt, lt = model.compute_text(text)
                    self.add(gt, lt, text["attention_mask"])
        finally:
            if was_training:
                model.train()
        return self

    # ---- persistence --------------------------------------------------------------------------------------------------
    def state_dict(self):
        self._alloc()
        state = dict(capacity=self.capacity, W=self.W, dtype=str(self.dtype).replace("torch.", ""), n=self.n, fused=self.fused,
                     gn=self.gn.cpu(), tm=self.tm.cpu(), local=self.local.cpu())
        if self.tiled:      # (only tiled indexes write the key: every other state dict is what it was)
            state["tiled"] = True
        if self.alive is not None:      # (the same pattern: written once something has been removed)
            state["alive"] = self.alive.cpu()
        return state

    def load_state_dict(self, state):
        if (state["capacity"], state["W"], _DTYPES[state["dtype"]], bool(state["fused"])) != (self.capacity, self.W, self.dtype, self.fused):
            raise ValueError("state_dict belongs to an index of another capacity / W / dtype")
        if bool(state.get("tiled", False)) != self.tiled:
            raise ValueError("state_dict belongs to an index of another route (tiled / not tiled)")
        self._alloc()
        for name in ("gn", "tm", "local"):
            getattr(self, name).copy_(state[name])
        self.n = int(state["n"])
        self.alive = state["alive"].to(self.gn.device) if "alive" in state else None
        return self

    # ---- search -------------------------------------------------------------------------------------------------------
    def shortlist_by_cosine(self, global_object_embeddings, shortlist, chunk=65536, allow=None):
        """The global stage alone: (ids int64 [Nv, S] ascending per row, cosines fp32 [Nv, S]) of the ``shortlist`` best captions per video
        embedding [Nv, 256] by cosine (ties by smaller id).  ``allow`` (bool [len(index)] or [Nv, len(index)] on the device; ``ValueError``
        otherwise): only allowed rows, and never a removed one; a video with fewer than S of them starts with ids -1 (cosine -inf)."""
        mask = self._filter(allow, global_object_embeddings.shape[0])
        if not global_object_embeddings.is_cuda or self.n == 0:
            raise DemoVLPHipError("shortlist_by_cosine needs a filled index and embeddings on an MI355X device")
        with torch.no_grad():
            ids, cos = self._global_stage(ops.rownorm_fwd(global_object_embeddings.detach().contiguous())[0], self._shortlist_size(shortlist),
                                          int(chunk), mask)
        return ids.long(), cos

    def _local_stage(self, local_loss, lo, om, ids, holes=False):
        lam, gate = float(local_loss.lambda_softmax), local_loss.focal_type == "equal"
        if self.tiled:
            return Fn.XattnLongCaptionIndexPairsFn.apply(self.local, self.capacity, self.W, self.tm, lo, om, ids, lam, gate)
        if self.fused:
            return Fn.XattnCaptionIndexPairsFn.apply(self.local, self.capacity, self.W, self.tm, lo, om, ids, lam, gate)
        out = torch.empty(ids.shape, device=ids.device, dtype=torch.float32)
        for i in range(ids.shape[0]):                              # parity route: the video's captions gathered, multi-kernel grid [1, S]
            rows = ids[i].long()
            if holes:                                              # a filtered search: the -1s of the video are dropped before the gather, NaN in their place
                keep = rows >= 0
                out[i] = float("nan")
                if bool(keep.any()):
                    rows = rows[keep]
                    out[i, keep] = local_loss.get_sim(lo[i:i + 1], self.local[rows], om[i:i + 1], None, self.tm[rows])[0]
                continue
            out[i] = local_loss.get_sim(lo[i:i + 1], self.local[rows], om[i:i + 1], None, self.tm[rows])[0]
        return out

    def _video_side(self, model, data):
        """One block of query videos through the object tower -> (global [Nv, 256], local [Nv, G, 256], additive region mask [Nv, G])."""
        go, lo, add_mask = model.compute_object(data["object"], data["object_mask"])
        if lo.dtype != self.dtype:
            raise ValueError(f"this index holds {self.dtype} embeddings, the model computes {lo.dtype}")
        if self.tiled:
            if call("dvlp_xattn_long_caption_index_query_workspace_bytes", lo.shape[0], lo.shape[1], self.W) < 0:
                raise DemoVLPHipError(f"videos of {lo.shape[1]} regions are beyond the tiled kernel's range (G <= 1152)")
        elif self.fused and call("dvlp_xattn_caption_index_query_workspace_bytes", lo.shape[0], lo.shape[1], self.W) < 0:
            raise DemoVLPHipError(f"videos of {lo.shape[1]} regions are beyond the fused kernel's range with captions of {self.W} words "
                                  "(G <= 288 and 160 KB of LDS per pair)")
        return go, lo.contiguous(), add_mask[:, 1:, ...].float().contiguous()

    def _score(self, model, loss_fn, data, S, chunk, side=None, mask=None):
        """One block of query videos through the object tower (or its outputs ``side``) and both stages -> (qn, ids int32 [Nv, S], cos, local);
        ``mask``: the block's rows of ``_filter``."""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        go, lo, om = side if side is not None else self._video_side(model, data)
        qn = ops.rownorm_fwd(go.contiguous())[0]
        ids, cos = self._global_stage(qn, S, chunk, mask)
        return qn, ids, cos, self._local_stage(local_loss, lo, om, ids, mask is not None)

    def _ground_block(self, loss_fn, side, ids, frames):
        """Grounding of one block's pairs (video i, index row ids[i, p]) from its object-tower outputs."""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        _, lo, om = side
        ground = ops.xattn_long_caption_index_pairs_ground if self.tiled else ops.xattn_caption_index_pairs_ground
        out = ground(self.local, self.capacity, self.W, self.tm, lo, om, ids.to(torch.int32).contiguous(),
                     float(local_loss.lambda_softmax), local_loss.focal_type == "equal", frames)
        inside = (ids >= 0) & (ids < self.capacity)
        out["word_valid"] = (self.tm[ids.long().clamp(0, self.capacity - 1)] == 0) & inside[..., None]
        if frames is not None:
            out["word_frame"] = torch.div(out["word_region"], lo.shape[1] // int(frames), rounding_mode="floor")
        return out

    def _ground_checks(self, frames, G):
        if not self.fused:
            raise DemoVLPHipError("grounding needs the fused route (a bf16 index of captions with W <= 112 words, videos of G <= 288 regions): "
                                  f"this index is {self.dtype} with W = {self.W}; there is no fp32 / long-caption grounding")
        if frames is not None and (int(frames) < 1 or G % int(frames) != 0):
            raise ValueError(f"frames = {frames} must be a positive divisor of G = {G}")

    @staticmethod
    def _blocks(data):
        n = data["object"].shape[0]
        for v0 in range(0, n, VIDEO_BLOCK):
            yield v0, {name: t[v0:v0 + VIDEO_BLOCK] for name, t in data.items() if isinstance(t, torch.Tensor)}

    def ground(self, model, loss_fn, data, ids, frames=None):
        """Where the local similarity of (video i, index row ``ids[i, p]``) comes from; ``data`` = ``{'object', 'object_mask'}`` on the
        device, ``ids`` int [Nv, k], typically what ``search`` returned.  -> a dict on the device (``ops.xattn_caption_index_pairs_ground``):
        ``score`` [Nv, k] (the local addend of the search score, bit for bit), ``word_scores`` / ``word_region`` / ``word_region_weight``
        [Nv, k, W], ``region_scores`` / ``region_word`` [Nv, k, G], ``word_valid`` bool [Nv, k, W] (words of caption ``ids[i, p]`` that are
        not padding, from the index's stored mask) and, with ``frames`` (a divisor of G: regions are frame-major), ``frame_scores``
        [Nv, k, frames] and ``word_frame`` = ``word_region // (G // frames)``.  Fused and tiled routes only; no gradient flows."""
        obj = data["object"]
        self._ground_checks(frames, int(obj.shape[1] * obj.shape[2]))
        if not (obj.is_cuda and ids.is_cuda):
            raise DemoVLPHipError("CaptionIndex.ground runs on an MI355X device only (no CPU fallback): move the videos and ids to cuda")
        if ids.dim() != 2 or ids.shape[0] != obj.shape[0] or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"ids must be int [Nv = {obj.shape[0]}, k], got {ids.dtype} {tuple(ids.shape)}")
        if self.n == 0:
            raise ValueError("the index is empty")
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for v0, block in self._blocks(data):
                    res.append(self._ground_block(loss_fn, self._video_side(model, block), self._live_ids(ids[v0:v0 + VIDEO_BLOCK]), frames))
        finally:
            if was_training:
                model.train()
        return {name: torch.cat([r[name] for r in res]) for name in res[0]}

    # ---- moments ------------------------------------------------------------------------------------------------------
    def _moment_checks(self, frames, windows, stride, G):
        """-> (starts, lengths, the window lengths as a list) on the host for query videos of G regions, or the error that names what is wrong"""
        if not self.tiled:
            raise DemoVLPHipError("moments need a bf16 index built with tiled=True (W <= 112): the region-range pair kernel "
                                  f"(dvlp_xattn_long_caption_index_moments_fwd) is the tiled kernel's; this index is {self.dtype} with W = {self.W}")
        if frames is None or int(frames) < 1 or G % int(frames) != 0:
            raise ValueError(f"frames = {frames} must be a positive divisor of G = {G}")
        starts, lengths = moment_windows(frames, windows, stride)
        return starts, lengths, [int(windows)] if isinstance(windows, (int, np.integer)) else [int(w) for w in windows]

    def _window_scores(self, loss_fn, side, ids, frames, wins, stride, window_major):
        """one launch per window length over all windows of the pairs (video i, index row ids[i, p]), concatenated along the window axis"""
        local_loss = getattr(loss_fn, "local_loss", loss_fn)
        _, lo, om = side
        lam, gate = float(local_loss.lambda_softmax), local_loss.focal_type == "equal"
        cand = ids.to(torch.int32).contiguous()
        return torch.cat([ops.xattn_long_caption_index_moments_fwd(self.local, self.capacity, self.W, self.tm, lo, om, cand, int(frames), w,
                                                                   int(stride), lam, gate, window_major=window_major) for w in wins],
                         dim=1 if window_major else 2)

    def _moments_block(self, loss_fn, side, ids, frames, windows, stride, top=None, iou=0.5):
        """Moments of one block's pairs (video i, index row ids[i, p]) from its object-tower outputs: one launch per window length, then the
        best window per pair by ``dvlp_topk_rows`` (ties: the smaller position -- the earlier length, then the earlier start) and, with
        ``top``, that many non-overlapping ones by ``dvlp_moment_select``."""
        starts, lengths, wins = windows
        return _best_moments(self._window_scores(loss_fn, side, ids, frames, wins, stride, False), starts, lengths, top, iou)

    def moments(self, model, loss_fn, data, ids, frames, windows, stride=1, top=None, iou=0.5):
        """WHEN (video i, index row ``ids[i, p]``) matched: every window of ``windows`` (a length or a sequence of lengths, in frames) at
        starts 0, ``stride``, ... of the query videos of ``frames`` frames (a divisor of their G: regions are frame-major) scored as a video
        of its own against the caption -- the local similarity of its regions alone; the global cosine, which does not depend on the window,
        is not added.  ``data`` = ``{'object', 'object_mask'}`` on the device, ``ids`` int [Nv, k], typically what ``search`` returned.
        -> the dict of ``VideoIndex.moments`` on the device: ``scores`` fp32 [Nv, k, M_total] (-inf for a window without an unmasked
        region), ``start`` / ``length`` int64 [M_total] (``moment_windows``), ``best`` int64 [Nv, k] (position of the best window; equal
        scores: the earlier length, then the earlier start) and ``best_start`` / ``best_length`` / ``best_score`` [Nv, k].  An id outside
        the index gives NaN scores, NaN ``best_score`` and -1 in ``best`` / ``best_start`` / ``best_length``.  Each score equals, bit for
        bit, what ``VideoIndex.moments`` gives for the same pair and window.  ``tiled=True`` indexes only; no gradient flows.
        ``top`` / ``iou``: as in ``VideoIndex.moments`` -- the keys ``top`` / ``top_start`` / ``top_length`` / ``top_score`` [Nv, k, top], the
        best windows of each pair that do not overlap one another by more than ``iou`` (``dvlp_moment_select``)."""
        obj = data["object"]
        if top is not None and not self.tiled:
            _select_checks(False, top, iou, 0, "top")
        win = self._moment_checks(frames, windows, stride, int(obj.shape[1] * obj.shape[2]))
        if top is not None:
            top, iou = _select_checks(True, top, iou, int(win[0].numel()), "top")
        if ids.dim() != 2 or ids.shape[0] != obj.shape[0] or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"ids must be int [Nv = {obj.shape[0]}, k], got {ids.dtype} {tuple(ids.shape)}")
        if self.n == 0:
            raise ValueError("the index is empty")
        if not (obj.is_cuda and ids.is_cuda):
            raise DemoVLPHipError("CaptionIndex.moments runs on an MI355X device only (no CPU fallback): move the videos and ids to cuda")
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for v0, block in self._blocks(data):
                    res.append(self._moments_block(loss_fn, self._video_side(model, block), self._live_ids(ids[v0:v0 + VIDEO_BLOCK]), frames, win,
                                                   stride, **_top_arg(top, iou)))
        finally:
            if was_training:
                model.train()
        return _cat_moments(res)

    def timeline(self, model, loss_fn, data, frames, windows, stride=1, k=5, shortlist=100, chunk=65536, allow=None):
        """WHICH captions apply WHEN: for every window of ``windows`` (as in ``moments``) of every query video of ``data``, the ``k`` best
        captions of the video's cosine shortlist (``shortlist`` captions chosen by the whole video's cosine, at most 1024; ``None`` or
        ``>= len(index)``: every caption), ranked by the window's local similarity alone -- the whole-video cosine does not depend on the
        window and is not added.  One window-major launch of ``dvlp_xattn_long_caption_index_moments_fwd`` per window length, then one
        ``dvlp_topk_rows`` over the [Nv M_total, S] rows.  -> a dict on the device: ``ids`` int64 [Nv, M_total, k] (index rows),
        ``scores`` fp32 [Nv, M_total, k], ``cosine`` fp32 [Nv, M_total, k] (the shortlist cosine of each returned caption, for a caller
        who wants to add a prior) and ``start`` / ``length`` int64 [M_total] (``moment_windows``).  Best first; equal scores go to the
        smaller index row.  A window without an unmasked region gives ``scores`` = -inf, ``ids`` = -1 and ``cosine`` = NaN.  The checks on
        ``k``, ``shortlist`` and ``chunk`` are those of ``search``.  ``tiled=True`` indexes only; no gradient flows.  ``allow`` as in
        ``search`` (bool [len(index)] or [Nv, len(index)] on the device): no disallowed or removed caption is listed; a window of a video
        with fewer than ``k`` allowed captions ends like an empty one (``ids`` = -1, ``scores`` = -inf, ``cosine`` = NaN)."""
        k, S, chunk = self._search_checks(k, shortlist, chunk)
        obj = data["object"]
        starts, lengths, wins = self._moment_checks(frames, windows, stride, int(obj.shape[1] * obj.shape[2]))
        mask = self._filter(allow, obj.shape[0])
        if not obj.is_cuda:
            raise DemoVLPHipError("CaptionIndex.timeline runs on an MI355X device only (no CPU fallback): move the videos to cuda")
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for v0, block in self._blocks(data):
                    side = self._video_side(model, block)
                    ids, cos = self._global_stage(ops.rownorm_fwd(side[0].contiguous())[0], S, chunk,          # ids ascending per row
                                                  self._rows_of(mask, v0, v0 + VIDEO_BLOCK))
                    scores = self._window_scores(loss_fn, side, ids, frames, wins, stride, True)                # [Nv, M_total, S]
                    Nv, M = scores.shape[:2]
                    val, pos = ops.topk_rows(scores.view(Nv * M, S), k)
                    val, pos = val.view(Nv, M, k), pos.view(Nv, M, k).long().clamp(min=0)
                    top = torch.gather(ids.long()[:, None, :].expand(Nv, M, S), 2, pos)
                    if mask is not None:                           # a hole of the shortlist (NaN in every window, sorted last)
                        val = _holes(top, val)
                    empty = torch.isneginf(val)
                    prior = torch.gather(cos[:, None, :].expand(Nv, M, S), 2, pos)
                    res.append((torch.where(empty, torch.full_like(top, -1), top), val,
                                torch.where(empty, torch.full_like(prior, float("nan")), prior)))
        finally:
            if was_training:
                model.train()
        return dict(ids=torch.cat([r[0] for r in res]), scores=torch.cat([r[1] for r in res]), cosine=torch.cat([r[2] for r in res]),
                    start=starts.to(obj.device), length=lengths.to(obj.device))

    def search(self, model, loss_fn, data, k=10, shortlist=100, chunk=65536, ground=False, frames=None, moments=None, moment_stride=1, allow=None,
               moment_top=None, moment_iou=0.5):
        """The ``k`` best captions for every video of ``data`` (``{'object', 'object_mask'}`` on the device) ->
        ``(ids int64 [Nv, k], scores fp32 [Nv, k])`` on the device, best first, equal scores by smaller id; ids are index rows.
        With ``ground=True``: ``(ids, scores, grounding)``, the dict of ``CaptionIndex.ground`` for the k winners (one more launch over them,
        on the object-tower outputs the search used; ``frames`` as there).  With ``moments`` (window lengths in frames; needs ``frames`` and
        a ``tiled=True`` index): the dict of ``CaptionIndex.moments`` for the k winners at stride ``moment_stride``, computed on the same
        object-tower outputs, is appended as the last element of the tuple; ``moment_top`` / ``moment_iou`` are its ``top`` / ``iou`` (they
        need ``moments``).

        ``loss_fn`` supplies ``lambda_softmax`` / ``focal_type`` (a ``GlobalLocalLoss`` or its ``RWALoss``).  ``shortlist``: captions per
        video that reach the local stage, chosen by cosine (at most 1024); ``None`` or ``>= len(index)`` scores every caption (exact search).
        ``chunk``: index rows per global-stage product.  The score is ``cos(video_i, text_j) + local(video_i, caption_j)``, the pair score of
        ``VideoIndex.search``: an exact search here is the transpose of an exact search there.  In ``trainer.evaluate``'s terms it is
        ``global_sims.T + local_sims``, NOT the transpose of its ``o2t_sims`` (which keeps the reference's transposed-addend quirk), so
        metrics of search results are not comparable with the reference's evaluation numbers.  No gradient flows.

        ``allow``: a filter, bool on the device, [len(index)] (every video) or [Nv, len(index)] (per video); anything else is a
        ``ValueError``.  Semantics of ``VideoIndex.search``: the shortlist is cut among the allowed rows, a removed row is never allowed,
        ``k`` is checked against ``shortlist`` / ``len(index)`` and not against the filter, and a video with fewer than ``k`` allowed
        captions ends in ids -1 with scores -inf."""
        k, S, chunk = self._search_checks(k, shortlist, chunk)
        obj = data["object"]
        mask = self._filter(allow, obj.shape[0])
        if ground:
            self._ground_checks(frames, int(obj.shape[1] * obj.shape[2]))
        if moment_top is not None and moments is None:
            raise ValueError(f"moment_top = {moment_top} selects among the windows of moments=...: give the window lengths")
        if moment_top is not None and not self.tiled:
            _select_checks(False, moment_top, moment_iou, 0, "moment_top")
        win = self._moment_checks(frames, moments, moment_stride, int(obj.shape[1] * obj.shape[2])) if moments is not None else None
        if moment_top is not None:
            moment_top, moment_iou = _select_checks(True, moment_top, moment_iou, int(win[0].numel()), "moment_top")
        if not obj.is_cuda:
            raise DemoVLPHipError("CaptionIndex.search runs on an MI355X device only (no CPU fallback): move the videos to cuda")
        was_training = model.training
        model.eval()
        res = []
        try:
            with torch.no_grad():
                for v0, block in self._blocks(data):
                    side = self._video_side(model, block)
                    _, ids, cos, local = self._score(model, loss_fn, block, S, chunk, side, **self._mask_arg(mask, v0, v0 + VIDEO_BLOCK))
                    val, pos = ops.topk_rows(cos + local, k)
                    top = torch.gather(ids, 1, pos.long()).long()
                    if mask is not None:
                        val = _holes(top, val)
                    res.append((top, val, self._ground_block(loss_fn, side, top, frames) if ground else None,
                                self._moments_block(loss_fn, side, top, frames, win, moment_stride, **_top_arg(moment_top, moment_iou))
                                if win is not None else None))
        finally:
            if was_training:
                model.train()
        out = (torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res]))
        if ground:
            out += ({name: torch.cat([r[2][name] for r in res]) for name in res[0][2]},)
        if win is not None:
            out += (_cat_moments([r[3] for r in res]),)
        return out


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


def evaluate_t2v(model, loss_fn, batches, shortlist=None, chunk=65536, tiled=False):
    """Text-to-video metrics of two-stage search on one loader (a re-iterable of tokenised batches ``{'text', 'object', 'object_mask'}``, query
    b of a batch belonging to its video b): every video goes into one ``VideoIndex``, every caption is searched with ``shortlist``, and
    ``metric.t2v_metrics`` is taken of ``two_stage_sims``.  Comparing ``shortlist=None`` with a partial one measures what the shortlist
    costs in recall.  ``tiled``: passed on to ``VideoIndex`` (long videos).  Search orientation (see the module docstring): not comparable
    with ``trainer.evaluate``.
    -> ``{'t2v_metrics': dict, 'sims': numpy [N, N]}``."""
    from . import metric as M
    batches = list(batches)
    N = sum(int(b["object"].shape[0]) for b in batches)
    obj = batches[0]["object"]
    index = VideoIndex(N, int(obj.shape[1] * obj.shape[2]), model.compute_dtype, obj.device, tiled=tiled).add_batches(model, batches)
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


def evaluate_v2t(model, loss_fn, batches, shortlist=None, chunk=65536, tiled=False):
    """Video-to-text metrics of two-stage search on one loader (as ``evaluate_t2v``: caption b of a batch belongs to its video b): every
    caption goes into one ``CaptionIndex``, every video is searched with ``shortlist``, and ``metric.v2t_metrics`` is taken of
    ``two_stage_sims``.  ``tiled``: passed on to ``CaptionIndex`` (long videos).  Search orientation (see the module docstring): not
    comparable with ``trainer.evaluate``.
    -> ``{'v2t_metrics': dict, 'sims': numpy [N captions, N videos]}`` -- text x video, the orientation ``metric.v2t_metrics`` expects (it
    transposes to rank captions per video itself), i.e. the transpose of the [video, caption] matrix the searches produce."""
    from . import metric as M
    batches = list(batches)
    ids0 = batches[0]["text"]["input_ids"]
    N = sum(int(b["text"]["input_ids"].shape[0]) for b in batches)
    index = CaptionIndex(N, int(ids0.shape[1]) - 1, model.compute_dtype, ids0.device, tiled=tiled).add_batches(model, batches)
    S = index._shortlist_size(shortlist)
    if S < N and S > TOPK_MAX:
        raise ValueError(f"a partial shortlist is limited to {TOPK_MAX} (dvlp_topk_rows)")
    was_training = model.training
    model.eval()
    g, ids, scores = [], [], []
    try:
        with torch.no_grad():
            for data in batches:
                qn, i, cos, local = index._score(model, loss_fn, data, S, int(chunk))
                g.append(ops.gemm(qn, index.gn, qn.shape[0], N, 256, dtype=ops.F32).cpu().numpy())
                ids.append(i.cpu().numpy())
                scores.append((cos + local).cpu().numpy())
    finally:
        if was_training:
            model.train()
    sims = two_stage_sims(np.concatenate(g), np.concatenate(ids), np.concatenate(scores)).T
    return dict(v2t_metrics=M.v2t_metrics(sims), sims=sims)
