"""Filtered search and row removal, host side: the export and the argument checks of ``dvlp_topk_rows_masked``, ``ops.pack_allow_bits``
against a bit-by-bit loop, the ``allow=`` / ``remove`` / ``replace`` checks of ``search.VideoIndex`` and ``search.CaptionIndex`` (no GPU
needed for any of them), and the numpy reference of the masked top-k that ``tests/test_gpu_filtered_search.py`` compares the kernel with,
itself checked here against a brute-force selection."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from demovlp_amd import DemoVLPHipError, _lib, ops, search
from demovlp_amd.loss import RWALoss

ONE = 1 << 12      # a non-null, 4-byte aligned pointer value for argument checks that return before anything is launched
ERR_SHAPE = -2     # DVLP_ERR_SHAPE (include/demovlp_hip.h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference: dvlp_topk_rows on each row with its disallowed columns deleted
# ---------------------------------------------------------------------------------------------------------------------------------------
def masked_topk_ref(x, allow, K, base=0):
    """x fp32 [M, N], allow bool [N] or [M, N] -> (val fp32 [M, K], idx int64 [M, K]): per row, delete the disallowed columns,
    ``np.argsort(-x, kind="stable")`` (larger first, equal values by smaller index, -0.0 == +0.0, NaN last), pad with (-inf, -1)."""
    M, N = x.shape
    allow = np.broadcast_to(allow, (M, N))
    val = np.full((M, K), -np.inf, np.float32)
    idx = np.full((M, K), -1, np.int64)
    for m in range(M):
        cols = np.flatnonzero(allow[m])
        row = x[m, cols]
        order = np.argsort(-row, kind="stable")[:K]
        val[m, :order.size] = row[order]
        idx[m, :order.size] = cols[order] + base
    return val, idx


def _before(a, i, b, j):
    """the total order of include/demovlp_hip.h spelt out: does (value a, index i) come before (value b, index j)?"""
    if np.isnan(a) or np.isnan(b):
        return (not np.isnan(a)) if np.isnan(a) != np.isnan(b) else i < j
    return a > b or (a == b and i < j)             # (IEEE: -0.0 == +0.0)


def brute_force(x, allow, K, base=0):
    M, N = x.shape
    allow = np.broadcast_to(allow, (M, N))
    val = np.full((M, K), -np.inf, np.float32)
    idx = np.full((M, K), -1, np.int64)
    for m in range(M):
        left = [c for c in range(N) if allow[m, c]]
        for p in range(min(K, len(left))):
            best = left[0]
            for c in left[1:]:
                if _before(x[m, c], c, x[m, best], best):
                    best = c
            left.remove(best)
            val[m, p], idx[m, p] = x[m, best], best + base
    return val, idx


def special_rows(M, N, seed):
    """Rows with what the order has to get right: values rounded to 1/8 (many ties, and -0.0), and from N = 5 on a NaN with sign and payload,
    a -inf and a +inf at fixed columns of every row (the masks below decide which of them are allowed)."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.standard_normal((M, N)) * 8) / 8).astype(np.float32)
    x[x == 0] = np.float32(-0.0)
    if N >= 5:
        x[:, 1] = np.float32(np.uint32(0xffc00123).view(np.float32))
        x[:, 2] = -np.inf
        x[:, N - 1] = np.inf
        x[:, N // 2] = x[:, 0]                                     # a duplicated value: a tie decided by the index
    return x


DENSITIES = ("all", "none", "one", "few", "half")


def allow_mask(M, N, K, density, per_row, seed):
    """bool [N] (shared) or [M, N]: all set | none | one bit | fewer than K (at most K - 1, at least 0) | random 50 %.  From N = 5 on, 'half'
    forces the NaN (1) and the -inf (2) in and the largest value (N - 1, +inf) out, so specials sit on both sides of the mask."""
    rng = np.random.default_rng(seed)
    shape = (M, N) if per_row else (1, N)
    if density == "all":
        a = np.ones(shape, bool)
    elif density == "none":
        a = np.zeros(shape, bool)
    elif density == "one":
        a = np.zeros(shape, bool)
        a[np.arange(shape[0]), rng.integers(0, N, shape[0])] = True
    elif density == "few":
        a = np.zeros(shape, bool)
        for r in range(shape[0]):
            a[r, rng.permutation(N)[:min(K - 1, N, 5)]] = True
    else:
        a = rng.random(shape) < 0.5
        if N >= 5:
            a[:, 1] = a[:, 2] = True
            a[:, N - 1] = False
    return a if per_row else a[0]


def _same(got, want):
    return np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


class TestReference:
    def test_masked_topk_reference_equals_a_brute_force_selection(self):
        for M, N, K in [(3, 1, 1), (3, 5, 7), (2, 33, 7), (2, 70, 1), (2, 70, 64)]:
            x = special_rows(M, N, N + K)
            for density in DENSITIES:
                for per_row in (False, True):
                    a = allow_mask(M, N, K, density, per_row, 3 * N + K)
                    for base in (0, 37):
                        ref, brute = masked_topk_ref(x, a, K, base), brute_force(x, a, K, base)
                        assert _same(ref, brute), (M, N, K, density, per_row, base)
                        n_allowed = np.broadcast_to(a, (M, N)).sum(1)
                        assert ((ref[1] >= 0).sum(1) == np.minimum(n_allowed, K)).all()
                        if density == "all":                           # nothing deleted: numpy's stable argsort of the whole row
                            order = np.argsort(-x, axis=1, kind="stable")[:, :K]
                            assert np.array_equal(ref[1][:, :order.shape[1]], order + base)
        # a larger value in a disallowed column is not listed; an allowed -inf is, with its index; -0.0 and +0.0 tie by index
        x = np.array([[5.0, -np.inf, 0.0, -0.0, 9.0]], np.float32)
        val, idx = masked_topk_ref(x, np.array([False, True, True, True, False]), 4)
        assert idx.tolist() == [[2, 3, 1, -1]] and val.view(np.uint32).tolist() == [[0, 0x80000000, 0xff800000, 0xff800000]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C entry and its wrappers
# ---------------------------------------------------------------------------------------------------------------------------------------
class TestEntryAndWrappers:
    def test_both_libraries_export_the_masked_entry_and_it_refuses_bad_arguments_before_any_launch(self):
        for path in (_lib.LIB_PATH, _lib.DEV_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), "dvlp_topk_rows_masked"), path
        assert "dvlp_topk_rows_masked" in _lib.exported_symbols()
        fn = _lib.load().dvlp_topk_rows_masked
        ok = dict(M=2, N=100, x=ONE, ld=100, K=10, base=0, allow=ONE, ald=4, val=ONE, idx=ONE, merge=0, ws=ONE)
        bad = [dict(K=0), dict(K=1025), dict(M=0), dict(N=0), dict(N=1 << 31), dict(ld=99), dict(base=-1), dict(base=(1 << 31) - 50),
               dict(merge=2), dict(x=None), dict(val=None), dict(idx=None), dict(ws=None), dict(x=ONE + 2),
               dict(allow=None), dict(ald=-1), dict(allow=ONE + 2), dict(ald=3), dict(base=37, ald=4)]      # (100 bits need 4 words, 137 need 5)
        for b in bad:
            a = {**ok, **b}
            args = (a["M"], a["N"], a["x"], a["ld"], a["K"], a["base"], a["allow"], a["ald"], a["val"], a["idx"], a["merge"], a["ws"], None)
            assert fn(*args) == ERR_SHAPE, b
            with pytest.raises(DemoVLPHipError):
                _lib.call("dvlp_topk_rows_masked", *args)

    def test_masked_wrapper_refuses_host_tensors_and_malformed_masks(self):
        x = torch.zeros(3, 50)
        words = torch.zeros(2, dtype=torch.int32).view(torch.uint32)
        with pytest.raises(DemoVLPHipError, match="MI355X"):
            ops.topk_rows_masked(x, 5, words)                                              # well-formed, but on the host
        for allow in (torch.zeros(2, dtype=torch.int64), torch.zeros(50, dtype=torch.bool), torch.zeros(4, 2, dtype=torch.int32), None,
                      torch.zeros(3, 4, dtype=torch.int32)[:, ::2]):
            with pytest.raises(DemoVLPHipError, match="allow"):
                ops.topk_rows_masked(x, 5, allow)
        with pytest.raises(DemoVLPHipError, match="bits"):
            ops.topk_rows_masked(x, 5, words[:1])                                          # 32 bits for 50 columns
        with pytest.raises(DemoVLPHipError, match="bits"):
            ops.topk_rows_masked(x, 5, words, index_base=20)                               # 64 bits, the columns end at 70
        with pytest.raises(DemoVLPHipError):
            ops.topk_rows_masked(x, 5, words, merge=True)

    def test_pack_allow_bits_against_a_bit_by_bit_loop(self):
        rng = np.random.default_rng(0)
        for n in (1, 31, 32, 33, 100):
            for shape in ((n,), (3, n)):
                a = rng.random(shape) < 0.5
                a[..., n - 1] = True                                                       # (the top bit of a full word: no sign trouble)
                got = ops.pack_allow_bits(torch.from_numpy(a))
                words = (n + 31) // 32
                assert got.dtype == torch.uint32 and tuple(got.shape) == shape[:-1] + (words,)
                want = np.zeros(shape[:-1] + (words,), np.uint32)
                for pos in np.ndindex(*shape):
                    if a[pos]:
                        want[pos[:-1] + (pos[-1] >> 5,)] |= np.uint32(1) << np.uint32(pos[-1] & 31)
                assert np.array_equal(got.numpy(), want), (n, shape)
                assert np.array_equal(search._unpack_bits(got, n).numpy(), a)              # and back
        for bad in (torch.zeros(4), torch.zeros(2, 2, 2, dtype=torch.bool), torch.zeros(0, dtype=torch.bool)):
            with pytest.raises(ValueError):
                ops.pack_allow_bits(bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the index classes
# ---------------------------------------------------------------------------------------------------------------------------------------
TEXT = dict(input_ids=torch.zeros(2, 13, dtype=torch.long), attention_mask=torch.ones(2, 13, dtype=torch.long))
VIDEOS = dict(object=torch.zeros(2, 4, 9, 6), object_mask=torch.ones(2, 4, 9))


def _video_out(n, G):
    return dict(global_object_embeddings=torch.zeros(n, 256, dtype=torch.bfloat16), local_object_embeddings=torch.zeros(n, G, 256, dtype=torch.bfloat16),
                object_mask=torch.zeros(n, G))


def _as_if_filled(ix, n=50):
    ix.n = n                   # (the checks below are host logic: none of them reaches the device)
    return ix


class TestIndexHostChecks:
    def test_allow_of_the_wrong_shape_dtype_or_device_is_a_value_error_naming_the_shape(self):
        loss = RWALoss(20, "equal")
        vix = _as_if_filled(search.VideoIndex(64, 36, torch.bfloat16, device="cpu"))
        cix = _as_if_filled(search.CaptionIndex(64, 12, torch.bfloat16, device="cpu", tiled=True))
        wrong = [torch.ones(49, dtype=torch.bool), torch.ones(3, 50, dtype=torch.bool), torch.ones(50), torch.ones(50, dtype=torch.uint8),
                 torch.ones(2, 50, 1, dtype=torch.bool), [True] * 50]
        for allow in wrong:
            calls = [lambda: vix.search(None, loss, TEXT, k=5, shortlist=10, allow=allow),
                     lambda: vix.shortlist_by_cosine(torch.zeros(2, 256), 10, allow=allow),
                     lambda: cix.search(None, loss, VIDEOS, k=5, shortlist=10, allow=allow),
                     lambda: cix.shortlist_by_cosine(torch.zeros(2, 256), 10, allow=allow),
                     lambda: cix.timeline(None, loss, VIDEOS, 4, 2, k=5, shortlist=10, allow=allow)]
            for fn in calls:
                with pytest.raises(ValueError, match=r"\[50\].*\[2, 50\]"):
                    fn()
        # a well-formed mask on the host for an index on the device: the same error; on a host index it passes and the device is asked for
        on_device = _as_if_filled(search.VideoIndex(64, 36, torch.bfloat16, device="cuda"))
        for allow in (torch.ones(50, dtype=torch.bool), torch.ones(2, 50, dtype=torch.bool)):
            with pytest.raises(ValueError, match="on cuda"):
                on_device.search(None, loss, TEXT, k=5, shortlist=10, allow=allow)
            with pytest.raises(DemoVLPHipError):
                vix.search(None, loss, TEXT, k=5, shortlist=10, allow=allow)
            with pytest.raises(DemoVLPHipError):
                cix.search(None, loss, VIDEOS, k=5, shortlist=10, allow=allow)
        # k is checked against the shortlist, not against the filter
        with pytest.raises(ValueError, match="shortlist"):
            vix.search(None, loss, TEXT, k=11, shortlist=10, allow=torch.ones(50, dtype=torch.bool))

    def test_remove_and_replace_refuse_rows_outside_the_index(self):
        vix = _as_if_filled(search.VideoIndex(64, 36, torch.bfloat16, device="cpu"))
        cix = _as_if_filled(search.CaptionIndex(64, 12, torch.bfloat16, device="cpu"))
        for ix in (vix, cix):
            for ids in ([50], [3, -1], torch.tensor([0, 63])):
                with pytest.raises(ValueError, match=r"outside \[0, len\(index\) = 50\)"):
                    ix.remove(ids)
            assert ix.alive is None and ix.live == 50 and ix.removed().numel() == 0 and ix.removed().dtype == torch.int64 and len(ix) == 50
            assert ix.remove([]) is ix and ix.alive is None
        with pytest.raises(ValueError, match="outside"):
            vix.replace([50], _video_out(1, 36))                                           # 50 is the next free row: that is ``add``'s
        with pytest.raises(ValueError, match="outside"):
            cix.replace([3, 50], torch.zeros(2, 256, dtype=torch.bfloat16), torch.zeros(2, 12, 256, dtype=torch.bfloat16), torch.ones(2, 13))
        with pytest.raises(ValueError, match="2 rows for 1"):
            vix.replace([3, 4], _video_out(1, 36))
        with pytest.raises(ValueError, match="G = 36"):
            vix.replace([3], _video_out(1, 37))                                            # ``add``'s checks hold
        with pytest.raises(DemoVLPHipError):
            vix.replace([3], _video_out(1, 36))                                            # well-formed, but on the host
        with pytest.raises(DemoVLPHipError):
            cix.replace([3], torch.zeros(1, 256, dtype=torch.bfloat16), torch.zeros(1, 12, 256, dtype=torch.bfloat16), torch.ones(1, 13))
        # the capacity check is ``add``'s alone: replacing rows of a full index is not "adding past the capacity"
        full = _as_if_filled(search.VideoIndex(50, 36, torch.bfloat16, device="cpu"))
        with pytest.raises(DemoVLPHipError):
            full.replace([3], _video_out(1, 36))

    def test_the_new_keywords_and_methods_are_in_the_signatures(self):
        for fn in (search.VideoIndex.search, search.VideoIndex.shortlist_by_cosine, search.CaptionIndex.search,
                   search.CaptionIndex.shortlist_by_cosine, search.CaptionIndex.timeline):
            par = inspect.signature(fn).parameters
            assert "allow" in par and par["allow"].default is None, fn.__qualname__
        assert "mask" in inspect.signature(search._ResidentIndex._global_stage).parameters
        assert list(inspect.signature(search.VideoIndex.replace).parameters) == ["self", "rows", "out"]
        assert list(inspect.signature(search.CaptionIndex.replace).parameters) == ["self", "rows", "global_text", "local_text", "attention_mask"]
        for cls in (search.VideoIndex, search.CaptionIndex):
            assert callable(cls.remove) and callable(cls.removed) and isinstance(inspect.getattr_static(cls, "live"), property)
        assert list(inspect.signature(ops.topk_rows_masked).parameters)[:3] == ["x", "K", "allow"]
        assert list(inspect.signature(ops.topk_rows).parameters) == ["x", "K", "N", "index_base", "out", "merge"]      # the existing wrapper is what it was
