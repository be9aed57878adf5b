"""DistilBERT self-attention (`dvlp_attention_fwd_ex` / `dvlp_attention_bwd_ex`, mode 1) on a real MI355X, element-wise against the
float64 oracle: every length branch of the bf16 dispatch and both sides of every 16-row tile edge, ragged per-sample key masks, dropout of
the attention probabilities (Philox keep masks shared with the oracle), and the packed `[B*L, 2304]` strides `BertLayerFn` runs at.

Branches (csrc/attention.hip, by cdiv(L, 16); fp32 always takes the generic wave-per-query kernels):
    forward   L <= 48 mattn_fwd<3,3> . 49..96 generic . 97..112 mattn_fwd<2,7> . 113..128 mattn_fwd<2,8>
    backward  L <= 32 generic . 33..48 mattn_bwd_full<3> . 49..96 generic . 97..112 mattn_bwd_full<7> . 113..128 mattn_bwd_full<8>

Error measure: per TOKEN ROW, max|got - ref| over the row / max(1, max|ref| over the row), maximum over rows -- a few wrong rows cannot hide
behind a matrix-wide maximum.  Bars are the project's own (`test_gpu_kernels.py`): fp32 1e-4, bf16 3e-2, forward 1x, each gradient 2x; dropout
only multiplies probabilities by 0 or 1 / (1 - p) and earns no wider bar.  The reference gets exactly the values the kernel gets (the bf16
inputs cast to double).  `-s` prints the maximum of every case and, at the end, per (dtype, branch, p, quantity): the figures for DESIGN.md section 4.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from demovlp_amd import ops  # noqa: E402
from oracle import restatement as orc  # noqa: E402

DEV = "cuda"
F32_TOL = 1e-4
BF16_TOL = 3e-2
B, D = 3, 768
SEED, OFFSET, SITE = 0x1234567890, 3, 7          # Philox state of the keep masks: a seed wider than 32 bits, a non-zero offset, a site other than 0
LENGTHS = [1, 5, 16, 17, 32, 33, 48, 49, 80, 96, 97, 112, 113, 128]
BRANCH_LENGTHS = [16, 40, 80, 100, 128]          # one length per branch (forward and backward) for the bit-exact checks
GUARD_LENGTHS = [1, 17, 33, 49, 97, 113]
DTYPES = [torch.float32, torch.bfloat16]
DROPS = [None, 0.1, 0.5]
GUARD = 16                                       # one 16-row tile: the most a padded tile could spill
SENTINEL = 24576.0                               # finite, exact in bf16

dtype_id = lambda d: "f32" if d == torch.float32 else "bf16"
drop_id = lambda p: "nodrop" if p is None else f"p{p}"
on_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)


def tol(dtype):
    return F32_TOL if dtype == torch.float32 else BF16_TOL


def fwd_branch(dtype, L):
    if dtype == torch.float32:
        return "attn_fwd<f32>"
    return "mattn_fwd<3,3>" if L <= 48 else "attn_fwd<bf16>" if L <= 96 else "mattn_fwd<2,7>" if L <= 112 else "mattn_fwd<2,8>"


def bwd_branch(dtype, L):
    if dtype == torch.float32:
        return "attn_bwd_seg<f32>"
    if L <= 32 or 49 <= L <= 96:
        return "attn_bwd_seg<bf16>"
    return "mattn_bwd_full<3>" if L <= 48 else "mattn_bwd_full<7>" if L <= 112 else "mattn_bwd_full<8>"


# ------------------------------------------------------------------------------------------------------------------
# inputs, masks and the float64 reference: computed once per case and shared (nothing below writes to them)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(dtype, L):
    g = torch.Generator().manual_seed(1000 + L)
    q, k, v = ((torch.randn(B * L, D, generator=g) * 1.5).to(dtype).to(DEV) for _ in range(3))
    dout = torch.randn(B * L, D, generator=g).to(dtype).to(DEV)
    att = torch.zeros(B, L, dtype=torch.long)                # ragged prefix masks: full, a third, the CLS position only
    att[0, :] = 1
    att[1, :max(1, L // 3)] = 1
    att[2, :1] = 1
    addmask = torch.zeros(B, L).masked_fill(att == 0, float("-inf")).to(DEV)
    return {"q": q, "k": k, "v": v, "dout": dout, "att": att, "addmask": addmask}


def keep_masks(L, p, offset=OFFSET):
    state = ops.dropout_state(torch.device(DEV), SEED)
    for _ in range(offset):
        ops.dropout_advance(state)
    return ops.attn_keep_masks(B, L, p, state, SITE, torch.device(DEV))


@functools.lru_cache(maxsize=None)
def device_keep(L, p):
    return keep_masks(L, p)


@functools.lru_cache(maxsize=None)
def oracle_keep(L, p):
    return torch.from_numpy(orc.dropout_keep_attention(B, L, p, SEED, OFFSET, SITE))              # [B, H, L, L] 0 / 1


@functools.lru_cache(maxsize=None)
def reference(dtype, L, p):
    """(out, dq, dk, dv) [B*L, 768] float64 on the CPU, from the values the kernel gets."""
    x = inputs(dtype, L)
    q, k, v = (x[n].cpu().double().reshape(B, L, D).requires_grad_(True) for n in "qkv")
    keep = None if p is None else oracle_keep(L, p).double()
    out = orc.text_attention(q, k, v, x["att"], keep=keep, p_drop=0.0 if p is None else p)
    out.backward(x["dout"].cpu().double().reshape(B, L, D))
    return tuple(t.detach().reshape(B * L, D) for t in (out, q.grad, k.grad, v.grad))


def run(x, L, keep, ld=768, out=None, ld_out=768, qkv=None):
    q, k, v = qkv if qkv is not None else (x["q"], x["k"], x["v"])
    o = ops.full_attention_fwd(q, k, v, x["addmask"], B, L, ld=ld, keep=keep)
    dq, dk, dv = ops.full_attention_bwd(q, k, v, x["addmask"], x["dout"], B, L, ld=ld, out=out, ld_out=ld_out, keep=keep)
    return o, dq, dk, dv


def packed(x):
    """q | k | v as the three column blocks of one [B*L, 2304] projection."""
    qkv = torch.cat([x["q"], x["k"], x["v"]], dim=1).contiguous()
    return qkv[:, :768], qkv[:, 768:1536], qkv[:, 1536:]


def row_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    e = (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1.0)
    return float(e.max()) if bool(torch.isfinite(got).all()) else float("nan")


MAXIMA = {}      # (dtype, branch, p, quantity) -> largest per-row error seen


@pytest.fixture(scope="module", autouse=True)
def _print_maxima():
    yield
    if MAXIMA:
        print("\ntext attention, per-row error maxima by (dtype, branch, p):")
        for (dt_, br, p, what), e in sorted(MAXIMA.items()):
            print(f"  {dt_:4s} {br:20s} {p:7s} {what:3s} {e:.3e}")


# ------------------------------------------------------------------------------------------------------------------
# element-wise against float64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", DROPS, ids=drop_id)
@pytest.mark.parametrize("L", LENGTHS)
@on_dtypes
def test_text_attention_vs_float64(dtype, L, p):
    """out, dq, dk, dv of one case, every token row (rows of masked query positions included: the tower's LayerNorm reads them)."""
    x = inputs(dtype, L)
    keep = None if p is None else device_keep(L, p)
    if p is not None:                   # the test really exercises dropout, with the masks the reference uses
        kd, kTd, scale = keep
        Ns = (L + 15) // 16 * 16
        want = oracle_keep(L, p).reshape(B * ops.HEADS, L, L).to(torch.uint8)
        kd, kTd = kd.cpu(), kTd.cpu()
        assert kd.shape == kTd.shape == (B * ops.HEADS, Ns, Ns) and abs(scale - 1.0 / (1.0 - p)) < 1e-12
        assert torch.equal(kd[:, :L, :L], want), "keep bytes differ from the oracle's Philox mask"
        assert torch.equal(kTd[:, :L, :L], want.transpose(1, 2)), "transposed keep bytes differ from the oracle's mask"
        for m in (kd, kTd):
            assert int(m[:, L:, :].sum()) == 0 and int(m[:, :, L:].sum()) == 0, "pad rows / columns of the keep bytes are not 0"
        if L >= 5:
            assert 0 < int(want.sum()) < want.numel(), "the mask does not hold both 0 and 1"
    out, dq, dk, dv = run(x, L, keep)
    if p is not None and L >= 5:
        assert not torch.equal(out, ops.full_attention_fwd(x["q"], x["k"], x["v"], x["addmask"], B, L)), "dropout changed nothing"
    ref = reference(dtype, L, p)
    bad = []
    for name, got, r, mult, br in (("out", out, ref[0], 1, fwd_branch(dtype, L)), ("dq", dq, ref[1], 2, bwd_branch(dtype, L)),
                                   ("dk", dk, ref[2], 2, bwd_branch(dtype, L)), ("dv", dv, ref[3], 2, bwd_branch(dtype, L))):
        e = row_err(got, r)
        print(f"text-attn {dtype_id(dtype)} L={L} {drop_id(p)} {name:3s} [{br}] per-row err {e:.3e} (bar {tol(dtype) * mult:.0e})")
        key = (dtype_id(dtype), br, drop_id(p), name)
        MAXIMA[key] = e if e != e else max(MAXIMA.get(key, 0.0), e)          # (a NaN stays)
        if not e < tol(dtype) * mult:
            bad.append(f"{name} {e:.3e} >= {tol(dtype) * mult:.0e} [{br}]")
    assert not bad, f"{dtype_id(dtype)} L={L} {drop_id(p)}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# bit-exact: no tolerance
# ------------------------------------------------------------------------------------------------------------------
NAMES = ("out", "dq", "dk", "dv")


@pytest.mark.parametrize("p", [None, 0.1], ids=drop_id)
@pytest.mark.parametrize("L", BRANCH_LENGTHS)
@on_dtypes
def test_packed_projection_equals_three_tensors(dtype, L, p):
    """ld = ld_out = 2304 (the column blocks of one packed projection, dq | dk | dv into one buffer) against ld = 768: the kernels have no
    atomics and the stride enters addresses only."""
    x = inputs(dtype, L)
    keep = None if p is None else device_keep(L, p)
    sep = run(x, L, keep)
    dqkv = torch.full((B * L, 2304), float("nan"), device=DEV, dtype=dtype)          # an element left unwritten compares unequal
    pk = run(x, L, keep, ld=2304, out=(dqkv[:, :768], dqkv[:, 768:1536], dqkv[:, 1536:]), ld_out=2304, qkv=packed(x))
    for name, a, b in zip(NAMES, sep, (pk[0], dqkv[:, :768], dqkv[:, 768:1536], dqkv[:, 1536:])):
        assert torch.equal(a, b), f"{name}: packed strides change the result ({dtype_id(dtype)} L={L} {drop_id(p)})"


@pytest.mark.parametrize("L", BRANCH_LENGTHS)
@on_dtypes
def test_all_ones_keep_masks_equal_no_masks(dtype, L):
    """p = 0 keep masks (all ones on the valid area, scale 1) against keep = None: isolates the row stride Ns and the pad clamps."""
    x = inputs(dtype, L)
    keep = keep_masks(L, 0.0)
    assert keep[2] == 1.0
    for m in keep[:2]:
        assert bool(m[:, :L, :L].all()) and int(m.sum()) == B * ops.HEADS * L * L
    for name, a, b in zip(NAMES, run(x, L, keep), run(x, L, None)):
        assert torch.equal(a, b), f"{name}: all-ones keep masks change the result ({dtype_id(dtype)} L={L})"


@pytest.mark.parametrize("L", BRANCH_LENGTHS)
@on_dtypes
def test_run_to_run_identical(dtype, L):
    x = inputs(dtype, L)
    keep = device_keep(L, 0.1)
    for name, a, b in zip(NAMES, run(x, L, keep), run(x, L, keep)):
        assert torch.equal(a, b), f"{name}: two calls on the same inputs differ ({dtype_id(dtype)} L={L})"


# ------------------------------------------------------------------------------------------------------------------
# guard rows around every output
# ------------------------------------------------------------------------------------------------------------------
def guarded(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), SENTINEL, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("p", [None, 0.1], ids=drop_id)
@pytest.mark.parametrize("layout", ["separate", "packed"])
@pytest.mark.parametrize("L", GUARD_LENGTHS)
@on_dtypes
def test_outputs_stay_inside_their_rows(dtype, L, layout, p):
    """out and dq / dk / dv are views into larger buffers with 16 sentinel rows before and after: a padded tile writes none of them, and what
    lands inside is what the allocating wrappers return."""
    x = inputs(dtype, L)
    keep = None if p is None else device_keep(L, p)
    ld = 768 if layout == "separate" else 2304
    q, k, v = (x["q"], x["k"], x["v"]) if layout == "separate" else packed(x)
    obuf, out = guarded(B * L, 768, dtype)
    ext = ops.AttnExt(keep=keep[0].data_ptr(), keepT=keep[1].data_ptr(), keep_scale=float(keep[2])) if keep is not None else ops.AttnExt()
    ops.call("dvlp_attention_fwd_ex", ops.dt(dtype), 1, B, L, ops.HEADS, 1, L, ops.p(q), ops.p(k), ops.p(v), ld, ops.p(x["addmask"]), ops.p(out),
             768, ops.SCALE, None, None, ctypes.byref(ext), ops.stream())
    if layout == "separate":
        gbufs, grads = zip(*(guarded(B * L, 768, dtype) for _ in range(3)))
    else:
        gbuf, dqkv = guarded(B * L, 2304, dtype)
        gbufs, grads = (gbuf,), (dqkv[:, :768], dqkv[:, 768:1536], dqkv[:, 1536:])
    ops.full_attention_bwd(q, k, v, x["addmask"], x["dout"], B, L, ld=ld, out=grads, ld_out=ld, keep=keep)
    assert guards_intact(obuf), f"forward wrote outside its rows ({dtype_id(dtype)} L={L} {layout} {drop_id(p)})"
    for name, buf in zip(("dq", "dk", "dv") if layout == "separate" else ("dq | dk | dv",), gbufs):
        assert guards_intact(buf), f"backward wrote outside the rows of {name} ({dtype_id(dtype)} L={L} {layout} {drop_id(p)})"
    for name, a, b in zip(NAMES, (out, *grads), run(x, L, keep)):
        assert torch.equal(a, b), f"{name}: the guarded call differs from the plain one ({dtype_id(dtype)} L={L} {layout} {drop_id(p)})"
