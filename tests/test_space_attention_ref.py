"""Pins ``tests/space_attention_ref.py`` on the CPU: the segment-by-segment float64 restatement of mode 0 equals the oracle's N x N
structural-mask form (space attention, and time attention through the region-major token order), and the kernel-naming helper
equals a table written by hand from the dispatch of csrc/attention.hip."""
import pytest
import torch

import space_attention_ref as sar
from oracle import restatement as orc

BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(2, 3, 17), (3, 4, 5), (2, 16, 30)]          # (B, frames, regions)


def case(B, F, R, seed):
    g = torch.Generator().manual_seed(seed)
    N = 1 + F * R
    qkv = (torch.randn(B, N, 2304, generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    mask01 = (torch.rand(B, F, R, generator=g) > 0.3).double()
    mask01[0, F // 2] = 0                                # a fully masked frame
    mask01[-1, :, R // 2] = 0                            # a region slot masked in every frame
    addmask = torch.cat([torch.zeros(B, 1, dtype=torch.float64), (mask01.reshape(B, -1) - 1) * 100], 1)
    dout = torch.randn(B, N, 768, generator=g, dtype=torch.float64)
    return qkv, addmask, dout


def split(qkv):
    return qkv[..., :768], qkv[..., 768:1536], qkv[..., 1536:]


@pytest.mark.parametrize("B,F,R", SHAPES)
def test_restatement_equals_the_oracle_space_attention(B, F, R):
    qkv, addmask, dout = case(B, F, R, 1)
    want = orc.space_attention(qkv, addmask, F, R)
    want.backward(dout)
    gwant, qkv.grad = qkv.grad, None
    got, (mx, sm) = sar.space_attention_ref(*split(qkv), addmask, F, R, 12)
    got.backward(dout)
    assert float((got - want).detach().abs().max()) < 1e-12 and float((qkv.grad - gwant).abs().max()) < 1e-12
    s = (qkv.detach()[:, :1, :768].reshape(B, 1, 12, 64).transpose(1, 2) * 0.125) @ qkv.detach()[:, :, 768:1536].reshape(B, -1, 12, 64).permute(0, 2, 3, 1)
    s = s[:, :, 0] + addmask[:, None, :]
    assert float((mx - s.amax(-1)).abs().max()) < 1e-12
    assert float((sm - torch.exp(s - s.amax(-1, keepdim=True)).sum(-1)).abs().max()) < 1e-10


@pytest.mark.parametrize("B,F,R", SHAPES)
def test_restatement_on_the_region_major_order_is_time_attention(B, F, R):
    """(segments, length) = (regions, frames) on the transposed token order, transposed back: `space_attention(..., time=True)`."""
    qkv, addmask, dout = case(B, F, R, 2)
    want = orc.space_attention(qkv, addmask, F, R, time=True)
    want.backward(dout)
    gwant, qkv.grad = qkv.grad, None
    out_t, _ = sar.space_attention_ref(*split(sar.to_segment_major(qkv, F, R)), sar.to_segment_major(addmask, F, R), R, F, 12)
    got = sar.to_segment_major(out_t, R, F)
    got.backward(dout)
    assert float((got - want).detach().abs().max()) < 1e-12 and float((qkv.grad - gwant).abs().max()) < 1e-12
    x = torch.arange(2 * (1 + F * R) * 3, dtype=torch.float64).reshape(2, 1 + F * R, 3)
    assert torch.equal(sar.to_segment_major(sar.to_segment_major(x, F, R), R, F), x)


def test_head_count_is_a_parameter():
    """H = 3: each head of the restatement is the H = 1 restatement of its 64 columns."""
    g = torch.Generator().manual_seed(3)
    B, S, R = 2, 3, 5
    q, k, v = (torch.randn(B, 1 + S * R, 192, generator=g, dtype=torch.float64) for _ in range(3))
    m = torch.zeros(B, 1 + S * R, dtype=torch.float64)
    m[1, 4:9] = -100
    out, (mx, sm) = sar.space_attention_ref(q, k, v, m, S, R, 3)
    for h in range(3):
        c = slice(64 * h, 64 * h + 64)
        o1, (m1, s1) = sar.space_attention_ref(q[..., c], k[..., c], v[..., c], m, S, R, 1)
        assert float((out[..., c] - o1).abs().max()) < 1e-13 and float((mx[:, h] - m1[:, 0]).abs().max()) < 1e-13
        assert float((sm[:, h] - s1[:, 0]).abs().max()) < 1e-12


GEN_F, GEN_B = "attn_fwd<bf16>", "attn_bwd_seg<bf16>+attn_bwd_cls<bf16>"
PRE, ST, CLS = "cls_pre+mattn_bwd_space_merged", "mattn_bwd_space_merged", "+attn_bwd_cls"
# (R, route) -> (forward, backward), bf16; written by hand from dvlp_attention_fwd_ex / dvlp_attention_bwd_ex
TABLE = {
    (1, "fold"): ("sattn_fwd<1>", "sattn_bwd<1>"), (15, "fold"): ("sattn_fwd<1>", "sattn_bwd<1>"),
    (17, "fold"): ("sattn_fwd<2>", "sattn_bwd<2>"), (31, "fold"): ("sattn_fwd<2>", "sattn_bwd<2>"),
    (33, "fold"): ("sattn_fwd<3>", "sattn_bwd<3>"), (47, "fold"): ("sattn_fwd<3>", "sattn_bwd<3>"),
    (1, "plain"): ("mattn_fwd<1,1>", PRE + "<1>"), (15, "plain"): ("mattn_fwd<1,1>", PRE + "<1>"),
    (16, "plain"): ("mattn_fwd<1,2>", PRE + "<2>"), (17, "plain"): ("mattn_fwd<2,2>", PRE + "<2>"),
    (31, "plain"): ("mattn_fwd<2,2>", PRE + "<2>"), (32, "plain"): ("mattn_fwd<2,3>", PRE + "<3>"),
    (33, "plain"): ("mattn_fwd<3,3>", PRE + "<3>"), (47, "plain"): ("mattn_fwd<3,3>", PRE + "<3>"),
    (48, "plain"): (GEN_F, GEN_B), (49, "plain"): (GEN_F, GEN_B), (96, "plain"): (GEN_F, GEN_B), (97, "plain"): (GEN_F, GEN_B),
    (127, "plain"): (GEN_F, GEN_B),
    (15, "three-launch"): ("mattn_fwd<1,1>", "mattn_bwd_space<1,1>" + CLS), (16, "three-launch"): ("mattn_fwd<1,2>", "mattn_bwd_space<1,2>" + CLS),
    (31, "three-launch"): ("mattn_fwd<2,2>", "mattn_bwd_space<2,2>" + CLS), (32, "three-launch"): ("mattn_fwd<2,3>", "mattn_bwd_space<2,3>" + CLS),
    (47, "three-launch"): ("mattn_fwd<3,3>", "mattn_bwd_space<3,3>" + CLS), (48, "three-launch"): (GEN_F, GEN_B),
    (15, "round4"): ("mattn_fwd<1,1>+combine", ST + "<1>/fwd-stats"), (31, "round4"): ("mattn_fwd<2,2>+combine", ST + "<2>/fwd-stats"),
    (47, "round4"): ("mattn_fwd<3,3>+combine", ST + "<3>/fwd-stats"),
}
NO_FOLD = [16, 32, 48, 49, 96, 97, 127]                # the CLS row finds no free query row in the last tile, or R + 1 > 48


def test_branch_helper_matches_the_dispatch_table():
    for (R, route), (fwd, bwd) in TABLE.items():
        assert sar.admits(BF, R, route), (R, route)
        assert (sar.fwd_branch(BF, R, route), sar.bwd_branch(BF, R, route)) == (fwd, bwd), (R, route)
    for R in sorted({R for R, _ in TABLE}):
        assert sar.folds(BF, R) == (R not in NO_FOLD) and not sar.folds(F32, R)
        assert sar.admits(BF, R, "fold") == sar.admits(BF, R, "round4") == (R not in NO_FOLD)
        assert sar.admits(F32, R, "plain") and not any(sar.admits(F32, R, r) for r in ("fold", "three-launch", "round4"))
        assert sar.fwd_branch(F32, R, "plain") == "attn_fwd<f32>" and sar.bwd_branch(F32, R, "plain") == "attn_bwd_seg<f32>+attn_bwd_cls<f32>"
    # the frame counts of time attention land on the asymmetric instances
    assert sar.fwd_branch(BF, 16, "plain") == "mattn_fwd<1,2>" and sar.fwd_branch(BF, 32, "plain") == "mattn_fwd<2,3>"
