"""``dvlp_attention_*`` mode 0 (VarAttention: space attention, and time attention on the region-major token order) restated in float64
torch, segment by segment (the definition of include/demovlp_hip.h, not the kernels' tiles and not the oracle's N x N structural mask),
with the head count as a parameter.  Token 0 (CLS) attends to every key; token ``1 + s*R + r`` attends to token 0 and to the R tokens of
its own segment s.  Also: which kernels `csrc/attention.hip` launches for a (dtype, R, route).  Shared by
``tests/test_space_attention_ref.py`` (which pins both, on the CPU) and ``tests/test_gpu_space_attention.py`` (which holds the kernels to it)."""
import torch

HEAD_DIM = 64
ROUTES = ("fold", "plain", "three-launch", "round4")
MFMA_TILES = ((1, 1), (2, 2), (3, 3), (1, 2), (2, 3))          # the (query tiles, key tiles) instances of the plain / three-launch kernels


def space_attention_ref(q, k, v, addmask, S, R, heads):
    """q, k, v [B, N, heads*64] (N = 1 + S*R), addmask [B, N] additive over keys -> out [B, N, heads*64] and the CLS query's softmax
    statistics (max [B, heads], sum of exp(score - max) [B, heads]).  Differentiable in q, k, v."""
    B, N, _ = q.shape
    assert N == 1 + S * R and addmask.shape == (B, N)
    q, k, v = (t.reshape(B, N, heads, HEAD_DIM).transpose(1, 2) for t in (q, k, v))              # [B, H, N, 64]
    m = addmask.to(q.dtype)
    scale = HEAD_DIM ** -0.5
    # the CLS query: every key of the clip
    s0 = (q[:, :, :1] * scale) @ k.transpose(-1, -2) + m[:, None, None, :]                         # [B, H, 1, N]
    mx = s0.amax(-1, keepdim=True)
    e0 = torch.exp(s0 - mx)
    sm = e0.sum(-1, keepdim=True)
    o0 = (e0 / sm) @ v                                                                             # [B, H, 1, 64]
    # the segment queries: the CLS key, then the keys of the query's own segment
    qs, ks, vs = (t[:, :, 1:].reshape(B, heads, S, R, HEAD_DIM) for t in (q, k, v))
    sc = (qs * scale * k[:, :, None, :1]).sum(-1, keepdim=True) + m[:, None, None, None, :1]      # [B, H, S, R, 1]
    ss = (qs * scale) @ ks.transpose(-1, -2) + m[:, 1:].reshape(B, 1, S, 1, R)                     # [B, H, S, R, R]
    a = torch.softmax(torch.cat([sc, ss], -1), -1)
    os_ = a[..., :1] * v[:, :, None, :1] + a[..., 1:] @ vs                                         # [B, H, S, R, 64]
    out = torch.cat([o0, os_.reshape(B, heads, S * R, HEAD_DIM)], 2).transpose(1, 2).reshape(B, N, heads * HEAD_DIM)
    return out, (mx[:, :, 0, 0].detach(), sm[:, :, 0, 0].detach())


def to_segment_major(x, F, R):
    """[B, 1 + F*R, ...] frame-major tokens -> region-major ('b (f n) d -> b (n f) d'), CLS in place; (R, F) transposes back."""
    B = x.shape[0]
    body = x[:, 1:].reshape(B, F, R, *x.shape[2:]).transpose(1, 2).reshape(B, F * R, *x.shape[2:])
    return torch.cat([x[:, :1], body], 1)


def tiles(R):
    return (R + 15) // 16, (R + 16) // 16           # query tiles of the R segment rows, key tiles of CLS + R keys


def folds(dtype, R):
    """Does the forward fold the CLS query into the frame waves (and return statistics)?  It needs a free query row in the last tile."""
    nqt, nkt = tiles(R)
    return dtype == torch.bfloat16 and nqt == nkt and R <= 47


def admits(dtype, R, route):
    if dtype == torch.float32:
        return route == "plain"
    return folds(dtype, R) if route in ("fold", "round4") else True


def fwd_branch(dtype, R, route):
    assert route in ROUTES and admits(dtype, R, route)
    if dtype == torch.float32:
        return "attn_fwd<f32>"
    nqt, nkt = tiles(R)
    if route == "fold":
        return f"sattn_fwd<{nkt}>"
    if route == "round4":
        return f"mattn_fwd<{nqt},{nkt}>+combine"
    return f"mattn_fwd<{nqt},{nkt}>" if (nqt, nkt) in MFMA_TILES else "attn_fwd<bf16>"


def bwd_branch(dtype, R, route):
    assert route in ROUTES and admits(dtype, R, route)
    if dtype == torch.float32:
        return "attn_bwd_seg<f32>+attn_bwd_cls<f32>"
    nqt, nkt = tiles(R)
    if route == "fold":
        return f"sattn_bwd<{nkt}>"
    if route == "round4":
        return f"mattn_bwd_space_merged<{nkt}>/fwd-stats"
    if route == "plain" and R <= 47:
        return f"cls_pre+mattn_bwd_space_merged<{nkt}>"
    if route == "three-launch" and (nqt, nkt) in MFMA_TILES:
        return f"mattn_bwd_space<{nqt},{nkt}>+attn_bwd_cls"
    return "attn_bwd_seg<bf16>+attn_bwd_cls<bf16>"
