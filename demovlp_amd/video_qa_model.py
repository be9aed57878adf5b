"""BUTD question-answering head: drop-in mirror of model/video_qa_mdoel.py:78-97 (`BUTDQAHead` and its FCNet / Attention /
SimpleClassifier parts; same sub-module names, so the `head.*` state_dict keys -- weight-normalised linears with `weight_g` /
`weight_v` -- interchange with reference checkpoints).

This head is a downstream classifier on top of the two towers, ~0.5 MFLOP per sample on [B, 256]
vectors: it runs on PyTorch-ROCm's stock kernels; the towers underneath are the hand-written HIP path.  Dropout layers of the
reference head (p = 0.2 in Attention, 0 elsewhere) follow module.train()/eval() as usual.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.nn.utils import weight_norm


def _fc(dims, norm=True):
    layers = []
    for a, b in zip(dims[:-1], dims[1:]):
        lin = nn.Linear(a, b)
        layers += [weight_norm(lin, dim=None) if norm else lin, nn.ReLU()]
    return layers


class FCNet(nn.Module):
    def __init__(self, dims, dropout=0.0, norm=True):
        super().__init__()
        self.main = nn.Sequential(*_fc(dims, norm))

    def forward(self, x):
        return self.main(x)


class SimpleClassifier(nn.Module):
    def __init__(self, in_dim, hid_dim, out_dim, dropout=0.0):
        super().__init__()
        self.q_net = FCNet([in_dim[0], hid_dim[0]], dropout)
        self.v_net = FCNet([in_dim[1], hid_dim[0]], dropout)
        self.main = nn.Sequential(nn.Linear(hid_dim[0], hid_dim[1]), nn.ReLU(), nn.Dropout(dropout, inplace=True), nn.Linear(hid_dim[1], out_dim))

    def forward(self, q_emb, v_emb):
        return self.main(self.q_net(q_emb) * self.v_net(v_emb))


class Attention(nn.Module):
    def __init__(self, v_dim, q_dim, hid_dim, glimpses=1, dropout=0.2):
        super().__init__()
        self.v_proj = FCNet([v_dim, hid_dim], dropout)
        self.q_proj = FCNet([q_dim, hid_dim], dropout)
        self.drop = nn.Dropout(dropout)
        self.linear = weight_norm(nn.Linear(hid_dim, glimpses), dim=None)

    def forward(self, v, v_mask, q):
        """v [B, k, v_dim], v_mask [B, k] (1 = real region), q [B, q_dim] -> (softmax over k of the masked logits, logits)."""
        logits = self.linear(self.drop(self.v_proj(v) * self.q_proj(q).unsqueeze(1)))
        logits = logits * v_mask.unsqueeze(-1)          # the reference MULTIPLIES by the 0/1 mask (padded regions keep logit 0)
        return torch.softmax(logits, 1), logits


class BUTDQAHead(nn.Module):
    """``impl="stock"`` (default): PyTorch-ROCm's stock kernels, as before.  ``impl="hip"``: the kernels of csrc/qahead.hip -- one launch folds
    the five weight-normalised linears, the region attention runs fused (bf16, G <= 288: H stays on chip), the classifier's small products are
    dvlp_gemm launches; like every op of the package it raises on CPU tensors.  In train mode the HIP path draws the Attention dropout's
    keep bits from a Philox state of its own (``seed_dropout``) at site ``ops.QA_HEAD_DROPOUT_SITE``."""

    def __init__(self, v_dim, q_dim, hid_dim, out_dim, impl="stock"):
        super().__init__()
        if impl not in ("stock", "hip"):
            raise ValueError(f"impl must be 'stock' or 'hip', got {impl!r}")
        if impl == "hip" and not (v_dim == q_dim == hid_dim == 256):
            raise ValueError("impl='hip' is built for v_dim = q_dim = hid_dim = 256 (the only widths the reference configures)")
        self.impl = impl
        self.v_att = Attention(v_dim, q_dim, hid_dim)
        self.classifier = SimpleClassifier([q_dim, v_dim], [hid_dim, hid_dim * 2], out_dim)
        self.dropout_seed, self._drop_state, self.last_att = 0, None, None

    def seed_dropout(self, seed):
        self.dropout_seed, self._drop_state = int(seed), None

    def dropout_state(self, device):
        """Device-resident Philox state of the HIP path's Attention dropout (advanced once per train-mode forward)."""
        from . import ops
        if self._drop_state is None or self._drop_state.device != device:
            self._drop_state = ops.dropout_state(device, self.dropout_seed)
        return self._drop_state

    def forward(self, txt_embed, obj_embed, obj_mask):
        if self.impl == "hip":
            return self._forward_hip(txt_embed, obj_embed, obj_mask)
        att, _ = self.v_att(obj_embed, obj_mask, txt_embed)
        return self.classifier(txt_embed, (att * obj_embed).sum(1))

    def _forward_hip(self, q, v, mask):
        """q [B, 256] fp32, v [B, G, 256] in the towers' compute dtype (any row-strided view), mask [B, G] 0/1 -> logits [B, out_dim] fp32."""
        from . import functional as Fn, ops
        ops.require_gpu(q, v, mask)
        a, c = self.v_att, self.classifier
        wn = [a.v_proj.main[0], a.q_proj.main[0], a.linear, c.q_net.main[0], c.v_net.main[0]]
        want_b = (0,) if v.dtype == torch.bfloat16 else ()
        folded = Fn.WeightNormFoldFn.apply(want_b, *[t for m in wn for t in (m.weight_v, m.weight_g)])
        Wv, Wq, wl, Wqn, Wvn = folded[:5]
        Wv_b = folded[5] if want_b else None
        drop = None
        p_drop = float(a.drop.p)
        if self.training and p_drop > 0.0:
            state = self.dropout_state(v.device)
            ops.dropout_advance(state)
            drop = (p_drop, state, ops.QA_HEAD_DROPOUT_SITE)
        pooled, self.last_att = Fn.QAAttendFn.apply(v, mask, q.float(), Wq, wn[1].bias, Wv, Wv_b, wn[0].bias, wl, wn[2].bias, drop)
        qn = Fn.PlainLinearFn.apply(q.float(), Wqn, wn[3].bias)
        vn = Fn.PlainLinearFn.apply(pooled, Wvn, wn[4].bias)
        joint = torch.relu(qn) * torch.relu(vn)
        l0, l3 = c.main[0], c.main[3]
        h = Fn.LinearFn.apply(joint, l0.weight, l0.bias, None)
        return Fn.LinearFn.apply(torch.relu(h), l3.weight, l3.bias, h)
