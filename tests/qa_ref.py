"""float64 restatements for the video-QA head tests (tests/test_gpu_qa.py): the pieces of ``oracle.restatement.qa_logits`` with the
train-mode keep mask of the head's Attention dropout written out (``orc.dropout_keep_flat`` at ``ops.QA_HEAD_DROPOUT_SITE``)."""
import numpy as np
import torch

from oracle import restatement as orc

WN = ("head.v_att.v_proj.main.0", "head.v_att.q_proj.main.0", "head.v_att.linear", "head.classifier.q_net.main.0", "head.classifier.v_net.main.0")


def fold(v, g):
    return g * v / v.norm()


def keep_scale(B, G, p, seed, offset, site):
    """keep / (1 - p) of the [B, G, 256] product inside Attention (flat element numbering), float64; all ones for p = 0."""
    if p <= 0.0:
        return torch.ones(B, G, 256, dtype=torch.float64)
    k = orc.dropout_keep_flat(B * G * 256, p, seed, offset, site).reshape(B, G, 256)
    return torch.from_numpy(k.astype(np.float64)) / (1.0 - float(np.float32(p)))


def attend(v, mask, q, Wq, bq, Wv, bv, wl, bl, ks=None):
    """Attention.forward + weighted sum on float64 tensors (folded weights) -> (pooled [B, 256], att [B, G])."""
    qp = torch.relu(q @ Wq.t() + bq)
    z = torch.relu(v @ Wv.t() + bv) * qp[:, None]
    if ks is not None:
        z = z * ks
    logit = (z @ wl.reshape(-1) + bl.reshape(())) * mask
    att = torch.softmax(logit, dim=1)
    return (att[..., None] * v).sum(1), att


def head_logits(p, q, v, mask, ks=None):
    """BUTDQAHead on float64 tensors; ``p`` maps state_dict names (``head.*``) to float64 tensors (leaves that may require grad)."""
    W = {n: fold(p[n + ".weight_v"], p[n + ".weight_g"]) for n in WN}
    b = {n: p[n + ".bias"] for n in WN}
    pooled, _ = attend(v, mask, q, W[WN[1]], b[WN[1]], W[WN[0]], b[WN[0]], W[WN[2]], b[WN[2]], ks)
    joint = torch.relu(q @ W[WN[3]].t() + b[WN[3]]) * torch.relu(pooled @ W[WN[4]].t() + b[WN[4]])
    h = torch.relu(joint @ p["head.classifier.main.0.weight"].t() + p["head.classifier.main.0.bias"])
    return h @ p["head.classifier.main.3.weight"].t() + p["head.classifier.main.3.bias"]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
