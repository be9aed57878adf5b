"""``dvlp_moment_select`` restated in numpy, row by row (the definition of include/demovlp_hip.h and DESIGN.md 6l, not the kernel's layout):
greedy temporal non-maximum suppression over the window scores of a pair.  float32 for the one multiply of the overlap test, the order of
``csrc/topk.hip`` for ties (by value with -0.0 == +0.0, then the smaller position).  Shared by ``tests/test_moment_hits.py`` (which pins it
by properties) and ``tests/test_gpu_moment_hits.py`` (which holds the kernel to it bit for bit)."""
import numpy as np

NAN_BITS = np.uint32(0x7FC00000)          # the padding value of a row that holds a NaN
NEG_INF_BITS = np.uint32(0xFF800000)


def overlap(start, length, p):
    """(inter, union) in frames, int64 [M], of window p with every window"""
    s, l = np.asarray(start, np.int64), np.asarray(length, np.int64)
    e = s + l
    inter = np.maximum(0, np.minimum(e, e[p]) - np.maximum(s, s[p]))
    return inter, l + l[p] - inter


def suppresses(inter, union, iou):
    """the kernel's test, one fp32 multiply: float(inter) > float(union) * iou"""
    return inter.astype(np.float32) > union.astype(np.float32) * np.float32(iou)


def moment_select_row(x, start, length, T, iou):
    """one row: x fp32 [M] -> (value bits uint32 [T], pos int32 [T])"""
    x = np.ascontiguousarray(x, np.float32)
    bits = x.view(np.uint32)
    alive = ~np.isnan(x) & ~np.isneginf(x)
    val = np.full(T, NAN_BITS if np.isnan(x).any() else NEG_INF_BITS, np.uint32)
    pos = np.full(T, -1, np.int32)
    for t in range(T):
        if not alive.any():
            break
        cand = np.flatnonzero(alive)
        p = int(cand[np.argmax(x[cand])])               # the first maximum: the smaller position among equal values (-0.0 == +0.0 as floats)
        val[t], pos[t] = bits[p], p
        inter, union = overlap(start, length, p)
        alive &= ~suppresses(inter, union, iou)
        alive[p] = False
    return val, pos


def moment_select_ref(scores, start, length, T, iou, M=None):
    """scores fp32 [P, ld] (first M columns) -> (val fp32 [P, T] with the bits the kernel must return, pos int32 [P, T])"""
    scores = np.asarray(scores, np.float32)
    P = scores.shape[0]
    M = scores.shape[1] if M is None else int(M)
    val, pos = np.empty((P, T), np.uint32), np.empty((P, T), np.int32)
    for r in range(P):
        val[r], pos[r] = moment_select_row(scores[r, :M], start, length, T, iou)
    return val.view(np.float32), pos
