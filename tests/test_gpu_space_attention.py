"""Space and time attention (`dvlp_attention_fwd_ex` / `dvlp_attention_bwd_ex`, mode 0) on a real MI355X, row by row against the float64
restatement `tests/space_attention_ref.py`: every tile branch of the dispatch by region count and both sides of every 16-row tile edge, the
frame-count edges of the folded forward, the shapes time attention runs at (frames and regions swapped), masks that close whole segments
and whole samples, head counts that leave a partial workgroup, and guards around every output and every workspace at its documented size.

Routes (csrc/attention.hip; the kernel names per (dtype, R, route) are `space_attention_ref.fwd_branch` / `bwd_branch`, pinned on the CPU):
    fold          the product route: forward with workspaces, its output and CLS statistics handed to the backward (sattn_fwd / sattn_bwd)
    plain         no statistics, as TimeSpaceBlockFn calls it: mattn_fwd<nqt,nkt> + the VALU CLS workgroup, then cls_pre + the one-pass
                  backward + cls_post (generic wave-per-query kernels from R = 48 on, and always in fp32)
    three-launch  dvlp_dev_attention_bwd_variant(0): mattn_bwd_space<nqt,nkt,0/1> + attn_bwd_cls
    round4        dvlp_dev_attention_lean(0) with statistics: mattn_fwd<n,n> + combine, the one-pass backward on the forward's statistics

Error measure: per TOKEN ROW, max|got - ref| over the row / max(1, max|ref| over the row), maximum over rows -- a wrong row of a padded
tile cannot hide behind a matrix-wide maximum.  Bars are the project's own (`test_gpu_kernels.py`): fp32 1e-4, bf16 3e-2, forward 1x, each of
dq / dk / dv 2x; the CLS statistics (max, log sum) 2e-2.  The reference gets exactly the values the kernel gets (bf16 inputs cast to
double).  The kernel name printed with every figure comes from `fwd_branch` / `bwd_branch`, a restatement of the host dispatch: it is
not read back from the launch (only the raw-ABI cases check `dvlp_attn_ext::folded`), so a change to the dispatch needs the helper and its
CPU table changed with it, or the table below mislabels its rows.  `-s` prints the maximum of every case and, at the end, per (dtype, kernel, quantity): the figures of DESIGN.md section 4 (mode 0).
"""
import contextlib
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import space_attention_ref as sar  # noqa: E402
from demovlp_amd import ops  # noqa: E402
from oracle import restatement as orc  # noqa: E402

DEV = "cuda"
F32_TOL = 1e-4
BF16_TOL = 3e-2
STATS_TOL = 2e-2
F32, BF = torch.float32, torch.bfloat16
R_GRID = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 96, 97, 127]
GUARD = 16                                       # one 16-row tile: the most a padded tile could spill
GUARD_FLOATS = 64
SENTINEL = 24576.0                               # finite, exact in bf16

dtype_id = lambda d: "f32" if d == F32 else "bf16"


def tol(dtype):
    return F32_TOL if dtype == F32 else BF16_TOL


def cases(shapes, routes=("plain", "fold"), dtypes=(F32, BF)):
    """[(dtype, route, *shape)] for every route of `routes` that the dtype and the shape's R (its last entry) admit"""
    return [pytest.param(d, r, *s, id=f"{dtype_id(d)}-{r}-" + "x".join(map(str, s)))
            for s in shapes for d in dtypes for r in routes if sar.admits(d, s[-1], r)]


def dev_cases(shapes):
    return cases(shapes, ("three-launch", "round4"), (BF,))


@contextlib.contextmanager
def developer_route(route):
    """the two routes behind developer switches; every switch back at its default afterwards"""
    try:
        if route == "three-launch":
            ops.call("dvlp_dev_attention_bwd_variant", 0)
        elif route == "round4":
            ops.call("dvlp_dev_attention_lean", 0)
        else:
            raise AssertionError(route)
        yield
    finally:
        ops.call("dvlp_dev_attention_bwd_variant", 1)
        ops.call("dvlp_dev_attention_lean", 1)


# ------------------------------------------------------------------------------------------------------------------
# inputs, masks and the float64 reference: computed once per case and shared (nothing below writes to them)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(dtype, B, F, R, H=12, mask="ragged"):
    """qkv [B*N, 3*H*64] packed, dout [B*N, H*64], additive key mask [B, N] (0 / -100 as object_prologue writes it, CLS key 0): sample 0 has a
    random 20 % of its regions masked; sample 1 its middle segment fully masked and only the first region of its last segment open
    (`ragged`), or every region masked (`cls-only`)."""
    N, D = 1 + F * R, H * 64
    g = torch.Generator().manual_seed(7000 + 1009 * F + 13 * R + 101 * H + B)
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 1.5).to(dtype).to(DEV)
    dout = torch.randn(B * N, D, generator=g).to(dtype).to(DEV)
    open_ = torch.rand(B, F, R, generator=g) > 0.2
    if B >= 2:
        open_[1, F // 2] = False
        open_[1, F - 1] = False
        open_[1, F - 1, 0] = True
        if mask == "cls-only":
            open_[1] = False
    addmask = torch.cat([torch.zeros(B, 1), (open_.reshape(B, -1).float() - 1) * 100], 1).to(DEV)
    return {"qkv": qkv, "dout": dout, "addmask": addmask}


@functools.lru_cache(maxsize=None)
def reference(dtype, B, F, R, H=12, mask="ragged"):
    """(out [B*N, D], dqkv [B*N, 3D], CLS max [B, H], CLS log sum [B, H]) float64 on the CPU, from the values the kernel gets."""
    x = inputs(dtype, B, F, R, H, mask)
    N, D = 1 + F * R, H * 64
    qkv = x["qkv"].cpu().double().reshape(B, N, 3 * D)
    q, k, v = (qkv[..., i * D:(i + 1) * D].clone().requires_grad_(True) for i in range(3))
    out, (mx, sm) = sar.space_attention_ref(q, k, v, x["addmask"].cpu().double(), F, R, H)
    out.backward(x["dout"].cpu().double().reshape(B, N, D))
    return out.detach().reshape(B * N, D), torch.cat([q.grad, k.grad, v.grad], -1).reshape(B * N, 3 * D), mx, torch.log(sm)


def run(x, B, F, R, route):
    """(out, stats or None, dqkv) through the allocating wrappers (H = 12, packed projection)"""
    if route in ("fold", "round4"):
        out, stats = ops.space_attention_fwd(x["qkv"], x["addmask"], B, F, R, want_stats=True)
        assert stats is not None, f"the forward did not fold at R={R}"
        return out, stats, ops.space_attention_bwd(x["qkv"], x["addmask"], x["dout"], B, F, R, out=out, stats=stats)
    return ops.space_attention_fwd(x["qkv"], x["addmask"], B, F, R), None, ops.space_attention_bwd(x["qkv"], x["addmask"], x["dout"], B, F, R)


def raw(dtype, B, F, R, H, route, qkv3, ld, addmask, dout, out, grads3, ldd, fws=None, stats=None, bws=None, after_fwd=None):
    """The C ABI itself: any head count and strides, caller-owned workspaces (by default exactly the sizes include/demovlp_hip.h documents).
    ``after_fwd``: called between the forward and the backward.  Returns the statistics (None off the fold)."""
    N, D = 1 + F * R, H * 64
    fold = route in ("fold", "round4")
    if fold and fws is None:
        fws = torch.empty(B * H * F * 66, device=DEV)
        stats = torch.full((B * H * 4,), float("nan"), device=DEV)
    if bws is None:
        bws = torch.empty(B * H * (F * 192 + 4), device=DEV)
    ext = ops.AttnExt()
    ops.call("dvlp_attention_fwd_ex", ops.dt(dtype), 0, B, N, H, F, R, ops.p(qkv3[0]), ops.p(qkv3[1]), ops.p(qkv3[2]), ld, ops.p(addmask), ops.p(out), D,
             ops.SCALE, ops.p(fws) if fold else None, ops.p(stats) if fold else None, ctypes.byref(ext), ops.stream())
    assert ext.folded == int(fold), f"dvlp_attn_ext::folded = {ext.folded} on the {route} route at R={R}"
    if after_fwd is not None:
        after_fwd()
    ext = ops.AttnExt()
    ops.call("dvlp_attention_bwd_ex", ops.dt(dtype), 0, B, N, H, F, R, ops.p(qkv3[0]), ops.p(qkv3[1]), ops.p(qkv3[2]), ld, ops.p(addmask), ops.p(dout), D,
             ops.p(grads3[0]), ops.p(grads3[1]), ops.p(grads3[2]), ldd, ops.p(bws), ops.SCALE, ops.p(out) if fold else None, D,
             ops.p(stats) if fold else None, ctypes.byref(ext), ops.stream())
    return stats.reshape(B, H, 4) if fold else None


def blocks(t, D):
    return t[:, :D], t[:, D:2 * D], t[:, 2 * D:]


def raw_packed(dtype, B, F, R, H, route, x):
    """(out, stats, dqkv) of the raw call on the packed projection; outputs pre-filled with NaN (an element left unwritten stays one)"""
    N, D = 1 + F * R, H * 64
    out = torch.full((B * N, D), float("nan"), device=DEV, dtype=dtype)
    dqkv = torch.full((B * N, 3 * D), float("nan"), device=DEV, dtype=dtype)
    stats = raw(dtype, B, F, R, H, route, blocks(x["qkv"], D), 3 * D, x["addmask"], x["dout"], out, blocks(dqkv, D), 3 * D)
    return out, stats, dqkv


def row_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    e = (got - ref).abs().amax(dim=1) / ref.abs().amax(dim=1).clamp_min(1.0)
    return float(e.max()) if bool(torch.isfinite(got).all()) else float("nan")


MAXIMA = {}      # (dtype, kernel, quantity) -> largest per-row error seen
FUSED = {}       # (R, F, deferred reductions on) -> did the backward queue the column sums itself


@pytest.fixture(scope="module", autouse=True)
def _print_maxima():
    yield
    if MAXIMA:
        print("\nspace / time attention, per-row error maxima by (dtype, kernel, quantity):")
        for (dt_, br, what), e in sorted(MAXIMA.items()):
            print(f"  {dt_:4s} {br:42s} {what:4s} {e:.3e}")
    if FUSED:
        print("fused qkv-bias column sums (R, F, deferred reductions):")
        for key, fused in sorted(FUSED.items()):
            print(f"  R={key[0]:3d} F={key[1]:2d} deferred={key[2]!s:5s} fused={fused}")


def check(dtype, B, F, R, route, got, H=12, mask="ragged", what="space-attn"):
    """every token row of out, dq, dk, dv (rows of masked query positions included: the block's LayerNorm reads them), and the statistics"""
    out, stats, dqkv = got
    D = H * 64
    ref_out, ref_d, ref_max, ref_lse = reference(dtype, B, F, R, H, mask)
    fb, bb = sar.fwd_branch(dtype, R, route), sar.bwd_branch(dtype, R, route)
    rows = [("out", out, ref_out, tol(dtype), fb)]
    rows += [(n, dqkv[:, i * D:(i + 1) * D], ref_d[:, i * D:(i + 1) * D], 2 * tol(dtype), bb) for i, n in enumerate(("dq", "dk", "dv"))]
    if stats is not None:
        st = stats.reshape(B * H, 4)
        assert bool((st[:, 1] > 0).all()) and bool((st[:, 2:] == 0).all()), "statistics: the sum is not positive, or the spare slots are not 0"
        rows += [("max", st[:, :1], ref_max.reshape(-1, 1), STATS_TOL, fb), ("lse", torch.log(st[:, 1:2]), ref_lse.reshape(-1, 1), STATS_TOL, fb)]
    bad = []
    for name, g, r, bar, br in rows:
        e = row_err(g, r)
        print(f"{what} {dtype_id(dtype)} B={B} F={F} R={R} H={H} {mask} {route} {name:3s} [{br}] per-row err {e:.3e} (bar {bar:.0e})")
        key = (dtype_id(dtype), br, name)
        MAXIMA[key] = e if e != e else max(MAXIMA.get(key, 0.0), e)          # (a NaN stays)
        if not e < bar:
            bad.append(f"{name} {e:.3e} >= {bar:.0e} [{br}]")
    assert not bad, f"{dtype_id(dtype)} B={B} F={F} R={R} H={H} {mask} {route}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# a. region counts: every tile instance and both sides of every tile edge
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,route,F,R", cases([(3, R) for R in R_GRID]))
def test_region_counts_vs_float64(dtype, route, F, R):
    x = inputs(dtype, 2, F, R)
    if route == "plain":      # asking for statistics: they come back exactly where the CLS row finds a free query row in the last tile
        no_fold = dtype == F32 or R % 16 == 0 or R > 47
        assert (ops.space_attention_fwd(x["qkv"], x["addmask"], 2, F, R, want_stats=True)[1] is None) == no_fold, f"fold at R={R}"
    check(dtype, 2, F, R, route, run(x, 2, F, R, route))


@pytest.mark.parametrize("dtype,route,F,R", dev_cases([(3, R) for R in R_GRID if R <= 48]))
def test_region_counts_vs_float64_developer_routes(dtype, route, F, R):
    """three-launch at every R up to 48 (48 lands on the generic kernels), round4 wherever the forward folds"""
    with developer_route(route):
        check(dtype, 2, F, R, route, run(inputs(dtype, 2, F, R), 2, F, R, route))


# ------------------------------------------------------------------------------------------------------------------
# b. frame counts of the folded forward: CLS partials merged in LDS (F <= 8) or by the combine launch, a partly filled last chunk
# ------------------------------------------------------------------------------------------------------------------
FRAME_SHAPES = [(F, 17) for F in (1, 7, 8, 9, 12, 17)] + [(9, 15), (9, 36)]


@pytest.mark.parametrize("dtype,route,F,R", cases(FRAME_SHAPES, ("fold",), (BF,)))
def test_frame_counts_vs_float64(dtype, route, F, R):
    check(dtype, 2, F, R, route, run(inputs(dtype, 2, F, R), 2, F, R, route))


@pytest.mark.parametrize("dtype,route,F,R", cases(FRAME_SHAPES, ("round4",), (BF,)))
def test_frame_counts_vs_float64_round4(dtype, route, F, R):
    with developer_route(route):
        check(dtype, 2, F, R, route, run(inputs(dtype, 2, F, R), 2, F, R, route))


# ------------------------------------------------------------------------------------------------------------------
# c. time attention: (segments, length) = (regions, frames)
# ------------------------------------------------------------------------------------------------------------------
TIME_SHAPES = [(2, 36, 1), (2, 30, 4), (2, 36, 8), (2, 36, 16), (2, 30, 32), (1, 36, 32)]


@pytest.mark.parametrize("dtype,route,B,S,L", cases(TIME_SHAPES, ("plain",)))
def test_time_attention_shapes_vs_float64(dtype, route, B, S, L):
    """what TimeSpaceBlockFn launches: one segment per region slot, as long as the clip has frames (16 -> <1,2>, 32 -> <2,3>)"""
    check(dtype, B, S, L, route, run(inputs(dtype, B, S, L), B, S, L, route), what="time-attn")


@pytest.mark.parametrize("dtype", [F32, BF], ids=dtype_id)
def test_time_attention_through_the_token_transposes(dtype):
    """16 frames x 30 regions end to end, frame-major in and out: token_transpose, mode 0 with (F, R) swapped, transpose back -- and the same
    chain for the gradient -- against the oracle's time attention (its N x N structural mask) in float64."""
    B, F, R = 2, 16, 30
    N = 1 + F * R
    x = inputs(dtype, B, F, R)
    addmask_t = sar.to_segment_major(x["addmask"].cpu(), F, R).contiguous().to(DEV)
    qkv_t = ops.token_transpose(x["qkv"].reshape(B, N, 2304), B, F, R).reshape(B * N, 2304)
    out_t = ops.space_attention_fwd(qkv_t, addmask_t, B, R, F)
    out = ops.token_transpose(out_t.reshape(B, N, 768), B, R, F).reshape(B * N, 768)
    dout_t = ops.token_transpose(x["dout"].reshape(B, N, 768), B, F, R).reshape(B * N, 768)
    dqkv_t = ops.space_attention_bwd(qkv_t, addmask_t, dout_t, B, R, F)
    dqkv = ops.token_transpose(dqkv_t.reshape(B, N, 2304), B, R, F).reshape(B * N, 2304)
    assert torch.equal(qkv_t.cpu().reshape(B, N, 2304), sar.to_segment_major(x["qkv"].cpu().reshape(B, N, 2304), F, R)), "token_transpose"
    q = x["qkv"].cpu().double().reshape(B, N, 2304).requires_grad_(True)
    ref = orc.space_attention(q, x["addmask"].cpu().double(), F, R, time=True)
    ref.backward(x["dout"].cpu().double().reshape(B, N, 768))
    fb, bb = sar.fwd_branch(dtype, F, "plain"), sar.bwd_branch(dtype, F, "plain")
    bad = []
    for name, g, r, mult, br in (("out", out, ref.detach().reshape(B * N, 768), 1, fb), ("dq", dqkv[:, :768], q.grad.reshape(B * N, 2304)[:, :768], 2, bb),
                                 ("dk", dqkv[:, 768:1536], q.grad.reshape(B * N, 2304)[:, 768:1536], 2, bb),
                                 ("dv", dqkv[:, 1536:], q.grad.reshape(B * N, 2304)[:, 1536:], 2, bb)):
        e = row_err(g, r)
        print(f"time-attn end to end {dtype_id(dtype)} {name:3s} [{br}] per-row err {e:.3e} (bar {tol(dtype) * mult:.0e})")
        key = (dtype_id(dtype), br, name)
        MAXIMA[key] = e if e != e else max(MAXIMA.get(key, 0.0), e)
        if not e < tol(dtype) * mult:
            bad.append(f"{name} {e:.3e} >= {tol(dtype) * mult:.0e} [{br}]")
    assert not bad, f"{dtype_id(dtype)}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------
# d. a sample with every region masked: only the CLS key is open
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,route,F,R", cases([(3, 15), (3, 31), (3, 47)]))
def test_sample_with_every_region_masked(dtype, route, F, R):
    x = inputs(dtype, 2, F, R, mask="cls-only")
    assert bool((x["addmask"][1, 1:] == -100).all()) and float(x["addmask"][1, 0]) == 0 and bool((x["addmask"][0, 1:] == 0).any())
    check(dtype, 2, F, R, route, run(x, 2, F, R, route), mask="cls-only")


@pytest.mark.parametrize("dtype,route,F,R", dev_cases([(3, 15), (3, 31), (3, 47)]))
def test_sample_with_every_region_masked_developer_routes(dtype, route, F, R):
    with developer_route(route):
        check(dtype, 2, F, R, route, run(inputs(dtype, 2, F, R, mask="cls-only"), 2, F, R, route), mask="cls-only")


# ------------------------------------------------------------------------------------------------------------------
# e. items = B*H*F that do not fill the last workgroup of four waves (the raw C ABI: the wrappers serve H = 12 only)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fold", "plain"])
@pytest.mark.parametrize("B,H,F,R", [(1, 3, 3, 17), (1, 1, 5, 36)], ids=["H3-items9", "H1-items5"])
def test_head_counts_that_leave_a_partial_workgroup(B, H, F, R, route):
    assert (B * H * F) % 4 != 0
    x = inputs(BF, B, F, R, H)
    check(BF, B, F, R, route, raw_packed(BF, B, F, R, H, route, x), H=H)


# ------------------------------------------------------------------------------------------------------------------
# f. bit-exact: no tolerance
# ------------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(F, R) for F in (3, 9) for R in (15, 16, 31, 32, 47, 48)]          # every tile class of every route, and the generic kernels
NAMES = ("out", "stats", "dqkv")


def keep_one_per_class(params):
    """fp32 has one pair of kernels for every R: keep R = 15 and 48 only.  bf16 keeps every R on every route -- plain: 15 / 16 / 31 / 32 / 47
    are the five MFMA forwards and the three classes of the one-pass backward behind its own statistics launch, 48 the generic kernels"""
    return [prm for prm in params if prm.values[0] != F32 or prm.values[3] in (15, 48)]


def same_twice(dtype, route, F, R):
    x = inputs(dtype, 2, F, R)
    a, b = raw_packed(dtype, 2, F, R, 12, route, x), raw_packed(dtype, 2, F, R, 12, route, x)
    for name, s, t in zip(NAMES, a, b):
        assert (s is None and t is None) or torch.equal(s, t), f"{name}: two calls on the same inputs differ ({dtype_id(dtype)} {route} F={F} R={R})"


def separate_equals_packed(dtype, route, F, R):
    """ld = ldo = ldd = 768 with three q / k / v tensors and three gradient tensors against the packed 2304-stride call: the stride enters
    addresses only"""
    B, N = 2, 1 + F * R
    x = inputs(dtype, B, F, R)
    pk = raw_packed(dtype, B, F, R, 12, route, x)
    qkv3 = tuple(t.contiguous() for t in blocks(x["qkv"], 768))
    out = torch.full((B * N, 768), float("nan"), device=DEV, dtype=dtype)
    grads3 = tuple(torch.full((B * N, 768), float("nan"), device=DEV, dtype=dtype) for _ in range(3))
    stats = raw(dtype, B, F, R, 12, route, qkv3, 768, x["addmask"], x["dout"], out, grads3, 768)
    for name, s, t in zip(NAMES, pk, (out, stats, torch.cat(grads3, 1))):
        assert (s is None and t is None) or torch.equal(s, t), f"{name}: separate tensors change the result ({dtype_id(dtype)} {route} F={F} R={R})"


@pytest.mark.parametrize("dtype,route,F,R", keep_one_per_class(cases(EXACT_SHAPES)))
def test_space_attention_run_to_run_identical(dtype, route, F, R):
    same_twice(dtype, route, F, R)


@pytest.mark.parametrize("dtype,route,F,R", dev_cases(EXACT_SHAPES))
def test_space_attention_run_to_run_identical_developer_routes(dtype, route, F, R):
    with developer_route(route):
        same_twice(dtype, route, F, R)


@pytest.mark.parametrize("dtype,route,F,R", keep_one_per_class(cases(EXACT_SHAPES)))
def test_separate_tensors_equal_the_packed_projection(dtype, route, F, R):
    separate_equals_packed(dtype, route, F, R)


@pytest.mark.parametrize("dtype,route,F,R", dev_cases(EXACT_SHAPES))
def test_separate_tensors_equal_the_packed_projection_developer_routes(dtype, route, F, R):
    with developer_route(route):
        separate_equals_packed(dtype, route, F, R)


# ------------------------------------------------------------------------------------------------------------------
# g. guards around every output and every workspace
# ------------------------------------------------------------------------------------------------------------------
GUARD_SHAPES = [(3, R) for R in (1, 16, 17, 33, 47, 48, 127)] + [(9, 17)]


def guarded_rows(rows, cols, dtype):
    buf = torch.full((rows + 2 * GUARD, cols), SENTINEL, device=DEV, dtype=dtype)
    buf[GUARD:GUARD + rows] = float("nan")
    return buf, buf[GUARD:GUARD + rows]


def guarded_floats(n):
    buf = torch.full((n + GUARD_FLOATS,), SENTINEL, device=DEV)
    buf[:n] = float("nan")
    return buf, buf[:n]


def stays_inside(dtype, route, F, R):
    """out [B*N, 768] and dqkv [B*N, 2304] are views with 16 sentinel rows before and after; the forward workspace, the statistics and the
    backward workspace have exactly the documented size (B*H*F*66, B*H*4 and B*H*(F*192 + 4) floats) and 64 sentinel floats behind them.
    Every guard survives each of the two calls (checked after the forward and again after the backward), every output element is written, and what lands inside is what the allocating wrappers return."""
    B, H, N = 2, 12, 1 + F * R
    x = inputs(dtype, B, F, R)
    where = f"({dtype_id(dtype)} {route} F={F} R={R})"
    obuf, out = guarded_rows(B * N, 768, dtype)
    gbuf, dqkv = guarded_rows(B * N, 2304, dtype)
    fbuf, fws = guarded_floats(B * H * F * 66)
    sbuf, st = guarded_floats(B * H * 4)
    bbuf, bws = guarded_floats(B * H * (F * 192 + 4))

    def guards_intact(call):
        torch.cuda.synchronize()
        for name, buf in (("out", obuf), ("dq | dk | dv", gbuf)):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f"the {call} wrote outside the rows of {name} {where}"
        for name, buf in (("forward workspace", fbuf), ("statistics", sbuf), ("backward workspace", bbuf)):
            assert bool((buf[-GUARD_FLOATS:] == SENTINEL).all()), f"the {call} wrote past the documented size of the {name} {where}"

    def after_forward():
        guards_intact("forward")
        assert bool(torch.isnan(dqkv).all()) and bool(torch.isnan(bws).all()), f"the forward wrote into the backward's buffers {where}"

    stats = raw(dtype, B, F, R, H, route, blocks(x["qkv"], 768), 2304, x["addmask"], x["dout"], out, blocks(dqkv, 768), 2304, fws=fws, stats=st, bws=bws,
                after_fwd=after_forward)
    guards_intact("backward")
    if stats is None:
        assert bool(torch.isnan(fws).all()) and bool(torch.isnan(st).all()), f"no fold, yet the forward workspace or the statistics were written {where}"
    want = run(x, B, F, R, route)
    for name, a, b in zip(NAMES, (out, stats, dqkv), want):
        if a is None and b is None:
            continue
        assert not bool(torch.isnan(a).any()), f"{name}: elements left unwritten {where}"
        assert torch.equal(a, b), f"{name}: the guarded call differs from the allocating wrappers {where}"


@pytest.mark.parametrize("dtype,route,F,R", cases(GUARD_SHAPES))
def test_outputs_and_workspaces_stay_inside_their_bounds(dtype, route, F, R):
    stays_inside(dtype, route, F, R)


@pytest.mark.parametrize("dtype,route,F,R", dev_cases([s for s in GUARD_SHAPES if s[1] <= 48]))
def test_outputs_and_workspaces_stay_inside_their_bounds_developer_routes(dtype, route, F, R):
    with developer_route(route):
        stays_inside(dtype, route, F, R)


# ------------------------------------------------------------------------------------------------------------------
# h. the qkv-bias gradient: column sums of dq | dk | dv queued from inside the backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "immediate"])
@pytest.mark.parametrize("F", [3, 9])
@pytest.mark.parametrize("R", [15, 31, 36, 47])
def test_fused_bias_gradient_column_sums(R, F, deferred):
    """Fold route with `colsum_to`.  Fused (the deferred-reduction queue is on): every column of the fp32 [2304] result is the sum of the STORED
    bf16 dqkv column to the worst-case bound of an fp32 summation in any order, rows * 2^-24 * sum|x| -- no measured constant.  Not fused
    (no queue to put it on): the destination is untouched and the caller sums the columns itself."""
    B = 2
    x = inputs(BF, B, F, R)
    dst = torch.full((2304,), SENTINEL, device=DEV)
    assert not ops._DEFER, "an earlier test left the deferred-reduction queue enabled"
    if deferred:
        ops.enable_deferred_reductions(torch.device(DEV), workspace_mb=64)
    try:
        out, stats = ops.space_attention_fwd(x["qkv"], x["addmask"], B, F, R, want_stats=True)
        assert stats is not None
        dqkv, fused = ops.space_attention_bwd(x["qkv"], x["addmask"], x["dout"], B, F, R, out=out, stats=stats, colsum_to=dst)
        if fused:
            ops.flush_reductions()
        torch.cuda.synchronize()
    finally:
        if deferred:
            ops.disable_deferred_reductions()
    FUSED[(R, F, deferred)] = fused
    assert fused == deferred, "the one-pass backward with forward statistics queues its column sums exactly when there is a queue"
    assert torch.equal(dqkv, run(x, B, F, R, "fold")[2]), "queueing the column sums changed dqkv"
    if not fused:
        assert bool((dst == SENTINEL).all()), "not fused, yet the destination was written"
        return
    xd = dqkv.double().cpu()
    err, bound = (dst.double().cpu() - xd.sum(0)).abs(), xd.shape[0] * 2.0 ** -24 * xd.abs().sum(0)
    worst = int((err - bound).argmax())
    print(f"colsum R={R} F={F}: largest err / bound {float((err / bound).max()):.3e} (column {worst}: err {float(err[worst]):.3e}, bound {float(bound[worst]):.3e})")
    assert bool((err <= bound).all()), f"column {worst}: |sum - ref| = {float(err[worst]):.3e} > {float(bound[worst]):.3e}"
