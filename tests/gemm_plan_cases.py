"""Cases of tests/golden/gemm_plan_cases.json and the call that asks a developer library what dvlp_gemm would launch for one of them
(`dvlp_dev_gemm_plan`, include/demovlp_hip_dev.h).  Pure host arithmetic on both sides: no GPU, no operand is dereferenced.

    python tests/gemm_plan_cases.py LIBRARY OUT.json

writes the case list with the answers of LIBRARY as expectations.  The committed table was NOT made from the library it now tests:
see tests/README.md ("gemm_plan_cases.json").
"""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["err", "family", "safe", "mih8", "S", "kchunk", "ek8", "p8p", "csum_fuse", "csum_rows", "vec", "a_vec", "b_vec", "grid_x", "grid_y", "grid_z",
          "block", "lds", "ntm", "ntn", "reduce_grid", "p8p_noqueue", "grid_x_noqueue"]
FAMILIES = {"f32": 0, "rb": 1, "reg": 2, "g128": 3, "wide": 4, "p8": 5}
KNOB_DEFAULTS = {"dvlp_dev_gemm_variant": 1, "dvlp_dev_gemm_ablate": 0, "dvlp_dev_gemm_wide_mode": 0, "dvlp_dev_gemm_p8_mode": 1,
                 "dvlp_dev_gemm_p8_short_tiles": 1, "dvlp_dev_gemm_p8_persistent": 1, "dvlp_dev_gemm_resident_b": 1, "dvlp_dev_gemm_force_split": 0,
                 "dvlp_dev_gemm_splitk_target": 768, "dvlp_dev_gemm_corun_split": 0}
GELU, GELU_BWD, RELU_BWD, ACCUM, LEAKY, OUT_F32 = 1, 2, 4, 8, 16, 32
WS = 256 << 20                 # split-K workspace of the "registered" variants
STREAM = 0x5000                # a map key in the library, never dereferenced
BASE = 0x10000000              # operand "addresses": only their 16-byte alignment is looked at


def case(form, M, N, K, batch=1, flags=0, dtype=1, **kw):
    """form: two letters, A then B, K = reduction dimension contiguous, R = rows contiguous (the `KK/KR/RK/RR` column of DVLP_PROF_REPORT)."""
    tA, tB = int(form[0] == "R"), int(form[1] == "R")
    c = dict(name=kw.pop("name", ""), form=form, dtype=dtype, M=M, N=N, K=K, batch=batch, flags=flags, alpha=1.0, lda=M if tA else K, ldb=N if tB else K, ldc=N,
             ldres=0, ldaux=0, A=0, B=0, C=0, bias=None, res=None, aux=None, colsum=0, ws=0, corun=0, knobs={})
    if flags & (GELU | GELU_BWD | RELU_BWD):
        c.update(aux=0, ldaux=N)
    c.update(kw)
    if c["res"] is not None and not c["ldres"]:
        c["ldres"] = N
    return c


def profile_rows():
    """(form, M, N, K, batch, flags, kern) of every dvlp_gemm row of profiles/r6_final_gemm_shapes.txt (its `p8g` rows are grouped weight-gradient launches,
    which dvlp_gemm's planner never sees)."""
    rows = []
    for ln in open(os.path.join(ROOT, "profiles", "r6_final_gemm_shapes.txt")):
        m = re.match(r"\[gemm\] (\w\w) M=\s*(\d+) N=\s*(\d+) K=\s*(\d+) b=\s*(\d+) epi=\s*(\d+) kern=(\w+)", ln)
        if m and m.group(7) != "p8g":
            rows.append((m.group(1),) + tuple(int(x) for x in m.group(2, 3, 4, 5, 6)) + (m.group(7),))
    return rows


LAYER = [("KK", 768, 768, 0), ("KK", 2304, 768, 0), ("KK", 3072, 768, GELU), ("KK", 768, 3072, 0),
         ("KR", 768, 768, 0), ("KR", 768, 2304, 0), ("KR", 768, 3072, 0), ("KR", 3072, 768, GELU_BWD)]


def cases():
    out = []

    def variants(c):       # with / without a registered workspace, stream plain / marked co-running
        for ws in (0, WS):
            for corun in (0, 1):
                out.append(dict(c, ws=ws, corun=corun, name=f"{c['name']} ws={int(ws > 0)} corun={corun}"))

    for form, M, N, K, b, flags, kern in profile_rows():
        variants(case(form, M, N, K, b, flags, bias=0 if form == "KK" and b == 1 else None, kern=kern, name=f"profile {form} {M}x{N}x{K} b{b} epi{flags}"))
    for M, tag in ((7712, "config 4"), (16 * (32 * 36 + 1), "config 5")):
        for form, N, K, flags in LAYER:
            variants(case(form, M, N, K, 1, flags, bias=0 if form == "KK" else None, name=f"{tag} {form} {M}x{N}x{K} epi{flags}"))
    one = lambda c: out.append(c)
    # ragged operands: the bounds-checked register-staged kernel
    one(case("RR", 100, 256, 512, name="safe: M % 8 != 0 with transA", lda=104))
    one(case("KK", 256, 256, 100, name="safe: K % 8 != 0", lda=104, ldb=104))
    one(case("KK", 256, 256, 4, name="safe: K < 8", lda=8, ldb=8))
    one(case("KR", 512, 100, 256, name="safe: N % 8 != 0 with transB", ldb=104, ldc=104))
    # refused without a launch
    one(case("KK", 256, 256, 100, name="error: lda % 8"))
    one(case("KK", 256, 256, 256, name="error: misaligned A", A=8))
    one(case("KK", 256, 256, 256, name="error: dtype", dtype=7))
    one(case("KK", 0, 256, 256, name="error: M = 0"))
    one(case("KK", 256, 256, 256, flags=GELU, name="error: GELU without aux", aux=None))
    # fp32
    for form in ("KK", "KR", "RK", "RR"):
        one(case(form, 300, 200, 96, dtype=0, name=f"fp32 {form}"))
    one(case("KK", 300, 200, 98, dtype=0, name="fp32 unaligned lda / ldb, batched", batch=3))
    one(case("KK", 300, 200, 96, dtype=0, name="fp32 misaligned B, unaligned ldc", B=4, ldc=202))
    # column sums of the output: fusable (256-column kernel, one batch, whole tiles) and not
    one(case("KR", 18496, 768, 768, name="colsum fused", colsum=1))
    one(case("KR", 18496, 768, 768, name="colsum fused, workspace", colsum=1, ws=WS))
    one(case("KK", 18432, 6656, 256, flags=LEAKY, name="colsum fused where the persistent form would run", colsum=1, bias=0))
    one(case("KR", 512, 256, 768, name="colsum not fusable: 128-row kernel", colsum=1, ws=WS))
    one(case("KR", 6400, 768, 3072, name="colsum not fusable: split K", colsum=1, ws=WS))
    one(case("KR", 18496, 768, 768, name="colsum not fusable: unaligned ldc", colsum=1, ldc=772))
    # epilogues: residual, unaligned outputs / bias
    one(case("KK", 18496, 768, 768, name="residual epilogue", bias=0, res=0))
    one(case("KK", 6400, 768, 3072, name="residual epilogue, workspace", bias=0, res=0, ws=WS))
    one(case("KK", 18496, 768, 768, name="unaligned ldc", bias=0, ldc=772))
    one(case("KK", 18496, 768, 768, name="misaligned bias", bias=4))
    one(case("KK", 18496, 768, 768, name="misaligned residual", res=8))
    one(case("KK", 18496, 3072, 768, flags=GELU, name="unaligned ldaux", bias=0, ldaux=3076))
    one(case("KK", 18496, 768, 768, name="alpha != 1", alpha=0.5))
    one(case("KK", 18496, 768, 768, flags=ACCUM, name="accumulate"))
    one(case("KK", 18496, 800, 768, name="N % 256 != 0"))
    one(case("KK", 18432, 6656, 256, flags=LEAKY, name="persistent form", bias=0))
    one(case("KK", 18432, 6656, 512, flags=GELU, name="persistent form, GELU", bias=0))
    # every developer switch of dvlp_gemm's planner at one non-default value, on a shape where it changes the plan
    k = lambda name, val, c, **kw: one(dict(c, knobs={name: val}, name=f"{name}({val}): {c['name']}", **kw))
    text, obj, small = case("KK", 6400, 768, 3072, name="6400x768x3072", bias=0), case("KK", 18496, 768, 768, name="18496x768x768", bias=0), case("KK", 6400, 256, 768, name="6400x256x768")
    k("dvlp_dev_gemm_variant", 0, obj)
    k("dvlp_dev_gemm_ablate", 1, obj)
    k("dvlp_dev_gemm_wide_mode", 2, small)
    k("dvlp_dev_gemm_wide_mode", 1, case("KK", 140000, 128, 768, name="140000x128x768"))
    k("dvlp_dev_gemm_p8_mode", 0, obj)
    k("dvlp_dev_gemm_p8_mode", 2, small)
    for v in (0, 2, 3, 11, 12, 13, 14):
        k("dvlp_dev_gemm_p8_short_tiles", v, obj)
        k("dvlp_dev_gemm_p8_short_tiles", v, text, ws=WS)
    k("dvlp_dev_gemm_p8_persistent", 0, case("KK", 18432, 6656, 256, flags=LEAKY, name="18432x6656x256", bias=0))
    k("dvlp_dev_gemm_resident_b", 0, case("KK", 6656, 288, 256, 64, name="6656x288x256 b64"))
    k("dvlp_dev_gemm_force_split", 3, text, ws=WS)
    k("dvlp_dev_gemm_force_split", 3, text)
    k("dvlp_dev_gemm_splitk_target", 256, case("RR", 256, 768, 6400, flags=OUT_F32, name="256x768x6400"), ws=WS)
    k("dvlp_dev_gemm_corun_split", 1, text, ws=WS, corun=1)
    return out


def query(call, c):
    """Ask the active developer library (``call`` = demovlp_amd._lib.call) for the plan of case ``c``: {field: value}.  Leaves no switch, workspace or hint set."""
    ptr = lambda off: None if off is None else BASE + off
    out = (ctypes.c_int64 * len(FIELDS))()
    try:
        for name, val in c["knobs"].items():
            call(name, val)
        if c["ws"]:
            call("dvlp_set_workspace_stream", STREAM, BASE, c["ws"])
        call("dvlp_stream_hint", STREAM, c["corun"])
        tA, tB = int(c["form"][0] == "R"), int(c["form"][1] == "R")
        M, N, K, b = c["M"], c["N"], c["K"], c["batch"]
        stride = lambda n: n if b > 1 else 0
        call("dvlp_dev_gemm_plan", c["dtype"], tA, tB, M, N, K, ptr(c["A"]), c["lda"], ptr(c["B"]), c["ldb"], ptr(c["C"]), c["ldc"], ptr(c["bias"]), ptr(c["res"]),
             c["ldres"], ptr(c["aux"]), c["ldaux"], c["flags"], c["alpha"], b, stride(M * K), stride(N * K), stride(M * c["ldc"]), stride(M * c["ldres"]),
             stride(M * c["ldaux"]), c["colsum"], STREAM, out)
    finally:
        for name in c["knobs"]:
            call(name, KNOB_DEFAULTS[name])
        call("dvlp_set_workspace_stream", STREAM, None, 0)
        call("dvlp_stream_hint", STREAM, 0)
    return dict(zip(FIELDS, (int(v) for v in out)))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from demovlp_amd import _lib
    _lib.use_library(os.path.abspath(sys.argv[1]))
    table = [dict(c, expect=query(_lib.call, c)) for c in cases()]
    with open(sys.argv[2], "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in table) + "\n]\n")
    print(len(table), "cases ->", sys.argv[2])
