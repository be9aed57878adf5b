"""The C-ABI shared library: builds for gfx950 without a GPU, loads, and exports every symbol include/demovlp_hip.h
declares.  No compute calls here (no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from demovlp_amd import _lib
    return _lib


def declared_symbols(header="demovlp_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dvlp_\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol(lib):
    names = declared_symbols()
    assert len(names) >= 25
    handle = ctypes.CDLL(lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/demovlp_hip.h but not exported"
    assert set(lib.exported_symbols()) == set(names)


def test_integration_doc_names_every_entry_point_with_the_reference_interface_it_replaces():
    """INTEGRATION.md section 2 maps every entry point of the product library to the reference code (file:line) it stands in for -- the table a
    maintainer binds against; a new entry point without a row fails here."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [ln for ln in doc.splitlines() if ln.startswith("| `dvlp_")]
    named = set(re.findall(r"`(dvlp_\w+)`", " ".join(r.split("|")[1] for r in rows)))
    assert named == set(declared_symbols()), sorted(set(declared_symbols()) ^ named)
    for r in rows:
        what = r.split("|")[2]
        assert re.search(r"\w+\.py:\d+", what) or "no reference counterpart" in what or "autograd" in what, r[:80]


def test_product_library_exports_no_developer_switch(lib):
    """`dvlp_dev_*` (A/B switches, timing ablations, forced code paths) exist only in the -DDVLP_DEV build: the shipped library has no
    process-global knob to flip (`nm -D libdemovlp_hip.so | grep dvlp_dev_` is empty), the developer build exports all of them on top of the
    product surface, and asking the product library for one fails loudly."""
    import subprocess
    assert not any(n.startswith("dvlp_dev_") for n in declared_symbols())
    dev = declared_symbols("demovlp_hip_dev.h")
    assert len(dev) >= 20 and all(n.startswith("dvlp_dev_") for n in dev)
    syms = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "dvlp_dev_" not in syms and "dvlp_gemm" in syms
    handle = ctypes.CDLL(lib.DEV_LIB_PATH)
    for n in dev + declared_symbols():
        assert hasattr(handle, n), f"{n} missing from the developer build"
    lib.use_dev_library(False)            # (conftest put this test on the developer build because it names the switch)
    assert lib.active_library() == lib.LIB_PATH and not lib.is_dev_library()
    with pytest.raises(lib.DemoVLPHipError):
        lib.call("dvlp_dev_gemm_p8_mode", 2)
    lib.use_dev_library(True)
    try:
        assert lib.is_dev_library()
        lib.call("dvlp_dev_gemm_p8_mode", 1)
        assert lib.call("dvlp_colsum_chunks", 100) == 2
    finally:
        lib.use_dev_library(False)
    assert not lib.is_dev_library()


FORMER_VARIABLES = ["DVLP_ABLATE_LN_FWD", "DVLP_NO_FUSED_QKV", "DVLP_NO_LN_COLSUM", "DVLP_NO_GEMM_COLSUM", "DVLP_NO_ATTN_COLSUM", "DVLP_XATTN_NO_GRAM",
                    "DVLP_XATTN_PARALLEL", "DVLP_P8_MIN_TILES", "DVLP_P8_ROUNDS", "DVLP_CORUN_SPLIT", "DVLP_CORUN_WGRAD_SPLIT"]


def test_product_reads_no_developer_variable(lib):
    """No stray `DVLP_*` variable changes what the shipped library or package computes or launches: the library holds no such name but
    DVLP_PROF_REPORT (which only prints), no module of the package reads one from the environment, and with every former variable set a fresh
    interpreter still has the Python-level switches at their defaults.  They are developer switches now, behind `_lib.call("dvlp_dev_*")`."""
    import subprocess
    import sys
    blob = open(lib.LIB_PATH, "rb").read()
    assert set(re.findall(rb"DVLP_[A-Z0-9_]+", blob)) <= {b"DVLP_PROF_REPORT"}
    pkg = os.path.join(ROOT, "demovlp_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                for ln in open(os.path.join(dirpath, f)):
                    assert not (re.search(r"environ|getenv", ln) and "DVLP_" in ln), (f, ln)
    code = ("from demovlp_amd import ops, functional as Fn; "
            "print(ops.LN_FWD_ABLATE, Fn.FUSE_TEXT_QKV, Fn.FUSE_LN_COLSUM, Fn.FUSE_GEMM_COLSUM, Fn.FUSE_ATTN_COLSUM)")
    env = {**os.environ, **{v: "1" for v in FORMER_VARIABLES}, "DVLP_XATTN_PARALLEL": "0", "PYTHONPATH": ROOT}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["False", "True", "True", "True", "True"]
    lib.use_dev_library(False)
    from demovlp_amd import ops
    with pytest.raises(lib.DemoVLPHipError):
        lib.call("dvlp_dev_ln_fwd_ablate", 1)
    lib.use_dev_library(True)
    try:
        lib.call("dvlp_dev_ln_fwd_ablate", 1)
        assert ops.LN_FWD_ABLATE is True
        lib.call("dvlp_dev_ln_fwd_ablate", 0)
    finally:
        lib.use_dev_library(False)
    assert ops.LN_FWD_ABLATE is False


def test_size_helpers_run_on_host(lib):
    # pure host arithmetic, safe without a GPU
    assert lib.call("dvlp_layernorm_bwd_blocks", 18496) == 1024
    assert lib.call("dvlp_colsum_chunks", 100) == 2
    fwd = lib.call("dvlp_xattn_workspace_bytes", lib.BF16, 64, 64, 288, 99, 0)
    bwd = lib.call("dvlp_xattn_workspace_bytes", lib.BF16, 64, 64, 288, 99, 1)
    fwd32 = lib.call("dvlp_xattn_workspace_bytes", lib.F32, 64, 64, 288, 99, 0)
    # inference in bf16 runs the fused per-pair kernel: O(B (G + W) d) operands only; the multi-kernel path (training, fp32) keeps
    # the [B, B, G, W] intermediates
    assert fwd < 5.0e7 and 1.0e9 < bwd < 3.0e9 and 2.0e9 < fwd32 < 6.0e9


def test_bad_arguments_are_reported_not_launched(lib):
    with pytest.raises(lib.DemoVLPHipError):
        lib.call("dvlp_gemm", 7, 0, 0, 16, 16, 16, None, 16, None, 16, None, 16, None, None, 0, None, 0, 0, 1.0, None)
    with pytest.raises(lib.DemoVLPHipError):
        lib.call("dvlp_layernorm_fwd", lib.F32, 4, 100, None, None, None, 1e-6, None, None, None, None, None)


def test_attention_and_keep_mask_entries_refuse_what_they_do_not_serve(lib):
    """Text attention (mode 1) serves 1 <= N <= 128 keys with R == N; there is no mode 2; a keep mask needs p < 1 and N >= 1.  Each is refused
    on the host with the status that names the reason (null pointers: nothing may be launched), by the `_ex` entries and the plain ones."""
    def fwd(entry, mode, N, R, ext=True):
        tail = (None, None) if ext else (None,)                         # (ext,) stream
        return lib.call(entry, lib.BF16, mode, 2, N, 12, 1, R, None, None, None, 768, None, None, 768, 0.125, None, None, *tail)

    def bwd(entry, mode, N, R, ext=True):
        tail = (None, None) if ext else (None,)
        return lib.call(entry, lib.BF16, mode, 2, N, 12, 1, R, None, None, None, 768, None, None, 768, None, None, None, 768, None, 0.125, None, 0,
                        None, *tail)

    for run, entry, ext in ((fwd, "dvlp_attention_fwd_ex", True), (bwd, "dvlp_attention_bwd_ex", True),
                            (fwd, "dvlp_attention_fwd", False), (bwd, "dvlp_attention_bwd", False)):
        with pytest.raises(lib.DemoVLPHipError, match="bad shape"):
            run(entry, 1, 129, 129, ext)                                # more keys than the kernels stage
        with pytest.raises(lib.DemoVLPHipError, match="bad shape"):
            run(entry, 1, 100, 99, ext)                                 # R != N
        with pytest.raises(lib.DemoVLPHipError, match="not supported"):
            run(entry, 2, 100, 100, ext)                                # no such mode
    with pytest.raises(lib.DemoVLPHipError, match="bad shape"):
        lib.call("dvlp_dropout_attn_mask", 36, 100, 1.0, None, 0, None, None, None)
    with pytest.raises(lib.DemoVLPHipError, match="bad shape"):
        lib.call("dvlp_dropout_attn_mask", 36, 0, 0.1, None, 0, None, None, None)


def test_space_attention_entries_refuse_what_they_do_not_serve(lib):
    """Space / time attention (mode 0) serves N == 1 + F*R tokens with at most 127 tokens per segment (CLS + R keys are staged together), positive
    B, H, N, fp32 or bf16, and its backward needs a workspace.  Each is refused on the host with the documented status (null tensors: nothing
    may be launched), by the `_ex` entries and the plain ones."""
    def fwd(entry, ext, dtype, B, N, H, F, R):
        tail = (None, None) if ext else (None,)                         # (ext,) stream
        return lib.call(entry, dtype, 0, B, N, H, F, R, None, None, None, 2304, None, None, 768, 0.125, None, None, *tail)

    host_ws = (ctypes.c_float * 16)()                                    # a non-null workspace: a shape refusal must not be the missing workspace's

    def bwd(entry, ext, dtype, B, N, H, F, R, ws=host_ws):
        tail = (None, None) if ext else (None,)
        return lib.call(entry, dtype, 0, B, N, H, F, R, None, None, None, 2304, None, None, 768, None, None, None, 2304, ws, 0.125, None, 0,
                        None, *tail)

    for run, entry, ext in ((fwd, "dvlp_attention_fwd_ex", True), (bwd, "dvlp_attention_bwd_ex", True),
                            (fwd, "dvlp_attention_fwd", False), (bwd, "dvlp_attention_bwd", False)):
        for dtype in (lib.F32, lib.BF16):
            for B, N, H, F, R in ((2, 1 + 3 * 17 + 1, 12, 3, 17), (2, 3 * 17, 12, 3, 17),          # N != 1 + F*R, either side
                                  (2, 1 + 3 * 128, 12, 3, 128),                                    # R + 1 keys > 128
                                  (0, 52, 12, 3, 17), (-1, 52, 12, 3, 17), (2, 52, 0, 3, 17), (2, 52, -12, 3, 17),
                                  (2, 0, 12, 0, 17), (2, -50, 12, -3, 17)):                        # (N <= 0 that still equals 1 + F*R)
                with pytest.raises(lib.DemoVLPHipError, match="bad shape"):
                    run(entry, ext, dtype, B, N, H, F, R)
        for dtype in (2, -1, 7):
            with pytest.raises(lib.DemoVLPHipError, match="dtype"):
                run(entry, ext, dtype, 2, 52, 12, 3, 17)
    # a valid shape (the dtype cases above got past the shape check with it), no workspace: only the workspace test can refuse it
    for entry, ext in (("dvlp_attention_bwd_ex", True), ("dvlp_attention_bwd", False)):
        for dtype in (lib.F32, lib.BF16):
            with pytest.raises(lib.DemoVLPHipError, match="bad shape"):
                bwd(entry, ext, dtype, 2, 52, 12, 3, 17, ws=None)
        with pytest.raises(lib.DemoVLPHipError, match="dtype"):                                   # the dtype is named before the missing workspace
            bwd(entry, ext, 7, 2, 52, 12, 3, 17, ws=None)


def test_no_reference_or_oracle_import_in_product():
    """The shipped package must never import the oracle (or /root/reference)."""
    pkg = os.path.join(ROOT, "demovlp_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
                assert "/root/reference" not in src, f
