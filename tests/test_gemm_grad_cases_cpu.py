"""The preconditions of tests/gemm_grad_cases.py and the argument checks of the backward GEMM forms, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_grad_cases as G
from vidil_amd import _lib
from vidil_amd import kernels as K


def test_exact_tier_sums_are_exact_in_f32():
    """Every exact-tier case: integer operands (exact in f16 and bf16) with sum |a||b| < 2^24 per output element, so every partial
    sum of products is an integer below 2^24 and f32 addition is exact in any order."""
    assert G.INT_RANGE <= 256 // 2          # bf16 holds integers up to 256 exactly
    for case in G.EXACT_CASES:
        a, w = G.exact_operands(case)
        assert np.array_equal(a, np.round(a)) and np.abs(a).max() <= G.INT_RANGE
        assert np.array_equal(w, np.round(w)) and np.abs(w).max() <= G.INT_RANGE
        for dt in (torch.float16, torch.bfloat16):
            assert torch.equal(torch.from_numpy(a).to(dt).double(), torch.from_numpy(a))
        _, sabs = G.reference(case[0], a, w)
        assert sabs.max() < 2 ** 24, G.case_id(case)
        L = G.dims(*case[:4])[2]
        assert L * G.INT_RANGE ** 2 < 2 ** 24


def test_table_is_inside_the_contract():
    for form, M, N, Kc, lda in G.EXACT_CASES + G.PATH_CASES:
        assert Kc % 8 == 0
        if form == G.GRAD_IN:
            assert N % 8 == 0 and (lda == 0 or (lda >= Kc and lda % 8 == 0))
        else:
            assert (N % 8 == 0) if lda == 0 else (lda >= N and lda % 8 == 0)
    ids = [G.case_id(c) for c in G.EXACT_CASES]
    assert len(set(ids)) == len(ids)


def test_straddles_straddle_what_they_name():
    idx = {"tile": 0, "nsplit": 1, "split_len": 2}
    for what, lo, hi, (vlo, vhi) in G.STRADDLES:
        assert lo in G.EXACT_CASES and hi in G.EXACT_CASES
        assert G.plan(*lo[:4])[idx[what]] == vlo, (what, lo)
        assert G.plan(*hi[:4])[idx[what]] == vhi, (what, hi)
        assert vlo != vhi
    # the constants the straddles are built from
    assert (G.GK, G.BIG_TILES, G.TARGET_BLOCKS, G.MIN_SPLIT, G.MAX_SPLIT) == (64, 64, 512, 128, 16)
    # one and seven rows past one and two split lengths
    for M, ns in ((129, 2), (135, 2), (257, 3), (263, 3)):
        bt, n, ln = G.plan(G.GRAD_W, M, 33, 72)
        assert (bt, n, ln) == (64, ns, 128) and (G.GRAD_W, M, 33, 72, 40) in G.EXACT_CASES
    # every kernel path has a representative
    paths = {(G.plan(*c[:4])[0], G.plan(*c[:4])[1] > 1, c[0]) for c in G.PATH_CASES}
    assert len(paths) == 8


def test_workspace_formula_matches_its_literal_restatement():
    shapes = {c[:4] for c in G.EXACT_CASES} | {(f, M, N, Kc) for f in (G.GRAD_IN, G.GRAD_W)
                                                for M, N, Kc in ((6304, 2304, 768), (6304, 768, 3072), (1024, 30528, 768),
                                                                 (96, 256, 768), (288, 256, 768), (96, 768, 768))}
    for form, M, N, Kc in shapes:
        assert K.gemm_grad_plan(form, M, N, Kc) == G.plan(form, M, N, Kc)
        assert K.gemm_grad_ws_bytes(form, M, N, Kc) == G.ws_bytes(form, M, N, Kc)
    # the ViT dW of the issue: 108 tiles of 128 x 128, four ranges of 1600 rows
    assert G.plan(G.GRAD_W, 6304, 2304, 768) == (128, 4, 1600)
    assert K.gemm_grad_ws_bytes(G.GRAD_W, 6304, 2304, 768) == 4 * 4 * 2304 * 768
    assert K.gemm_grad_ws_bytes(G.GRAD_IN, 1, 8, 8) == 0
    with pytest.raises(K.VidilHipError):
        K.gemm_grad_plan(1, 8, 8, 8)


def _args(form, **kw):
    g = _lib.GemmArgs()
    g.A, g.W, g.out = 16, 32, 48
    g.M, g.N, g.K, g.ldo = 16, 16, 16, 16
    g.epi = form
    g.dtype = _lib.DT_BF16
    for k, v in kw.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("form,name", [(G.GRAD_IN, b"grad_in"), (G.GRAD_W, b"grad_w")])
def test_refusals_go_through_the_library_without_a_gpu(form, name):
    lib = _lib.load()

    def refused(**kw):
        rc = lib.vidil_gemm(ctypes.byref(_args(form, **kw)), None)
        msg = lib.vidil_last_error()
        assert rc == -1 and name in msg, (kw, rc, msg)
        return msg

    refused(bias=16)
    refused(act=_lib.ACT_GELU_ERF)
    refused(ln_fold=1)
    refused(out16=16)
    refused(out16_split3=1)
    refused(ln_stats_out=16)
    refused(rln_gamma=16)
    refused(rln_beta=16)
    refused(split_k=1)
    assert b"fp8" in refused(dtype=_lib.DT_FP8)
    assert b"aligned" in refused(A=24)
    assert b"aligned" in refused(W=8)
    assert b"aligned" in refused(out=52)
    assert b"multiple of 8" in refused(K=12)
    assert b"ldo" in refused(ldo=8)
    if form == G.GRAD_IN:
        assert b"multiple of 8" in refused(N=12, ldo=16)
        refused(lda=8)
        refused(lda=20)
    else:
        refused(N=12)            # dense A needs N % 8 == 0 ...
        refused(N=12, lda=12)
        refused(lda=8)
    # a split contraction without a workspace names the byte count (checked before any launch)
    g = _args(form, M=8 if form == G.GRAD_IN else 264, K=264 if form == G.GRAD_IN else 8, N=8, ldo=264)
    assert lib.vidil_gemm(ctypes.byref(g), None) == -1
    need = G.ws_bytes(form, g.M, g.N, g.K)
    assert need > 0 and str(need).encode() in lib.vidil_last_error() and name in lib.vidil_last_error()
    # accepted arguments: the kernel name and the split_k question answer without a GPU
    ok = _args(form, lda=24)
    buf = ctypes.create_string_buffer(128)
    assert lib.vidil_gemm_kernel_name(ctypes.byref(ok), buf, 128) == 0
    assert buf.value.decode() == f"gemm_grad_kernel<__bf16, {form}, 64>"
    big = _args(form, M=1024, N=1024, K=1024, ldo=1024, dtype=_lib.DT_F16)
    assert lib.vidil_gemm_kernel_name(ctypes.byref(big), buf, 128) == 0
    assert buf.value.decode() == f"gemm_grad_kernel<_Float16, {form}, 128>"
    assert lib.vidil_gemm_split_k_serves(ctypes.byref(ok)) == 0
    # contraction lengths that are no multiple of 64 are inside the contract
    assert lib.vidil_gemm_kernel_name(ctypes.byref(_args(form, M=9, N=8, K=8, ldo=8)), buf, 128) == 0


def test_k_rule_still_refuses_the_forward_forms():
    lib = _lib.load()
    for epi in range(6):
        g = _args(epi, K=72, dtype=_lib.DT_F16)
        assert lib.vidil_gemm(ctypes.byref(g), None) == -1
        assert b"multiple of 64" in lib.vidil_last_error() or b"multiple of 128" in lib.vidil_last_error() or b"fp8" in lib.vidil_last_error()
    g = _args(1, K=72, dtype=_lib.DT_F16)
    assert lib.vidil_gemm(ctypes.byref(g), None) == -1 and b"K=72 must be a multiple of 64" in lib.vidil_last_error()
    g = _args(8, K=64)
    assert lib.vidil_gemm(ctypes.byref(g), None) == -3 and b"unsupported epi" in lib.vidil_last_error()


def test_wrapper_shape_errors():
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    z = lambda *s, dt=bf: torch.zeros(*s, dtype=dt)
    bad = [
        lambda: K.gemm_grad_input(z(4, 16), z(24, 8)),                        # dy columns != w rows
        lambda: K.gemm_grad_input(z(4, 16), z(16, 8, dt=f16)),                # mixed types
        lambda: K.gemm_grad_input(z(4, 16, dt=f32), z(16, 8, dt=f32)),        # not 16-bit
        lambda: K.gemm_grad_input(z(4, 12), z(12, 8)),                        # Nout % 8
        lambda: K.gemm_grad_input(z(4, 16), z(16, 12)),                       # Kin % 8
        lambda: K.gemm_grad_input(z(4, 24), z(16, 8), lda=24),                # lda without M
        lambda: K.gemm_grad_input(z(4, 24), z(16, 8), lda=20, M=4),           # lda % 8
        lambda: K.gemm_grad_input(z(4, 24), z(32, 8), lda=24, M=4),           # lda < Nout
        lambda: K.gemm_grad_input(z(4, 16), z(16, 8), out=z(4, 4, dt=f32)),   # out too narrow
        lambda: K.gemm_grad_input(z(4, 16), z(16, 8), out=z(4, 8)),           # out not f32
        lambda: K.gemm_grad_input(z(4, 16), z(16, 8), out=z(4, 8, dt=f32), resid=z(4, 16, dt=f32)),
        lambda: K.gemm_grad_input(z(4, 16, 1), z(16, 8)),
        lambda: K.gemm_grad_weight(z(4, 16), z(5, 8)),                        # row counts differ
        lambda: K.gemm_grad_weight(z(4, 12), z(4, 8)),                        # dense dy with Nout % 8
        lambda: K.gemm_grad_weight(z(4, 16), z(4, 12)),                       # Kin % 8
        lambda: K.gemm_grad_weight(z(4, 16), z(4, 8), lda=16, M=4),           # strided dy without out
        lambda: K.gemm_grad_weight(z(4, 16), z(4, 8), lda=16, M=4, out=z(20, 8, dt=f32)),   # lda < Nout
        lambda: K.gemm_grad_weight(z(4, 16), z(4, 8), out=z(12, 8, dt=f32)),  # out rows != Nout
        lambda: K.gemm_grad_input(z(1, 3 * 24 + 8), z(16, 8), lda=24, M=4),   # the last row's K = 16 columns reach past dy's end
        lambda: K.gemm_grad_weight(z(1, 3 * 16 + 4), z(4, 8), lda=16, M=4, out=z(12, 8, dt=f32)),   # ... its 8-column chunks
        lambda: K.gemm_grad_weight(z(4, 16), z(4, 8), lda=16, M=4, out=z(12, dt=f32)),              # out not 2-D
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(K.VidilHipError):
            fn()
            pytest.fail(f"wrapper accepted bad call {i}")
    # good shapes fail only at the device check (host tensors: no CPU fallback)
    with pytest.raises(K.VidilHipError, match="CUDA/HIP"):
        K.gemm_grad_input(z(4, 16), z(16, 8))
    for name in ("gemm_grad_input", "gemm_grad_weight", "gemm_grad_ws_bytes"):
        assert name in K.__all__
