"""The backward forms of vidil_gemm (VIDIL_EPI_GRAD_IN: dX = dY · W, VIDIL_EPI_GRAD_W: dW = dY^T · X) against fp64: exact
tier at every tile / step / split edge, confinement of the stores, untouched memory behind the contraction edge, resid,
determinism, and the derived rounding bound (include/vidil_hip.h "Backward forms"; cases in gemm_grad_cases.py)."""
import numpy as np
import pytest
import torch

import gemm_grad_cases as G
from vidil_amd import kernels as K

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
SENT = 12345.0          # sentinel in every f32 element a launch must not write
GUARD = 1024            # f32 elements of guard allocation before and after out
PAD_ROWS = 128          # rows of NaN behind the last valid row of A and W (one tile: mapped, never to be read)
WS_GUARD = 4096         # bytes behind the workspace


def _dev():
    return torch.device("cuda:0")


def _launch(case, dtype, a, w, *, ldo_extra=8, resid=None, poison=False, extra_rows=3):
    """Run one case with sentinels around everything the launch may write and (poison) NaNs around everything it may read.
    a, w: numpy [rows, valid columns] operands.  resid: None, "alias" or "separate" (an f32 numpy array is drawn).
    Returns (out [R, C] on the host, resid values or None); asserts that every sentinel survived."""
    form, M, N, Kc, lda = case
    R, C, L = G.dims(form, M, N, Kc)
    dev = _dev()
    (ar, astride, ac), (wr, wc) = G.operand_shapes(*case)
    fill = float("nan") if poison else 0.0
    abuf = torch.full((ar + PAD_ROWS, astride), fill, dtype=dtype, device=dev)
    abuf[:ar, :ac] = torch.from_numpy(np.asarray(a, np.float32)).to(dtype).to(dev)
    wbuf = torch.full((wr + PAD_ROWS, wc), fill, dtype=dtype, device=dev)
    wbuf[:wr] = torch.from_numpy(np.asarray(w, np.float32)).to(dtype).to(dev)
    ldo = C + ldo_extra
    whole = torch.full((GUARD + (R + extra_rows) * ldo + GUARD,), SENT, dtype=torch.float32, device=dev)
    out = whole[GUARD:GUARD + R * ldo].view(R, ldo)
    rv = None
    rt = None
    if resid is not None:
        rng = np.random.default_rng(7)
        rv = rng.integers(-1000, 1001, size=(R, C)).astype(np.float32)
        if resid == "alias":
            out[:, :C] = torch.from_numpy(rv).to(dev)
            rt = out
        else:
            rt = torch.full((R, ldo), SENT, dtype=torch.float32, device=dev)
            rt[:, :C] = torch.from_numpy(rv).to(dev)
    need = K.gemm_grad_ws_bytes(form, M, N, Kc)
    ws = torch.full((need + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    fn = K.gemm_grad_input if form == G.GRAD_IN else K.gemm_grad_weight
    strided = lda != 0                      # (dense cases go through the library's lda == 0 path)
    ret = fn(abuf[:ar], wbuf[:wr], out=out, resid=rt, M=M if strided else None, lda=astride if strided else None, workspace=ws)
    torch.cuda.synchronize()
    assert ret is out
    host = whole.cpu()
    assert torch.all(host[:GUARD] == SENT) and torch.all(host[GUARD + R * ldo:] == SENT), "guard allocation or a row past the last written"
    grid = host[GUARD:GUARD + R * ldo].view(R, ldo)
    assert torch.all(grid[:, C:] == SENT), "columns C .. ldo - 1 written"
    assert torch.all(ws[need:].cpu() == 0xA5), "bytes behind the workspace written"
    if resid == "separate":
        assert torch.equal(rt[:, :C].cpu(), torch.from_numpy(rv)) and torch.all(rt[:, C:].cpu() == SENT), "resid modified"
    return grid[:, :C].clone().numpy(), rv


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", G.EXACT_CASES, ids=G.case_id)
def test_exact_tier(case, dtype):
    """Small-integer operands: bit equality with fp64 at every edge, inside sentinels, with NaNs in A's pad columns and in the
    rows behind the last valid row of A and W."""
    a, w = G.exact_operands(case)
    ref, _ = G.reference(case[0], a, w)
    got, _ = _launch(case, dtype, a, w, poison=True)
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.float64), ref), f"max |d| = {np.abs(got - ref).max()}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", G.PATH_CASES, ids=G.case_id)
def test_confinement_and_poison(case, dtype):
    """The same bits with zeros and with NaNs around the operands (rounded operands: nothing hides a stray term)."""
    a, w = G.normal_operands(case)
    clean, _ = _launch(case, dtype, a, w, poison=False)
    dirty, _ = _launch(case, dtype, a, w, poison=True)
    assert np.isfinite(dirty).all()
    assert np.array_equal(clean.view(np.uint32), dirty.view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("mode", ["alias", "separate"])
@pytest.mark.parametrize("case", G.PATH_CASES, ids=G.case_id)
def test_resid(case, mode, dtype):
    """out = product + resid, exactly on the exact tier (integers below 2^24), aliased and not."""
    a, w = G.exact_operands(case)
    ref, _ = G.reference(case[0], a, w)
    got, rv = _launch(case, dtype, a, w, resid=mode, poison=True)
    assert np.array_equal(got.astype(np.float64), ref + rv.astype(np.float64))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", G.PATH_CASES, ids=G.case_id)
def test_determinism(case, dtype, monkeypatch):
    """Equal bits: twice, inside a larger ldo, and with the forward kernels' selection switches set either way."""
    a, w = G.normal_operands(case, seed=1)
    first, _ = _launch(case, dtype, a, w)
    again, _ = _launch(case, dtype, a, w)
    wide, _ = _launch(case, dtype, a, w, ldo_extra=72, extra_rows=1)
    bits = first.view(np.uint32)
    assert np.array_equal(bits, again.view(np.uint32))
    assert np.array_equal(bits, wide.view(np.uint32))
    for v256, v4w in (("0", "0"), ("1", "1"), ("0", "1"), ("1", "0")):
        monkeypatch.setenv("VIDIL_GEMM256", v256)
        monkeypatch.setenv("VIDIL_GEMM4W", v4w)
        sw, _ = _launch(case, dtype, a, w)
        assert np.array_equal(bits, sw.view(np.uint32)), (v256, v4w)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", G.PATH_CASES + [(G.GRAD_W, 2049, 2, 8, 8), (G.GRAD_IN, 129, 264, 200, 208)], ids=G.case_id)
def test_rounded_tier(case, dtype):
    """Normal operands rounded to T16 against fp64 of the rounded operands: |error| <= (L + 8) 2^-24 sum |a||b| per element."""
    a, w = G.normal_operands(case, seed=2)
    a16 = torch.from_numpy(a).to(dtype).double().numpy()
    w16 = torch.from_numpy(w).to(dtype).double().numpy()
    ref, sabs = G.reference(case[0], a16, w16)
    got, _ = _launch(case, dtype, a16, w16, poison=True)
    L = G.dims(*case[:4])[2]
    err = np.abs(got.astype(np.float64) - ref)
    bound = G.rounded_bound(L, sabs)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{G.case_id(case)} {dtype}: worst error / bound = {worst:.3f}")
    assert (err <= bound).all(), worst


def test_kernel_names_and_workspace_errors():
    dev = _dev()
    dy = torch.zeros((263, 40), dtype=torch.bfloat16, device=dev)
    x = torch.zeros((263, 72), dtype=torch.bfloat16, device=dev)
    out = torch.zeros((33, 72), dtype=torch.float32, device=dev)
    need = K.gemm_grad_ws_bytes(K.EPI_GRAD_W, 263, 33, 72)
    assert need == 4 * 3 * 33 * 72
    with pytest.raises(K.VidilHipError, match="workspace"):
        K.gemm_grad_weight(dy, x, out=out, M=263, lda=40, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    # allocated by the wrapper when none is given
    got = K.gemm_grad_weight(dy, x, out=out, M=263, lda=40)
    torch.cuda.synchronize()
    assert torch.all(got == 0)
