"""The plain 16-bit main loop of gemm4w on v_mfma_f32_16x16x32 (two products per K-tile of 64 k) and the epilogues that read its
16 x 16 accumulator tiles for the first time: 16-bit rows with the folded LayerNorm (+ erf-GELU), the per-head scatter with the
fold, f32 rows + row partials with and without the residual LayerNorm, and the arena rows.

Every case runs the forced 4-wave kernel ($VIDIL_GEMM4W=1, or $VIDIL_GEMM4W128=1 for the 128-row form where it is built: plain 16-bit
rows and plain arena rows) and compares it
  * with what serves the problem when gemm4w is switched off ($VIDIL_GEMM4W=0: gemm256, still on v_mfma_f32_32x32x16; for the plain
    epilogues of the 128-row form at this size the small-tile kernel, itself bit-identical to gemm256) — bit for bit;
  * with the fp64 product of the rounded operands pushed through the epilogue in fp64, within the bound tests/test_gemm4w_gpu.py uses
    for that epilogue: f32 rows rtol 1e-4, atol 2e-3 * sqrt(K / 768); 16-bit rows behind the fold rtol = atol = 3e-2.  Arena rows
    are compared there with the ROUNDED f32 GEMM for equality; against fp64 that is one unit in the last place of the 16-bit type
    (2^-10 / 2^-7 relative) on top of the f32 bound.  Row partials: the f32 bound of the 64 elements they sum (see _partials_close).

Shapes: M = 300 is one full 256-row tile and a 44-row edge (three 128-row tiles, the last with 44 rows).  N = 248 — a column edge
whose last quad meets the N - 4 clamp — wherever the epilogue takes it; the row partials need N % 64 == 0 and the scatters
N % (H * 64) == 0, so those use N = 320 / 384: one full 256-column tile and an edge tile of 64 / 128 columns, in which whole
64-column halves and a whole wave column lie past N.  K = 64, 128, 192 are 1, 2 and 3 K-tiles — but vidil_gemm gives a 256-column
kernel only K >= 128 (vidil_gemm256_eligible): with K = 64 the epilogues that exist on those kernels alone are refused at the entry
point and the plain ones run on the small-tile kernel whatever the switches say, so the FIRST-and-LAST iteration cannot be launched;
the K = 64 cases pin exactly that.  K = 128 is first + last with no middle iteration, K = 192 the first launch with one.

Row statistics: the rows of every LayerNorm input here are scaled by 1 + row / 37 and shifted by a row-dependent offset, so rstd
and mean * rstd differ from row to row by tens of percent — a wrong (row tile, group) -> lane mapping of the statistics cannot
cancel."""
import os

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
M = 300
DTYPES = [torch.float16, torch.bfloat16]
KS = [64, 128, 192]
ULP16 = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


def _k():
    from vidil_amd import kernels
    return kernels


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _run(env, fn):
    old = {k: os.environ.get(k) for k in gc.ENV_KEYS}
    try:
        for k in gc.ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


OFF = {"VIDIL_GEMM4W": "0", "VIDIL_GEMM4W128": "0"}
ON256 = {"VIDIL_GEMM4W": "1", "VIDIL_GEMM4W128": "0"}
ON128 = {"VIDIL_GEMM4W128": "1"}


def _is_4w(name, tm):
    return name.startswith("gemm4w_kernel") and name.endswith(f", {tm}, false>")


def _f32_atol(K):
    return 2e-3 * (K / 768) ** 0.5


def _rows(K, seed):
    """LayerNorm input rows whose statistics differ per row: scaled by 1 + row / 37, shifted by ((row % 7) - 3) / 2."""
    r = torch.arange(M, dtype=torch.float32)[:, None]
    return _rand(M, K, seed=seed) * 1.5 * (1.0 + r / 37.0) + ((r % 7) - 3.0) * 0.5


def _row_partials(x32):
    m, d = x32.shape
    xs = x32.view(m, d // 64, 64)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).contiguous()


def _ln_of_partials(st, width, eps):
    """(rstd, mean * rstd) in fp64 of the rows whose f32 partials are `st` — the formula of the kernels."""
    s, ss = st[..., 0].double().sum(-1), st[..., 1].double().sum(-1)
    mean = s / width
    var = (ss / width - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return rstd[:, None], (mean * rstd)[:, None]


_FOLD = {}


def _fold_operands(dtype, K, N):
    """x16 [M, K], its row partials, folded W' / b' / colsum, and the fp64 value of LayerNorm(x16) . W^T + b in the folded form."""
    key = (dtype, K, N)
    if key not in _FOLD:
        from vidil_amd.packing import fold_layernorm

        x16 = _rows(K, 100 + K).to(dtype)
        st = _row_partials(x16.float())
        g, bt = _rand(K, seed=101) * 0.2 + 1.0, _rand(K, seed=102) * 0.2
        wf, bf, cs = fold_layernorm(_rand(N, K, scale=0.1, seed=103 + N), _rand(N, seed=104) * 0.1, g, bt, dtype)
        rstd, mrs = _ln_of_partials(st, K, 1e-6)
        ref = rstd * (x16.double() @ wf.double().t()) - mrs * cs.double()[None, :] + bf.double()[None, :]
        _FOLD[key] = (x16.to(DEV), st.to(DEV), wf.to(DEV), bf.to(DEV), cs.to(DEV), ref)
    return _FOLD[key]


def _refused(fn):
    from vidil_amd._lib import VidilHipError

    with pytest.raises(VidilHipError, match="K >= 128"):
        fn()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
def test_folded_layernorm_gelu_rows_equal_gemm256_and_fp64(dtype, K):
    k = _k()
    N = 248
    x16, st, wf, bf, cs, ref = _fold_operands(dtype, K, N)
    call = lambda: k.gemm(x16, wf, bf, act=k.ACT_GELU_ERF, ln=(cs, 1e-6, st))
    if K < 128:
        _refused(lambda: _run(ON256, call))
        return
    assert _is_4w(_run(ON256, lambda: k.gemm_kernel_name(x16, wf, bf, act=k.ACT_GELU_ERF, ln=(cs, 1e-6, st))), 4)
    assert "gemm256_kernel" in _run(OFF, lambda: k.gemm_kernel_name(x16, wf, bf, act=k.ACT_GELU_ERF, ln=(cs, 1e-6, st)))
    got, base = _run(ON256, call), _run(OFF, call)
    want = torch.nn.functional.gelu(ref)
    d = (got.cpu().double() - want).abs().max().item()
    print(f"fold + erf-GELU {dtype} K = {K}: max|d| vs fp64 {d:.3e}, |ref| max {want.abs().max().item():.2f}")
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))
    assert torch.allclose(got.cpu().double(), want, rtol=3e-2, atol=3e-2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["rows", "tiled"])
@pytest.mark.parametrize("K", KS)
def test_folded_per_head_scatter_equals_gemm256_and_fp64(dtype, layout, K):
    """Q | K | V of 12 sequences of 25 tokens (a sequence straddles every 16- and 32-row boundary), 2 heads: N = 384."""
    k = _k()
    H, T, B = 2, 25, 12
    D = H * 64
    N = 3 * D
    x16, st, wf, bf, cs, ref = _fold_operands(dtype, K, N)
    cap = 32
    tiled = layout == "tiled"

    def call():
        q = torch.zeros(B, H, T, 64, dtype=dtype, device=DEV)
        kk = torch.zeros(B, H, cap, 64, dtype=dtype, device=DEV)
        v = torch.zeros(B, H, cap, 64, dtype=dtype, device=DEV)
        hd = dict(q=q, k=kk, vt=v, T=T, H=H, part0=0, t_off=3, Tq_cap=T, Tk_cap=cap, NP=0, q_scale=0.125, tiled=tiled)
        name = k.gemm_kernel_name(x16, wf, bf, heads=hd, ln=(cs, 1e-6, st))
        k.gemm(x16, wf, bf, heads=hd, ln=(cs, 1e-6, st))
        return name, q, kk, v

    if K < 128:
        _refused(lambda: _run(ON256, call))
        return
    (name, *got), (name0, *base) = _run(ON256, call), _run(OFF, call)
    assert _is_4w(name, 4) and "gemm256_kernel" in name0, (name, name0)
    for g_, b_ in zip(got, base):
        assert torch.equal(g_.view(torch.int16), b_.view(torch.int16))
    # fp64: element (m, part, h, d) -> its place in q / k / v
    m = np.arange(M)[:, None]
    b, t = m // T, m % T
    hcol = np.arange(D)[None, :]
    h, d = hcol // 64, hcol % 64
    want_q = torch.zeros(B, H, T, 64, dtype=torch.float64)
    want_q.view(-1)[torch.from_numpy(((b * H + h) * T + t) * 64 + d).reshape(-1)] = (ref[:, :D] * 0.125).reshape(-1)
    assert torch.allclose(got[0].cpu().double(), want_q, rtol=3e-2, atol=3e-2)
    for part, name_ in ((1, "k"), (2, "v")):
        if tiled:
            off = gc.ktile_off(3 + t, d) if part == 1 else gc.vtile_off(3 + t, d)
        else:
            off = (3 + t) * 64 + d
        want = torch.zeros(B, H, cap, 64, dtype=torch.float64)
        want.view(-1)[torch.from_numpy((b * H + h) * cap * 64 + off).reshape(-1)] = ref[:, part * D:(part + 1) * D].reshape(-1)
        assert torch.allclose(got[part].cpu().double(), want, rtol=3e-2, atol=3e-2), name_


def _partials_close(st, ref, tol):
    """Row partials of rows that are each within `tol` (elementwise) of `ref`: a sum of 64 elements moves by at most 64 tol, a sum
    of 64 squares by at most sum(2 |ref| tol + tol^2); f32 summation of 64 terms adds 64 * 2^-24 of the sum of magnitudes."""
    m, n = ref.shape
    r = ref.view(m, n // 64, 64)
    t = tol.view(m, n // 64, 64)
    want_s, want_ss = r.sum(-1), (r * r).sum(-1)
    bound_s = t.sum(-1) + 64 * 2.0 ** -24 * r.abs().sum(-1)
    bound_ss = (2 * r.abs() * t + t * t).sum(-1) + 64 * 2.0 ** -24 * want_ss
    st = st.cpu().double()
    return bool(((st[..., 0] - want_s).abs() <= bound_s).all()) and bool(((st[..., 1] - want_ss).abs() <= bound_ss).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rln", [False, True])
@pytest.mark.parametrize("K", KS)
def test_f32_rows_with_row_partials_and_residual_layernorm_equal_gemm256_and_fp64(dtype, rln, K):
    """out = [LayerNorm](resid) + A . W^T + bias in place, the 16-bit copy and the (sum, sum of squares) per 64 columns."""
    k = _k()
    N = 320
    a = _rand(M, K, seed=201).to(dtype)
    w = _rand(N, K, scale=0.05, seed=202).to(dtype)
    bias = _rand(N, seed=203)
    r = torch.arange(M, dtype=torch.float32)[:, None]
    u = _rand(M, N, seed=204) * 1.3 * (1.0 + r / 37.0) + ((r % 7) - 3.0) * 0.5
    gr, br = _rand(N, seed=205) * 0.2 + 1.0, _rand(N, seed=206) * 0.2
    st_in = _row_partials(u)
    res = u.double()
    if rln:
        rstd, mrs = _ln_of_partials(st_in, N, 1e-12)
        res = (res * rstd - mrs) * gr.double()[None, :] + br.double()[None, :]
    ref = a.double() @ w.double().t() + bias.double()[None, :] + res
    ad, wd, bd, ud = a.to(DEV), w.to(DEV), bias.to(DEV), u.to(DEV)
    kw = dict(rln=(gr.to(DEV), br.to(DEV), 1e-12, st_in.to(DEV))) if rln else {}

    def call():
        x = ud.clone()
        x16 = torch.zeros(M, N, dtype=dtype, device=DEV)
        st = torch.zeros(M, N // 64, 2, device=DEV)
        name = k.gemm_kernel_name(ad, wd, bd, out=x, resid=x, out16=x16, ln_stats_out=st, **kw)
        k.gemm(ad, wd, bd, out=x, resid=x, out16=x16, ln_stats_out=st, **kw)
        return name, x, x16, st

    if K < 128:
        _refused(lambda: _run(ON256, call))
        return
    (name, x, x16, st), (name0, x0, x16_0, st0) = _run(ON256, call), _run(OFF, call)
    assert _is_4w(name, 4) and "gemm256_kernel" in name0, (name, name0)
    assert torch.equal(x, x0) and torch.equal(x16.view(torch.int16), x16_0.view(torch.int16)) and torch.equal(st, st0)
    d = (x.cpu().double() - ref).abs().max().item()
    print(f"f32 + partials{' + residual LayerNorm' if rln else ''} {dtype} K = {K}: max|d| vs fp64 {d:.3e}, |ref| max {ref.abs().max().item():.2f}")
    tol = 1e-4 * ref.abs() + _f32_atol(K)
    assert bool(((x.cpu().double() - ref).abs() <= tol).all())
    assert bool(((x16.cpu().double() - ref).abs() <= tol + ULP16[dtype] * ref.abs()).all())
    assert _partials_close(st, ref, tol)


_ARENA = {}


def _arena_operands(dtype, K, fold):
    key = (dtype, K, fold)
    if key not in _ARENA:
        H = 2
        N = 3 * H * 64
        if fold:
            x16, st, wf, bf, cs, ref = _fold_operands(dtype, K, N)
            _ARENA[key] = (x16, wf, bf, dict(ln=(cs, 1e-6, st)), ref)
        else:
            a = _rand(M, K, seed=301).to(dtype)
            w = _rand(N, K, scale=0.05, seed=302).to(dtype)
            bias = _rand(N, seed=303)
            ref = a.double() @ w.double().t() + bias.double()[None, :]
            _ARENA[key] = (a.to(DEV), w.to(DEV), bias.to(DEV), {}, ref)
    return _ARENA[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["256-row, folded LayerNorm", "128-row, plain"])
@pytest.mark.parametrize("K", KS)
def test_arena_rows_of_single_token_sequences_behind_an_offset_equal_the_other_kernels_and_fp64(dtype, form, K):
    """T = 1, t_off = 5, every third arena slot: Q rows + K / V rows at position 5 of a 16-position arena, 2 heads (N = 384).  The
    256-row kernel takes the arena epilogue at this size with the folded LayerNorm (the decode steps' Q | K | V), the 128-row form
    without it."""
    k = _k()
    fold = form.startswith("256")
    H, T, t_off, Tcap, stride = 2, 1, 5, 16, 3
    D = H * 64
    a, w, bias, kw, ref = _arena_operands(dtype, K, fold)
    rows = (M - 1) * stride + 1
    qs = 0.125

    def call():
        q = torch.zeros(M, D, dtype=dtype, device=DEV)
        ka = torch.zeros(Tcap, rows, D, dtype=dtype, device=DEV)
        va = torch.zeros(Tcap, rows, D, dtype=dtype, device=DEV)
        ar = dict(q=q, k=ka, v=va, T=T, H=H, part0=0, t_off=t_off, arena_rows=rows, slot_stride=stride, Tcap=Tcap, q_scale=qs)
        name = k.gemm_kernel_name(a, w, bias, arena=ar, **kw)
        k.gemm(a, w, bias, arena=ar, **kw)
        return name, q, ka, va

    on = ON256 if fold else ON128
    if K < 128 and fold:
        _refused(lambda: _run(on, call))
        return
    (name, *got), (name0, *base) = _run(on, call), _run(OFF, call)
    if K < 128:
        assert "gemm4w_kernel" not in name, name        # (no 256-column kernel below K = 128: the switch changes nothing)
    else:
        assert _is_4w(name, 4 if fold else 2), name
    assert "gemm4w_kernel" not in name0, name0
    for g_, b_ in zip(got, base):
        assert torch.equal(g_.view(torch.int16), b_.view(torch.int16))
    rtol, atol = (3e-2, 3e-2) if fold else (1e-4 + ULP16[dtype], _f32_atol(K))
    want_q = ref[:, :D] * qs
    assert bool(((got[0].cpu().double() - want_q).abs() <= rtol * want_q.abs() + atol).all())
    for part in (1, 2):
        arena = got[part].cpu().double()
        want = ref[:, part * D:(part + 1) * D]
        assert bool(((arena[t_off, ::stride] - want).abs() <= rtol * want.abs() + atol).all())
        arena[t_off, ::stride] = 0
        assert bool((arena == 0).all())          # (nothing outside position t_off of the sequences' slots)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
def test_gelu_rows_of_the_128_row_form_equal_the_small_tile_kernel_and_fp64(dtype, K):
    """16-bit rows + erf-GELU without the fold on 128-row tiles (the 256-row kernel takes this epilogue only on grids that fill the
    chip: tests/test_gemm4w_gpu.py), ragged N = 248."""
    k = _k()
    N = 248
    a = _rand(M, K, seed=401).to(dtype).to(DEV)
    w = _rand(N, K, scale=0.05, seed=402).to(dtype).to(DEV)
    bias = _rand(N, seed=403).to(DEV)
    ref = torch.nn.functional.gelu(a.cpu().double() @ w.cpu().double().t() + bias.cpu().double()[None, :])
    name = _run(ON128, lambda: k.gemm_kernel_name(a, w, bias, act=k.ACT_GELU_ERF))
    assert _is_4w(name, 2) if K >= 128 else "gemm4w_kernel" not in name, name
    got = _run(ON128, lambda: k.gemm(a, w, bias, act=k.ACT_GELU_ERF))
    base = _run(OFF, lambda: k.gemm(a, w, bias, act=k.ACT_GELU_ERF))
    assert torch.equal(got.view(torch.int16), base.view(torch.int16))
    # (the bound of the f16 GELU rows in tests/test_gemm4w_gpu.py; bf16 rounds to 2^-9 relative where f16 rounds to 2^-12: that
    #  difference on top for bf16)
    rtol = 3e-3 if dtype == torch.float16 else 3e-3 + 2.0 ** -9 - 2.0 ** -12
    assert torch.allclose(got.cpu().double(), ref, rtol=rtol, atol=3e-3)
