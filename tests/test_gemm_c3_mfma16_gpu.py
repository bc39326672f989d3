"""The compensated (C3, split_k) main loop of gemm4w on v_mfma_f32_16x16x32, both tile heights, and the epilogues it reaches
through the 16 x 16 accumulator view of gemm_epilogue.inc.

  * K-tile count edges: vidil_gemm takes K in multiples of 64 and the compensated form K = 3 Kl in multiples of 96, so Kl is a
    multiple of 64 and a tile has an EVEN number nk = Kl / 32 of K-tiles: Kl = 64, 128, 192 are nk = 2 (the FIRST and the LAST
    variant of the iteration back to back), 4 and 6 (the middle variant twice / four times); nk = 1 and odd nk (Kl = 32, 96) do
    not exist behind the library's entry point, which the last test pins.  On the 128-row form (M = 300, N = 248: ragged rows
    and columns) and the 256-row form (M = 160 * 256 - 8, N = 256: the smallest grid the dispatcher gives 256-row tiles),
    against the fp64 product of the split operands.
  * Error bound: the yardstick is the 32x32x16 loop this one replaced, on the same inputs (PARENT_MAX_D, measured with that
    build of the library and recorded in profiles/c3_mfma16_ab.md): within 2x of it plus 1e-6 — a regrouped f32 sum may land on
    either side, a factor of 2 separates regrouping from a lost product — and within 1e-5 * max(1, |ref|) + 1e-5.
  * Same bits in both tile heights: rows 0, 1, M/2, M-1 multiplied alone (128-row tiles) equal the same rows of the full problem
    (256-row tiles) for every f32 epilogue form and the patch epilogue.
  * Per-head scatter in every layout the mode uses, against the K-tripled launch by the ordinal rule of test_parity_mode_gpu."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

M128, N128 = 300, 248
M256, N256 = 160 * 256 - 8, 256

# max |d| against the fp64 product of the split operands of the 32x32x16 C3 loop (the parent of this change), same inputs
PARENT_MAX_D = {
    (128, 64): 4.1318e-07,
    (128, 128): 7.6259e-07,
    (128, 192): 1.1508e-06,
    (256, 64): 6.7904e-07,
    (256, 128): 1.1833e-06,
    (256, 192): 1.6110e-06,
}


def _k():
    from vidil_amd import kernels
    return kernels


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _split(x, dtype=torch.float16):
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    return hi, lo


_OPS = {}


def _operands(M, N, Kl):
    """(a3 [M, 3 Kl], w3 [N, 3 Kl], bias, fp64 product of the split operands + bias), computed once per shape."""
    key = (M, N, Kl)
    if key not in _OPS:
        from vidil_amd.packing import w3

        k = _k()
        x = _rand(M, Kl, seed=11 + Kl)
        w = _rand(N, Kl, scale=0.05, seed=12 + Kl)
        bias = _rand(N, seed=13)
        xh, xl = _split(x)
        wh, wl = _split(w)
        ref = (xh.double() + xl.double()) @ (wh.double() + wl.double()).t() + bias.double()
        a3 = k.split3(x.to(DEV), torch.empty(M, 3 * Kl, dtype=torch.float16, device=DEV))
        assert torch.equal(a3[:, :Kl].cpu(), xh) and torch.equal(a3[:, Kl:2 * Kl].cpu(), xl)
        _OPS[key] = (a3, w3(w, dtype=torch.float16).to(DEV), bias.to(DEV), ref)
    return _OPS[key]


def _form(name):
    assert name.startswith("gemm4w_kernel") and name.endswith(", true>"), name
    return 256 if name.endswith(", 4, true>") else 128


@pytest.mark.parametrize("rows,Kl", [(128, 64), (128, 128), (128, 192), (256, 64), (256, 128), (256, 192)])
def test_k_tile_count_edges_in_both_tile_heights_against_fp64_and_the_32x32_loop(rows, Kl):
    k = _k()
    M, N = (M128, N128) if rows == 128 else (M256, N256)
    a3, w3d, bias, ref = _operands(M, N, Kl)
    name = k.gemm_kernel_name(a3, w3d, bias, out_dtype=torch.float32, split_k=True)
    assert _form(name) == rows, name
    got = k.gemm(a3, w3d, bias, out_dtype=torch.float32, split_k=True)
    d = (got.cpu().double() - ref).abs().max().item()
    parent = PARENT_MAX_D.get((rows, Kl))
    print(f"C3 {rows}-row form, Kl = {Kl} (nk = {Kl // 32}): max|d| vs fp64 {d:.3e} (32x32x16 loop: {parent}) |ref| max {ref.abs().max().item():.2f}")
    assert d <= 1e-5 * max(1.0, ref.abs().max().item()) + 1e-5
    assert parent is not None, "no recorded figure of the 32x32x16 loop for this case"
    assert d <= 2 * parent + 1e-6, (d, parent)


def test_a_row_has_the_same_bits_in_both_tile_heights_for_every_f32_form_and_the_patch_epilogue():
    k = _k()
    Kl = 128
    M, N = M256, N256
    a3, w3d, bias, _ = _operands(M, N, Kl)
    rows = torch.tensor([0, 1, M // 2, M - 1], device=DEV)
    sub3 = a3[rows].contiguous()
    res = _rand(M, N, seed=21).to(DEV)
    forms = {
        "plain": (dict(out_dtype=torch.float32), dict(out_dtype=torch.float32)),
        "residual": (dict(out=res.clone(), resid=res), dict(out=res[rows].clone(), resid=res[rows].contiguous())),
        "quick_gelu": (dict(out_dtype=torch.float32, act=k.ACT_QUICK_GELU), dict(out_dtype=torch.float32, act=k.ACT_QUICK_GELU)),
        "split3 x 3": (dict(split3_out=torch.zeros(M, 3 * N, dtype=torch.float16, device=DEV)),
                       dict(split3_out=torch.zeros(4, 3 * N, dtype=torch.float16, device=DEV))),
        "split3 x 2": (dict(split3_out=torch.full((M, 3 * N), 7.0, dtype=torch.float16, device=DEV), split3_planes=2),
                       dict(split3_out=torch.full((4, 3 * N), 7.0, dtype=torch.float16, device=DEV), split3_planes=2)),
    }
    for what, (kw_full, kw_sub) in forms.items():
        assert _form(k.gemm_kernel_name(a3, w3d, bias, split_k=True, **kw_full)) == 256, what
        assert _form(k.gemm_kernel_name(sub3, w3d, bias, split_k=True, **kw_sub)) == 128, what
        full = k.gemm(a3, w3d, bias, split_k=True, **kw_full)
        sub = k.gemm(sub3, w3d, bias, split_k=True, **kw_sub)
        assert torch.equal(sub, full[rows]), what
        if what == "split3 x 2":
            assert bool((full[:, 2 * N:] == 7.0).all()) and not bool((full[:, :2 * N] == 7.0).all())
    # patch embedding (256-row tiles at every size): three images of P tokens against the four rows as one image of 4 tokens whose
    # position rows are the ones those tokens have in the full problem
    P, B = 196, 3
    Mp = B * P
    ap, wp, bp, _ = _operands(Mp, N, Kl)
    pos = _rand(P + 1, N, seed=22).to(DEV)
    out = torch.zeros(B * (P + 1), N, dtype=torch.float32, device=DEV)
    assert _form(k.gemm_kernel_name(ap, wp, bp, patch=dict(out=out, pos=pos, tpi=P), split_k=True)) == 256
    k.gemm(ap, wp, bp, patch=dict(out=out, pos=pos, tpi=P), split_k=True)
    prow = torch.tensor([0, 1, Mp // 2, Mp - 1], device=DEV)
    pos_sub = torch.cat([torch.zeros(1, N, device=DEV), pos[(prow % P) + 1]])
    out_sub = torch.zeros(5, N, dtype=torch.float32, device=DEV)
    k.gemm(ap[prow].contiguous(), wp, bp, patch=dict(out=out_sub, pos=pos_sub, tpi=4), split_k=True)
    assert torch.equal(out_sub[1:], out[prow + prow // P + 1])
    assert bool((out_sub[0] == 0).all()) and bool((out[::P + 1] == 0).all())      # (the class-token rows are not the GEMM's)


def _ordinal_close(a_, b_):
    """test_split_k_gemm_per_head_scatter...'s rule: 16-bit outputs at most one unit in the last place apart, or 4e-6 absolute."""
    ia, ib = a_.view(torch.int16).int(), b_.view(torch.int16).int()
    oa, ob = torch.where(ia >= 0, ia, -(ia & 0x7FFF)), torch.where(ib >= 0, ib, -(ib & 0x7FFF))
    ulps = (oa - ob).abs()
    ok = (ulps <= 1) | ((a_.float() - b_.float()).abs() <= 4e-6)
    return bool(ok.all()), (ulps > 0).float().mean().item()


@pytest.mark.parametrize("B,T,layout", [(3, 197, "kv_tiled"), (3, 197, "kv_rows_vt"), (3, 197, "qkv_rows"), (3, 197, "qkv_vt"),
                                         (40, 8, "kv_tiled"), (40, 8, "kv_rows_vt"), (208, 197, "kv_tiled"), (5120, 8, "kv_tiled")])
def test_per_head_scatter_layouts_equal_the_k_tripled_launch_to_rounding(B, T, layout):
    """T = 197 (a sequence straddles every 16- and 32-row boundary; 591 rows end in a ragged tile) and T = 8 (the shortest the form
    takes), K | V as fragment tiles, as rows + V^T, Q | K | V with row-major V and with V^T; the last two shapes fill the chip
    (256-row tiles)."""
    k = _k()
    H, Kl = 2, 128
    M = B * T
    kv = layout.startswith("kv")
    N = (2 if kv else 3) * H * 64
    a3, w3d, bias, _ = _operands(M, N, Kl)
    Tc = (T + 31) // 32 * 32
    NP = (T + 15) // 16 * 16
    outs = []
    for sk in (True, False):
        q = torch.zeros(B, H, T, 64, dtype=torch.float16, device=DEV)
        kk = torch.zeros(B, H, Tc, 64, dtype=torch.float16, device=DEV)
        if layout.endswith("vt"):
            vv = torch.zeros(B, H, 64, NP, dtype=torch.float16, device=DEV)
        else:
            vv = torch.zeros(B, H, Tc, 64, dtype=torch.float16, device=DEV)
        heads = dict(k=kk, vt=vv, T=T, H=H, part0=1 if kv else 0, t_off=0, Tk_cap=Tc, NP=NP if layout.endswith("vt") else 0,
                     tiled=layout == "kv_tiled")
        if not kv:
            heads.update(q=q, Tq_cap=T, q_scale=0.125)
        if sk:
            name = k.gemm_kernel_name(a3, w3d, bias, heads=heads, split_k=True)
            assert _form(name) == (256 if M > 40000 else 128), name
        k.gemm(a3, w3d, bias, heads=heads, split_k=sk)
        outs.append((q, kk, vv))
    for what, a_, b_ in zip("qkv", outs[0], outs[1]):
        if what == "q" and kv:
            continue
        assert bool((a_ != 0).any()), what
        ok, frac = _ordinal_close(a_, b_)
        assert ok and frac < 0.02, (what, (a_.float() - b_.float()).abs().max().item(), frac)


@pytest.mark.parametrize("Kl", [32, 96])
def test_an_odd_number_of_k_tiles_is_refused_at_the_entry_point(Kl):
    """K = 3 Kl = 96 / 288 is no multiple of 64: vidil_gemm refuses it for every form, so the C3 iteration never runs alone
    (FIRST + LAST in one) or an odd number of times."""
    from vidil_amd._lib import VidilHipError

    k = _k()
    a3 = torch.zeros(M128, 3 * Kl, dtype=torch.float16, device=DEV)
    w3d = torch.zeros(N128, 3 * Kl, dtype=torch.float16, device=DEV)
    with pytest.raises(VidilHipError, match="multiple of 64"):
        k.gemm(a3, w3d, None, out_dtype=torch.float32, split_k=True)
