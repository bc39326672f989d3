"""Branches and loop passes of the row and selection kernels that the workload's own shapes never execute, against fp64 /
exact-integer references (inputs and references: tests/branch_cases.py; their preconditions: tests/test_branch_cases_cpu.py).

Case -> branch
  kernel                      branch / pass                                              case
  --------------------------  ---------------------------------------------------------  ------------------------------------------
  lsm_topk_kernel (beam.hip)  refresh guard `(it & 7) == 1 && ballot == ~0` on a ragged   V = 1028 (one lane), 1500 (wave 1 partial),
                              iteration                                                  2044 (wave 3 minus a lane), 9220, 9716, 10236
                              vector path, threads with no element (m = -inf), waves     V = 8, 260, 1000
                              with fewer than 2 nb elements
                              scalar path                                                V = 1023, 30521
                              NB = 2 instantiations, plain and penalty                   nb = 2 (every V)
                              penalty form with all 64 cells of hs_tok / one cell        cur_len = 64 / 1
  topk_rows_kernel            threads that hold nothing                                  N = 1, 63, 255
                              more than 64 KB of dynamic LDS through the opt-in          N = 16385, 38400
                              -inf / -1 tails                                            row 2 of every N
                              row_stride > N                                             N = 257 (stride 264)
  layernorm_kernel            VPL = 5 / VPL = 1                                          D = 1280 / D = 256
                              in place (out32 == x, __restrict__, non-temporal loads)     D = 768, 1280
                              SPLIT2 (third plane left alone), fp8, unsupported D         planes = 2, float8_e4m3fn, D = 640
  patchify_f32 / _u8 / _any   second, partial pass of the grid-stride loop               B = 56 / 168 (16, 224), B = 7 (14, 224)
  split3_kernel               second, partial pass                                       1366 x 3072
  embed_tokens_kernel         id clamp; D % 256 != 0                                     ids -5, vocab + 3; D = 260
  l2norm_kernel               D % 256 != 0, one row                                      D = 260, n = 1
  resample_h_kernel           LDS need above 64 KB                                       blip_frames 8 x 3840 -> 224; 16 -> 2400 wide
  resample_v_kernel           out_w * 3 % 4 != 0                                         S = 225; 1023 wide
  resample_h / _v / _v4       second, partial pass of the grid-stride loop               583 x 2400, 1367 x 1023, 5464 x 1024
  beam_attn_kernel<T, 4 / 8>  8 | 9 keys, 32 | 33 keys (MAXJ 4 -> 8), 64 keys; 65 refused  n_keys = 8, 9, 32, 33, 64, 65

Every yardstick and the kernel's worst error against it is printed by its test; the figures of one MI355X run are recorded in
the tests' docstrings.  (The yardsticks are evaluated on the host the test runs on: torch's and numpy's f32 sums are vectorised
differently from CPU to CPU, so they move by a few percent between machines.)

Found by these tests and fixed with them: `topk_rows_kernel` let an element at -inf beat the empty candidate on the index, so a
row with fewer than k finite values repeated the index of its first -inf element in the tail (0, 0, 0, ...) instead of the
documented -inf / -1 (test_topk_rows_branches, row 2 of every N)."""
import numpy as np
import pytest
import torch

import branch_cases as bc

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
F8 = torch.float8_e4m3fn


def _k():
    from vidil_amd import kernels
    return kernels


def _bits(t):
    """Integer view of a 16-bit / 32-bit float tensor: equality of these is bit equality (-0 != +0, NaN payloads count)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


# ============================================================================================ A. beam candidate selection
@pytest.mark.parametrize("V", bc.BEAM_V)
def test_logsoftmax_topk_branches(V):
    """`logsoftmax_topk`, plain and with the repetition penalty, for nb in 1..4, beams_in_logits in {1, nb}, ban in {-1, the second
    best logit of image 0's first row}, B = 5; the penalty form with cur_len in {64, 1} and penalties 0.6 and 1.3 over histories
    that hold -1, V, the banned token and repeats.  Left out: (V, nb, beams_in_logits) = (8, 4, 1) alone — 8 candidates, fewer
    than 2 nb + 1.  Indices equal the reference's (f32 log-softmax + beam score, score descending, flat index ascending) exactly;
    scores are within 4x the error of torch's own f32 `log_softmax + beam score` against fp64 on the same case.

    MI355X, 70 launches per V (60 at V = 8): torch f32 vs fp64 per case 3.4e-07 .. 3.2e-06; the kernel's worst |error| over the
    launches of a V, in units of its case's yardstick: 0.42 (1028), 0.49 (1500), 0.42 (2044), 0.28 (9220), 0.24 (9716),
    0.33 (10236), 1.26 (8), 0.43 (260), 0.36 (1000), 0.38 (1023), 0.26 (30521)."""
    k = _k()
    B = bc.BEAM_B
    worst_ratio, yards, n = 0.0, [], 0
    dev = {}
    for key in bc.beam_case_keys():
        if key[0] != V:
            continue
        c = bc.beam_case(*key)
        nb, nbl = c["nb"], c["nbl"]
        if nbl not in dev:
            dev[nbl] = c["logits"].to(DEV)
        kw = {}
        if c["hist"] is not None:
            kw = dict(seqs=c["hist"].to(DEV), cur_len=c["cur_len"], penalty=c["penalty"])
        s, i = k.logsoftmax_topk(dev[nbl], c["beam_scores"].to(DEV), B, nb, c["ban"], beams_in_logits=nbl, **kw)
        s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64)
        assert np.array_equal(i, c["order"][:, :2 * nb]), (key, i, c["order"])
        err = np.abs(s - np.take_along_axis(c["full64"], i, 1)).max()
        worst_ratio = max(worst_ratio, err / c["yardstick"])
        yards.append(c["yardstick"])
        n += 1
        assert err <= 4.0 * c["yardstick"], (key, err, c["yardstick"])
    print(f"\nlogsoftmax_topk V={V}: {n} launches; torch f32 vs fp64 per case {min(yards):.3e} .. {max(yards):.3e}; "
          f"kernel worst |error| / that = {worst_ratio:.2f} (allowed 4)")


# ========================================================================================================== B. topk_rows
@pytest.mark.parametrize("N", bc.TOPK_N)
def test_topk_rows_branches(N):
    """k in {1, min(N, 128)}, three rows with planted ties (inside one thread's stride, across the four waves) and one row with
    fewer than k finite values; values and indices bit-equal to a numpy lexsort (value descending, index ascending), -inf / -1
    in the places no finite value fills.  N = 257 also with row_stride = 264.

    Before the fix in topk.hip the short row failed at every N: the tail repeated the row's first -inf index instead of -1."""
    k = _k()
    x = bc.topk_input(N)
    xd = torch.from_numpy(x).to(DEV)
    for kk in sorted({1, min(N, 128)}):
        rv, ri = bc.topk_ref(x, kk)
        v, i = k.topk_rows(xd, kk)
        assert np.array_equal(v.cpu().numpy().view(np.int32), rv.view(np.int32)), (N, kk)
        assert np.array_equal(i.cpu().numpy(), ri), (N, kk)
        if N == bc.TOPK_STRIDED_N:
            wide = torch.full((bc.TOPK_ROWS, N + 7), 99.0, device=DEV)      # the columns past N would win if they were read
            wide[:, :N] = xd
            v2, i2 = k.topk_rows(wide[:, :N], kk)
            assert wide[:, :N].stride(0) == N + 7
            assert torch.equal(_bits(v2), _bits(v)) and torch.equal(i2, i)


def test_topk_rows_refuses_rows_beyond_the_lds_buffer():
    k = _k()
    x = torch.zeros(1, bc.TOPK_TOO_LONG, device=DEV)
    with pytest.raises(k.VidilHipError):
        k.topk_rows(x, 1)


# =============================================================================================================== C. rows
@pytest.mark.parametrize("D", bc.LN_D)
def test_layernorm_f32_output_vs_fp64_by_row_family(D):
    """M in {1, 5, 333} and every 5th row through x_stride, eps in {1e-6, 1e-12}: per row family the f32 output is within 4x the
    error of a plain numpy-f32 two-pass LayerNorm (largest over 8 column orders) against fp64; a constant row gives beta
    exactly.

    MI355X, families (3 randn + 0.5 | 100 + 0.05 randn | constant | spike | 1e-4 randn), worst over D:
      numpy-f32 vs fp64   1.3e-06 .. 4.1e-06 | 1.7e-03 .. 3.9e-03 | 0 | 5.1e-05 .. 7.6e-04 | 5.6e-08 .. 3.4e-06
      kernel worst        4.6e-07 .. 7.3e-07 | 2.3e-04 .. 3.2e-04 | 0 | 1.7e-06 .. 1.7e-05 | 5.6e-08 .. 1.1e-06
      kernel / yardstick  <= 0.38            | <= 0.14            | - | <= 0.04            | <= 1.00  (1.00 at eps = 1e-6, where
      both are the rounding of an output of ~1e-1 magnitude)."""
    k = _k()
    x, g, b = bc.ln_input(D)
    xd, gd, bd = (torch.from_numpy(a).to(DEV) for a in (x, g, b))
    fam_of = np.array([bc.ln_family(m) for m in range(x.shape[0])])
    for eps in bc.LN_EPS:
        ref, yard = bc.ln_reference(D, eps)
        worst = np.zeros(len(bc.LN_FAMILIES))

        def check(got, rows):
            got = got.cpu().numpy()
            err = np.abs(got.astype(np.float64) - ref[rows]).max(1)
            for f in range(len(bc.LN_FAMILIES)):
                sel = fam_of[rows] == f
                if sel.any():
                    worst[f] = max(worst[f], err[sel].max())
            const = fam_of[rows] == 2
            assert np.array_equal(got[const].view(np.int32), np.ascontiguousarray(np.broadcast_to(b, got[const].shape)).view(np.int32)), (D, eps)

        for M in bc.LN_M:
            if M == 1:
                for r in range(5):                                  # one launch per family
                    o = torch.full((1, D), float("nan"), device=DEV)
                    k.layernorm(xd[r:r + 1].contiguous(), gd, bd, eps, out32=o)
                    check(o, np.array([r]))
            else:
                o = torch.full((M, D), float("nan"), device=DEV)
                k.layernorm(xd[:M].contiguous(), gd, bd, eps, out32=o)
                check(o, np.arange(M))
        Ms = max(bc.LN_M) // 5
        o = torch.full((Ms, D), float("nan"), device=DEV)
        k.layernorm(xd, gd, bd, eps, M=Ms, D=D, x_stride=5 * D, out32=o)
        check(o, np.arange(Ms) * 5)
        ratio = np.divide(worst, yard, out=np.zeros_like(worst), where=yard > 0)
        print(f"\nlayernorm D={D} eps={eps:g}: numpy-f32 two-pass vs fp64 per family {np.array2string(yard, precision=2)}; "
              f"kernel worst |error| {np.array2string(worst, precision=2)}; ratio {np.array2string(ratio, precision=2)} (allowed 4)")
        assert (worst <= 4.0 * yard).all(), (D, eps, worst, yard)


@pytest.mark.parametrize("D", bc.LN_D)
def test_layernorm_16bit_split3_and_fp8_outputs_are_roundings_of_the_f32_output(D):
    """Outputs written in the same launch as out32: f16 / bf16 rows are torch's rounding of that out32 bit for bit; split3 rows
    are [hi | lo | hi] of it (planes = 3) and leave a poisoned third plane untouched (planes = 2); fp8 rows are within one e4m3
    step of it everywhere and torch's conversion of it on at least 99.9 % of the elements.

    MI355X: fp8 rows equal torch's conversion on 100.000 % of the elements at every D and eps; worst |error| 0.500 e4m3 steps."""
    k = _k()
    x, g, b = bc.ln_input(D)
    M = 35
    xd, gd, bd = (torch.from_numpy(a).to(DEV) for a in (x[:M], g, b))
    for eps in bc.LN_EPS:
        for dtype in DTYPES:
            o32 = torch.full((M, D), float("nan"), device=DEV)
            o16 = torch.full((M, D), float("nan"), dtype=dtype, device=DEV)
            k.layernorm(xd, gd, bd, eps, out16=o16, out32=o32)
            assert _same_bits(o16, o32.cpu().to(dtype)), (D, eps, dtype)
            o3 = torch.full((M, 3 * D), float("nan"), dtype=dtype, device=DEV)
            k.layernorm(xd, gd, bd, eps, out16=o3, out32=o32, split3=True)
            assert _same_bits(o3, bc.split3_ref(o32.cpu(), dtype)), (D, eps, dtype)
            poison = torch.full((M, 3 * D), float("nan"), dtype=dtype, device=DEV)
            _bits(poison).fill_(0x7E5A)                             # (a NaN in f16, 4.5e37 in bf16: nothing a LayerNorm writes)
            k.layernorm(xd, gd, bd, eps, out16=poison, out32=o32, split3=True, planes=2)
            assert _same_bits(poison[:, :2 * D], bc.split3_ref(o32.cpu(), dtype)[:, :2 * D]), (D, eps, dtype)
            assert bool((_bits(poison[:, 2 * D:]) == 0x7E5A).all()), (D, eps, dtype)
        o32 = torch.full((M, D), float("nan"), device=DEV)
        o8 = torch.zeros((M, D), dtype=F8, device=DEV)
        k.layernorm(xd, gd, bd, eps, out16=o8, out32=o32)
        y = o32.cpu()
        got = o8.cpu().float()
        step = torch.from_numpy(bc.ulp(y.double().clamp(-448, 448).numpy(), F8))
        d = (got.double() - y.double().clamp(-448, 448)).abs()
        same = (got == y.to(F8).float()).float().mean().item()
        print(f"\nlayernorm fp8 D={D} eps={eps:g}: equal to torch's conversion on {same * 100:.3f} % (>= 99.9 %), "
              f"worst |error| / e4m3 step = {(d / step).max().item():.3f} (allowed 1)")
        assert bool((d <= step).all()) and same >= 0.999, (D, eps, same)


@pytest.mark.parametrize("D", [768, 1280])
def test_layernorm_in_place_equals_out_of_place(D):
    """`clip.py` and `med.py` pass out32 = x; the kernel declares both `__restrict__` and loads non-temporally."""
    k = _k()
    x, g, b = bc.ln_input(D)
    xd, gd, bd = (torch.from_numpy(a).to(DEV) for a in (x, g, b))
    for eps in bc.LN_EPS:
        out = torch.full_like(xd, float("nan"))
        k.layernorm(xd, gd, bd, eps, out32=out)
        inplace = xd.clone()
        o16 = torch.full(xd.shape, float("nan"), dtype=torch.float16, device=DEV)
        k.layernorm(inplace, gd, bd, eps, out32=inplace, out16=o16)
        assert _same_bits(inplace, out), (D, eps)
        assert _same_bits(o16, out.cpu().half()), (D, eps)


def test_layernorm_refuses_an_unsupported_width_and_writes_nothing():
    k = _k()
    D = 640
    x = torch.ones(5, D, device=DEV)
    g, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    o32 = torch.full((5, D), -7.0, device=DEV)
    o16 = torch.full((5, D), -7.0, dtype=torch.float16, device=DEV)
    with pytest.raises(k.VidilHipError):
        k.layernorm(x, g, b, 1e-6, out16=o16, out32=o32)
    torch.cuda.synchronize()
    assert bool((o32 == -7.0).all()) and bool((o16 == -7.0).all())


def _join_tolerance(ref64, dtype):
    """|hi + lo - ref| allowed for split3 rows of the u8 entry: the f32 evaluation of x * scale + shift (scale = 1 / (255 std),
    two roundings; the product; shift = -mean / std, two roundings; the sum: at most (3 * 3.83 + 1.8 + 2.7) * 2^-24 < 1e-6 for
    the CLIP constants) plus half a unit of the output type at |lo| <= one unit at |ref|."""
    return 1e-6 + 0.5 * bc.ulp(bc.ulp(ref64, dtype), dtype)


@pytest.mark.parametrize("ps,S", bc.PATCH_GEOMETRIES)
def test_patchify_geometries_plain_and_split3(ps, S):
    """B = 2, f16 and bf16.  f32 entry: a pure cast, bit-equal to the rearranged `img.to(T)` (split3: [hi | lo | hi] of the
    rearranged f32 image).  u8 entry: within one unit in the last place of T around the fp64 value of (x / 255 - mean) / std.
    Pad columns (ps = 14) are exactly +0 in every plane.

    MI355X, the same at every geometry: u8 entry worst |error| 0.520 (f16) / 0.499 (bf16) units of the output type (allowed 1);
    hi + lo of the split3 rows 0.35 / 0.25 of the allowance of `_join_tolerance`."""
    k = _k()
    img, u8 = bc.patch_images(ps, S, bc.PATCH_B)
    imgd, u8d = img.to(DEV), u8.to(DEV)
    ldk, used = bc.patch_ldk(ps), 3 * ps * ps
    table = torch.from_numpy(bc.patch_u8_table())
    ref64 = bc.patch_u8_lookup(u8, table, ps).numpy()
    worst = {}
    for dtype in DTYPES:
        # ---- f32 entry
        out = k.patchify_f32(imgd, ps, dtype=dtype)
        assert _same_bits(out, bc.patch_rows(img.to(dtype), ps)[:, :out.shape[1]]), (ps, S, dtype)
        out3 = k.patchify_f32(imgd, ps, dtype=dtype, split3=True)
        assert out3.shape[1] == 3 * ldk
        want3 = bc.split3_ref(bc.patch_rows(img, ps), dtype)
        assert _same_bits(out3, want3), (ps, S, dtype)
        for plane in range(3):
            assert bool((_bits(out3[:, plane * ldk + used:(plane + 1) * ldk]) == 0).all())
        # ---- u8 entry
        lo, hi = bc.patch_u8_bounds(dtype)
        lo_rows, hi_rows = bc.patch_u8_lookup(u8, lo, ps), bc.patch_u8_lookup(u8, hi, ps)
        o8 = k.patchify_u8(u8d, ps, bc.CLIP_MEAN, bc.CLIP_STD, dtype=dtype)
        assert o8.shape[1] == ldk
        got = o8.cpu().float()
        assert bool(((got >= lo_rows) & (got <= hi_rows)).all()), (ps, S, dtype)
        assert bool((_bits(o8[:, used:]) == 0).all())
        o83 = k.patchify_u8(u8d, ps, bc.CLIP_MEAN, bc.CLIP_STD, dtype=dtype, split3=True)
        assert o83.shape[1] == 3 * ldk
        assert _same_bits(o83[:, :ldk], o8) and _same_bits(o83[:, 2 * ldk:], o8), (ps, S, dtype)   # hi planes: the plain rows
        assert bool((_bits(o83[:, ldk + used:2 * ldk]) == 0).all())
        join = o83[:, :ldk].cpu().double().numpy() + o83[:, ldk:2 * ldk].cpu().double().numpy()
        assert (np.abs(join - ref64) <= _join_tolerance(ref64, dtype)).all(), (ps, S, dtype)
        worst[str(dtype)] = (float((np.abs(got.double().numpy() - ref64) / bc.ulp(ref64, dtype)).max()),
                             float((np.abs(join - ref64) / _join_tolerance(ref64, dtype)).max()))
    print(f"\npatchify_u8 ps={ps} S={S}: worst |error| in units of the output type / of the hi + lo allowance: {worst}")


@pytest.mark.parametrize("kernel", ["f32", "u8", "any"])
def test_patchify_grid_stride_second_pass(kernel):
    """The smallest batch of each kernel whose work items exceed 4,096 blocks x 256 threads (counts in tests/branch_cases.py:
    1,053,696 / 1,053,696 / 1,146,880 against 1,048,576): every row, those of the second pass included, is right."""
    k = _k()
    ps, S, B = bc.PATCH_BIG[kernel]
    img, u8 = bc.patch_images(ps, S, B)
    if kernel in ("f32", "any"):
        split3 = kernel == "any"                                    # patchify_any_kernel<T, false>, split3 form
        out = k.patchify_f32(img.to(DEV), ps, dtype=torch.float16, split3=split3)
        rows = bc.patch_rows(img, ps)
        want = bc.split3_ref(rows, torch.float16) if split3 else rows.half()
        assert _same_bits(out, want)
    if kernel in ("u8", "any"):
        dtype = torch.float16 if kernel == "u8" else torch.bfloat16    # patchify_any_kernel<T, true>, plain form
        lo, hi = bc.patch_u8_bounds(dtype)
        o8 = k.patchify_u8(u8.to(DEV), ps, bc.CLIP_MEAN, bc.CLIP_STD, dtype=dtype).cpu().float()
        assert bool(((o8 >= bc.patch_u8_lookup(u8, lo, ps)) & (o8 <= bc.patch_u8_lookup(u8, hi, ps))).all())
        assert bool((o8[:, 3 * ps * ps:] == 0).all())


@pytest.mark.parametrize("M,D", [(bc.SPLIT3_M, D) for D in bc.SPLIT3_D] + [bc.SPLIT3_BIG])
def test_split3_rows_bit_equal(M, D):
    """[hi | lo | hi] bit-equal to the torch restatement, f16 and bf16; 1366 x 3072 is 1,049,088 float4s: a second grid-stride pass."""
    k = _k()
    x = bc.split3_input(M, D)
    for dtype in DTYPES:
        out = k.split3(x.to(DEV), torch.full((M, 3 * D), float("nan"), dtype=dtype, device=DEV))
        assert _same_bits(out, bc.split3_ref(x, dtype)), (M, D, dtype)


@pytest.mark.parametrize("D", bc.EMBED_D)
def test_embed_tokens_clamps_ids_and_reaches_the_last_position_row(D):
    k = _k()
    for M, T, ids in bc.EMBED_CASES:
        ids_t, word, pos, pos_off, want = bc.embed_case(D, M, T, ids)
        out = torch.full((M, D), float("nan"), device=DEV)
        k.embed_tokens(ids_t.to(DEV), word.to(DEV), pos.to(DEV), out, T=T, pos_off=pos_off)
        assert _same_bits(out, want), (D, M, T)


@pytest.mark.parametrize("D", bc.L2_D)
def test_l2_normalize_rows_vs_fp64(D):
    """Within 4x the error of numpy-f32 `x / ||x||` against fp64 on the same rows.

    MI355X: numpy f32 vs fp64 4.6e-09 .. 1.8e-08; kernel 0.85x .. 1.00x of it, 1.77x at D = 768, n = 9."""
    k = _k()
    for n in bc.L2_N:
        x, ref, yard = bc.l2_case(D, n)
        got = k.l2_normalize_rows(x.to(DEV).clone()).cpu().double().numpy()
        err = np.abs(got - ref).max()
        print(f"\nl2_normalize_rows D={D} n={n}: numpy f32 vs fp64 {yard:.3e}; kernel worst |error| {err:.3e} = {err / yard:.2f}x (allowed 4x)")
        assert err <= 4.0 * yard, (D, n, err, yard)


# ============================================================================================================= D. resize
def test_resize_wide_frame_takes_the_generic_horizontal_kernel():
    """blip_frames of 8 x 3840 frames to 224 x 224: the tiled horizontal kernel would need 111,488 B of LDS (> 64 KB, asserted
    from the formula of `vidil_resample_u8`), so `resample_h_kernel` runs.  Bit-exact against oracle/resize_ref.py."""
    from oracle import resize_ref
    from vidil_amd import preprocess

    H, W, S = bc.RESIZE_H_GENERIC
    ksize, _, _ = preprocess.axis_weights(W, S)
    assert bc.resample_h_lds_bytes(W, S, ksize) > 64 * 1024
    f = bc.resize_frames(3, H, W)
    got = preprocess.blip_frames(torch.from_numpy(f).to(DEV), S).cpu().numpy()
    want = np.stack([resize_ref.blip_process_frame_u8(x, S) for x in f])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("H,W", bc.RESIZE_ODD_FRAMES)
def test_resize_to_an_odd_size_takes_the_bytewise_vertical_kernel(H, W):
    """S = 225: rows of 675 bytes are no multiple of 4, so `resample_v_kernel` runs (blip_frames and clip_frames)."""
    from oracle import resize_ref
    from vidil_amd import preprocess

    S = bc.RESIZE_ODD_S
    assert (S * 3) % 4 != 0
    f = bc.resize_frames(3, H, W)
    fd = torch.from_numpy(f).to(DEV)
    got = preprocess.blip_frames(fd, S).cpu().numpy()
    assert np.array_equal(got, np.stack([resize_ref.blip_process_frame_u8(x, S) for x in f]))
    got = preprocess.clip_frames(fd, S).cpu().numpy()
    assert np.array_equal(got, np.stack([resize_ref.clip_process_frame_u8(x, S) for x in f]))


@pytest.mark.parametrize("kind", ["h", "v", "v4"])
def test_resample_grid_stride_second_pass(kind):
    """`resample_u8` directly, tables from `preprocess.axis_weights`, more than 16,384 x 256 output bytes (v4: words), so the
    grid-stride loop of resample_h_kernel / resample_v_kernel / resample_v4_kernel makes a second, partial pass.  Bit-exact
    against clip8((2^21 + sum p * k) >> 22) in numpy int64."""
    k = _k()
    src, bounds, coeffs, vertical, want = bc.resize_stride_case(kind)
    assert bc.resample_items(kind) > bc.RESAMPLE_CAP_ITEMS
    dst = torch.full(want.shape, 7, dtype=torch.uint8, device=DEV)
    k.resample_u8(torch.from_numpy(src).to(DEV), dst, torch.from_numpy(bounds).to(DEV), torch.from_numpy(coeffs).to(DEV),
                  vertical=vertical)
    assert np.array_equal(dst.cpu().numpy(), want)


# ===================================================================================================== E. beam_attention
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", bc.ATTN_H)
@pytest.mark.parametrize("n_keys", bc.ATTN_NKEYS)
def test_beam_attention_key_count_boundaries(n_keys, H, dtype):
    """rows = 5; unused arena cells are NaN.  Against fp64 softmax attention of the 16-bit inputs: |error| <= one unit in the last
    place of the output type at |ref| + 4x the error of the same computation in torch f32.

    MI355X: torch f32 vs fp64 1.8e-07 .. 5.6e-07; kernel worst |error| / (ulp + 4x that) 0.493 .. 0.500 over the 20 cases (the
    rounding of the result to the output type, half a unit, is all of it)."""
    k = _k()
    q, ka, va, anc, ref, f32_err = bc.attn_case(n_keys, H, dtype)
    out = torch.full((bc.ATTN_ROWS, H * 64), float("nan"), dtype=dtype, device=DEV)
    k.beam_attention(q.to(DEV), ka.to(DEV), va.to(DEV), anc.to(DEV), out, rows=bc.ATTN_ROWS, H=H, n_keys=n_keys)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    allowed = bc.ulp(ref, dtype) + 4.0 * f32_err
    ratio = (np.abs(got - ref) / allowed).max()
    print(f"\nbeam_attention n_keys={n_keys} H={H} {dtype}: torch f32 vs fp64 {f32_err:.3e}; kernel worst |error| / (ulp + 4 x that) = {ratio:.3f}")
    assert ratio <= 1.0, (n_keys, H, dtype, ratio)


def test_beam_attention_refuses_more_than_64_keys():
    k = _k()
    q, ka, va, anc, _, _ = bc.attn_case(64, 2, torch.float16)
    out = torch.full((bc.ATTN_ROWS, 128), -7.0, dtype=torch.float16, device=DEV)
    with pytest.raises(k.VidilHipError):
        k.beam_attention(q.to(DEV), ka.to(DEV), va.to(DEV), anc.to(DEV), out, rows=bc.ATTN_ROWS, H=2, n_keys=65)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
