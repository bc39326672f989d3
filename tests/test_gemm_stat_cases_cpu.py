"""The preconditions of tests/test_gemm_stat_forms_gpu.py, asserted without a GPU: the table reaches every instantiation of the
256-row launchers that the features can reach (and names what it cannot); every part count and row boundary is present; the
exact tier's inputs really are exact in f32 in two summation orders; an f32 emulation of the kernels' chain stays within half
the derived bound; and the checker reports each way the kernels could be wrong — built as a wrong EXPECTED array, never as a
kernel run."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_cases as gc
import gemm_stat_cases as sc
from gemm_cases import ACT_GELU_ERF, ACT_NONE, ACT_QUICK_GELU, C3_128, EPI_ARENA, EPI_F16, EPI_F32, EPI_HEADS, EPI_PATCH, G256, GUARD, W4
from gemm_stat_cases import EPI_F8

IDS = [c.name for c in sc.CASES]
ACTS = (ACT_NONE, ACT_GELU_ERF, ACT_QUICK_GELU)
OF = {f: [c for c in sc.CASES if c.feature == f] for f in sc.FEATURES}


def struct_of(c):
    """vidil_gemm_args of a case with placeholder pointers: enough for check_args and vidil_gemm_kernel_name, which launch nothing."""
    from vidil_amd import _lib

    p = 4096
    g = _lib.GemmArgs()
    g.A, g.W, g.bias = p, p, (p if c.bias else None)
    g.M, g.N, g.K, g.lda, g.epi, g.act, g.split_k = c.M, c.N, c.K, c.lda, c.epi, c.act, c.split_k
    g.dtype = _lib.DT_FP8 if c.fp8 else (_lib.DT_BF16 if c.dtype == "bf16" else _lib.DT_F16)
    g.dtype16 = _lib.DT_BF16 if c.dtype == "bf16" else _lib.DT_F16
    if c.fp8:
        g.w_scale = p
    if c.epi in (EPI_F16, EPI_F32, EPI_F8, EPI_PATCH):
        g.out, g.ldo = p, c.ldo
        if c.resid != "none":
            g.resid = p
        if c.epi == EPI_PATCH:
            g.pos, g.tpi = p, c.tpi
    else:
        g.q, g.k, g.vt = p, p, p
        g.T, g.H, g.part0, g.t_off, g.Tq_cap, g.Tk_cap, g.NP = c.T, c.H, c.part0, c.t_off, c.Tq_cap, c.Tk_cap, c.NP
        g.q_scale, g.kv_tiled, g.arena_rows, g.slot_stride = c.q_scale, int(c.tiled), c.arena_rows, c.slot_stride
    if c.fold:
        g.ln_fold, g.ln_colsum, g.ln_stats, g.ln_eps = 1, p, p, c.eps
    if c.out16:
        g.out16, g.ldo16, g.out16_split3 = p, c.ldo16, c.split3
    if c.stats:
        g.ln_stats_out = p
    if c.rln:
        g.rln_gamma, g.rln_beta, g.ln_stats, g.ln_eps = p, p, p, c.eps
    return g


# ------------------------------------------------------------------------------------------------ the dispatcher, restated
def test_every_case_runs_on_the_bodies_it_names_and_the_library_names_the_same_kernel(monkeypatch):
    """`expected_kernel` against the library's own answer for the same struct (vidil_gemm_kernel_name launches nothing)."""
    from vidil_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)
    for c in sc.CASES:
        assert c.bodies and set(c.bodies) <= {G256, W4, C3_128}, c.name
        for body in c.bodies:
            cb = sc.with_body(c, body)
            assert gc.form_of(sc.expected_kernel(cb)) == body, (c.name, body, sc.expected_kernel(cb))
            for key in gc.ENV_KEYS:
                monkeypatch.delenv(key, raising=False)
            for key, val in cb.env.items():
                monkeypatch.setenv(key, val)
            g = struct_of(cb)
            assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0, (c.name, lib.vidil_last_error())
            assert buf.value.decode() == sc.expected_kernel(cb), (c.name, body)
        # both bodies wherever both are built: the 8-wave kernel alone for HEADS with T < 8 and for the two -1000 answers of launch4w_fp8
        if c.split_k:
            assert c.bodies == (C3_128,) and sc.c3_serves(c), c.name
        elif (c.epi == EPI_HEADS and c.T < 8) or sc.not_built_4w(c):
            assert c.bodies == (G256,), c.name
        else:
            assert c.bodies == (G256, W4), c.name


def test_the_kernel_name_restates_the_two_fall_backs_of_the_fp8_4_wave_launcher(monkeypatch):
    """fp8 f32 rows with an activation and fp8 patch rows: launch4w_fp8 answers -1000 and vidil_gemm256_launch runs gemm256_kernel,
    also with VIDIL_GEMM4W=1 — and the name query says gemm256_kernel then (it used to name the 4-wave kernel)."""
    from vidil_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)
    monkeypatch.setenv("VIDIL_GEMM4W", "1")
    seen = 0
    for c in sc.CASES:
        if sc.not_built_4w(c):
            g = struct_of(c)
            assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0
            forced = sc.SCase(**{**{f: getattr(c, f) for f in c.__dataclass_fields__}, "env": {"VIDIL_GEMM4W": "1"}})
            assert buf.value.decode() == sc.expected_kernel(forced) and buf.value.startswith(b"gemm256_kernel<fp8"), c.name
            seen += 1
    assert seen >= 8


def reachable():
    """Every (fold, stats, rln, epilogue, activation, body, 16-bit type, fp8) that launch256_dispatch, launch256_fp8,
    launch4w_dispatch, launch4w_fp8 and launch4w_c3_tm<., 2> instantiate AND a call with one of this table's features can reach."""
    r = set()
    for dt in ("f16", "bf16"):
        for body in (G256, W4):
            for act in ACTS:
                r.add((True, False, False, EPI_F16, act, body, dt, False))             # ln_fold: f16 rows x activation
                r.add((False, False, False, EPI_F32, act, body, dt, False))            # out16 / out16_split3 on the plain f32 rows
                r.add((False, False, False, EPI_F8, act, body, dt, True))              # fp8 hand-over
            for epi in (EPI_HEADS, EPI_ARENA):
                r.add((True, False, False, epi, 0, body, dt, False))                   # ln_fold: scatter epilogues
            r.add((False, True, False, EPI_F32, 0, body, dt, False))                   # producer
            r.add((False, True, True, EPI_F32, 0, body, dt, False))                    # residual LayerNorm
            r.add((False, False, False, EPI_F32, 0, body, dt, True))                   # fp8 -> f32 rows
            r.add((False, False, False, EPI_HEADS, 0, body, dt, True))                 # fp8 -> per-head scatter
        for act in ACTS[1:]:
            r.add((False, False, False, EPI_F32, act, G256, dt, True))                 # (gemm4w: -1000)
        r.add((False, False, False, EPI_PATCH, 0, G256, dt, True))                     # (gemm4w: -1000)
        for act in ACTS:
            r.add((False, False, False, EPI_F32, act, C3_128, dt, False))              # compensated producer of the planes
    return r


def test_every_reachable_instantiation_has_a_case_and_the_unreachable_ones_are_named():
    covered = {sc.instantiation(c, b) for c in sc.CASES for b in c.bodies}
    want = reachable()
    assert want <= covered, sorted(want - covered)
    assert covered <= want, sorted(covered - want)
    # the refusals behind UNREACHABLE, asked of the library itself
    from vidil_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(128)

    def refused(c, needle, **fields):
        g = struct_of(c)
        for k, v in fields.items():
            setattr(g, k, v)
        assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) != 0, (c.name, fields)
        assert needle in lib.vidil_last_error(), lib.vidil_last_error()

    fold = sc.BY_NAME["fold_f16_K128_none_M1_N8_f16"]
    prod = next(c for c in OF["prod"] if c.stats)
    rln = OF["rln"][0]
    fp8 = next(c for c in OF["fp8"] if c.epi == EPI_F32 and c.act == ACT_NONE)
    refused(fold, b"only EPI_F16 / EPI_HEADS / EPI_ARENA", epi=EPI_F32)
    refused(prod, b"gemm/ln_stats_out", act=ACT_GELU_ERF)
    refused(rln, b"gemm/rln", ln_stats_out=None)
    refused(fp8, b"16-bit feature", out16=4096, ldo16=fp8.N)
    refused(fp8, b"not built for fp8", epi=EPI_F16)
    assert all(("VIDIL_REQUIRE" in v) or ("-1000" in v) or ("returns false" in v) or ("M above" in v) for v in sc.UNREACHABLE.values())
    # the compensated form does not take these features: a split_k launch with ln_fold is refused, with a producer it is K-tripled
    refused(fold, b"gemm/split_k", split_k=1, K=192, lda=192)
    g = struct_of(prod)
    g.split_k, g.K, g.lda = 1, 192, 192
    assert lib.vidil_gemm_split_k_serves(ctypes.byref(g)) == 0


def test_every_part_count_row_boundary_and_listed_edge_is_present():
    fold = OF["fold"]
    assert {c.K // 64 for c in fold} == {2, 3, 4, 5, 9, 12, 13, 16}
    for epi in (EPI_F16, EPI_HEADS, EPI_ARENA):
        mine = [c for c in fold if c.epi == epi]
        assert {"f16", "bf16"} <= {c.dtype for c in mine} and {True, False} <= {c.bias for c in mine}, epi
        assert {"exact", "bound"} <= {c.tier for c in mine}, epi
    f16 = [c for c in fold if c.epi == EPI_F16]
    for K in sc.FOLD_K:
        assert set(ACTS) <= {c.act for c in f16 if c.K == K}, K
    assert {8, 72, 264, 520} <= {c.N for c in f16} and {0, 8} <= {c.ldo_pad for c in f16}
    for K in (832, 128, 1024, 576):                 # every row boundary at 13, 2, 16 and 9 parts
        assert set(sc.M_SET) & {c.M for c in f16 if c.K == K and c.act == ACT_NONE} and len({c.M for c in f16 if c.K == K}) >= 4, K
    heads = [c for c in fold if c.epi == EPI_HEADS]
    assert {1, 7, 8, 9, 33} <= {c.T for c in heads}
    v = [c for c in heads if c.part0 + c.nparts == 3]
    assert any(c.NP and not c.tiled for c in v) and any(c.NP == 0 and not c.tiled for c in v) and any(c.tiled for c in v)
    assert all(c.bodies == ((G256,) if c.T < 8 else (G256, W4)) for c in heads)
    kv = [c for c in heads if c.part0 + c.nparts > 1]
    assert any(c.t_off > 0 for c in kv) and all(c.Tk_cap > c.t_off + c.T for c in kv) and all(c.Tq_cap > c.T for c in heads)
    arena = [c for c in fold if c.epi == EPI_ARENA]
    assert {(1, 1), (5, 3)} <= {(c.T, c.slot_stride) for c in arena} and all(c.arena_rows > (c.B - 1) * c.slot_stride + 1 for c in arena)
    for f in sc.FEATURES:
        assert set(sc.M_SET) <= {c.M for c in OF[f]}, f
        assert all(c.M <= 600 and c.N <= 1088 and c.K <= 3072 for c in OF[f]), f
    prod = OF["prod"]
    st = [c for c in prod if c.stats]
    assert {64, 192, 320, 1088} <= {c.N for c in st} and {128, 192, 1024} <= {c.K for c in st}
    assert {(0, 0), (0, 4), (4, 0), (4, 4)} <= {(c.ldo_pad, c.ldo16_pad) for c in st} and {"none", "alias", "own"} <= {c.resid for c in st}
    copy = [c for c in prod if not c.stats]
    assert copy and all(c.out16 for c in copy) and any(c.N % 64 for c in copy) and {"none", "alias", "own"} <= {c.resid for c in copy}
    rln = OF["rln"]
    assert {c.N for c in rln if c.tier == "exact"} == {64, 128, 256, 512, 1024} and {c.N for c in rln if c.tier == "bound"} == {192, 320, 768, 960}
    for N in sc.EXACT_WIDTHS + sc.RLN_BOUND_N:
        assert {"alias", "own"} <= {c.resid for c in rln if c.N == N}, N
    assert all(c.ldo == c.N and c.stats and c.out16 for c in rln)
    s3 = OF["split3"]
    for bodies in ((G256, W4), (C3_128,)):
        mine = [c for c in s3 if c.bodies == bodies]
        assert {(v, a, p) for v in (1, 2) for a in ACTS for p in (0, 4)} <= {(c.split3, c.act, c.ldo16_pad) for c in mine}, bodies
        assert all(c.ldo16 % 12 == 0 and c.ldo16 // 3 >= c.N for c in mine)
    assert all(c.split_k == 1 and c.K % 96 == 0 for c in s3 if c.bodies == (C3_128,))
    fp8 = OF["fp8"]
    assert {128, 384, 1024} <= {c.K for c in fp8} and {0, 16} <= {c.lda_pad for c in fp8}
    assert {EPI_F32, EPI_PATCH, EPI_HEADS, EPI_F8} == {c.epi for c in fp8}
    f8 = [c for c in fp8 if c.epi == EPI_F8]
    assert {(N, p, a) for N in (16, 80, 272) for p in (0, 16) for a in ACTS} <= {(c.N, c.ldo_pad, c.act) for c in f8}
    assert {"none", "alias", "own"} <= {c.resid for c in fp8 if c.epi == EPI_F32} and set(ACTS) <= {c.act for c in fp8 if c.epi == EPI_F32}
    hv = [c for c in fp8 if c.epi == EPI_HEADS and c.part0 + c.nparts == 3]
    assert any(c.NP and not c.tiled for c in hv) and any(c.NP == 0 and not c.tiled for c in hv) and any(c.tiled for c in hv)


# ------------------------------------------------------------------------------------------------ the exact tier is exact
def _f32_sum(x, axis_len, reverse):
    acc = np.zeros(x.shape[:-1], np.float32)
    for i in (range(axis_len - 1, -1, -1) if reverse else range(axis_len)):
        acc = acc + x[..., i].astype(np.float32)
    return acc


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_inputs_are_exact_in_their_types_and_the_exact_tier_is_exact_in_f32_in_two_orders(c):
    d = sc.inputs(c)
    dt = sc.F8 if c.fp8 else gc.T16[c.dtype]
    for k in ("A", "W"):
        x = torch.from_numpy(d[k])
        assert torch.equal(x.float().to(dt).double(), x), k
    for k in ("bias", "resid", "pos", "colsum", "stats_in", "gamma", "beta", "w_scale"):
        if d[k] is not None:
            assert np.array_equal(d[k].astype(np.float32).astype(np.float64), d[k]), k
    S = np.abs(d["A"]) @ np.abs(d["W"]).T
    assert S.max() < 2 ** 24                                         # every summation order of the product is exact
    V, dV = sc.source_values(c, d)
    P, dP = sc.pre_activation(c, d)
    if c.fp8:
        assert set(np.unique(np.log2(d["w_scale"]))) <= set(range(-3, 4)) and np.unique(d["w_scale"]).size >= 4
        assert (d["w_scale"][:-4] != d["w_scale"][4:]).any()
    if c.act != ACT_NONE:
        assert np.array_equal(P * 8, np.round(P * 8)) or c.tier == "bound"
        assert np.abs(P).max() <= 6.0 and np.unique(P).size >= min(20, P.size // 2), (np.abs(P).max(), np.unique(P).size)
    if c.tier == "exact":
        assert (dV == 0).all() and np.array_equal(P.astype(np.float32).astype(np.float64), P)
    if c.fold or c.rln:
        st = d["stats_in"]
        assert st.shape == (c.M, c.nstat, 2) and (st != 0).all()
        if c.nstat > 1:                                              # the parts of a row differ from each other
            for k in (0, 1):
                srt = np.sort(st[:, :, k], axis=1)
                assert (np.diff(srt, axis=1) != 0).all()
        ch = sc.stat_chain(st, c.width, c.eps)
        assert (ch["var"] > 0).all() and (c.tier == "exact" or (ch["dt"] < 1e-3 * ch["t"]).all())
        pairs = np.stack([ch["mean"], ch["rstd"]], axis=1)
        assert (np.abs(np.diff(pairs, axis=0)).sum(1) > 0).all()     # neighbouring rows never share their statistics
        for dist in (32, 128, 256):
            if c.M > dist:
                assert (np.abs(pairs[dist:] - pairs[:-dist]).sum(1) > 0).all(), dist
        if c.tier == "exact":
            assert c.width in sc.EXACT_WIDTHS and c.eps == 2.0 ** -6
            j = np.log2(ch["var"] + c.eps) / 2
            assert np.array_equal(j, np.round(j)) and np.array_equal(ch["rstd"], 2.0 ** -j)
            for order in (0, 1):                                     # the whole f32 chain, parts added front to back and back to front
                e = sc.emulate_f32(c, d, order).astype(np.float64)
                ref = P if c.fold else V
                assert np.array_equal(e, ref), (order, np.abs(e - ref).max())
            if np.unique(pairs, axis=0).shape[0] < c.M:              # fewer combinations than rows (rln, activations): still dozens
                assert np.unique(pairs, axis=0).shape[0] >= min(c.M, 18)
        else:
            assert (ch["mean"] ** 2 <= 4 * ch["var"]).all()
            e = sc.emulate_f32(c, d, 0).astype(np.float64)
            ref, bound = (P, dP) if c.fold else (V, dV)
            assert (np.abs(e - ref) <= 0.5 * bound).all(), float((np.abs(e - ref) / bound).max())
    if c.stats and c.tier == "exact":
        assert np.abs(V).max() <= 512
        p = V.reshape(c.M, c.N // 64, 64)
        for vals in (p, p * p):
            assert np.array_equal(vals.astype(np.float32).astype(np.float64), vals)
            a, b = _f32_sum(vals, 64, False), _f32_sum(vals, 64, True)
            assert np.array_equal(a, b) and np.array_equal(a.astype(np.float64), vals.sum(2))
    if c.split3 and c.act == ACT_NONE:
        hi = torch.from_numpy(V).float().to(gc.T16[c.dtype])
        lo = (torch.from_numpy(V).float() - hi.float()).to(gc.T16[c.dtype])
        assert torch.isfinite(hi.float()).all() and (lo.float() != 0).float().mean() > 0.25            # a low plane worth checking
        assert np.abs(V).max() > (5e4 if c.dtype == "f16" else 2 ** 8)
    # room in every direction for a store that escapes
    for dest, (vals, written, bound) in sc.expected(c, d).items():
        shape, kind = sc.dest_shapes(c)[dest]
        assert written.any() and written.mean() <= 0.93, (dest, written.mean())
        if dest in ("out", "out16", "stats"):
            w = written.reshape(shape)
            assert shape[0] > c.out_rows and not w[c.out_rows:].any()
        if c.exact and bound is None:
            assert np.isfinite(sc.values_of(c, kind, sc.bits_of(c, kind, vals))).all(), dest


def test_e4m3_reference_rounds_ties_to_even_and_saturates_and_the_cases_contain_both():
    """torch's e4m3 cast, against a hand-written table, before it is trusted as the reference of EPI_F8."""
    table = [(17.0, 16.0), (19.0, 20.0), (18.0, 18.0), (21.0, 20.0), (23.0, 24.0), (0.5625, 0.5625), (0.59375, 0.625), (0.53125, 0.5),
             (-17.0, -16.0), (-19.0, -20.0), (232.0, 224.0), (248.0, 256.0), (440.0, 448.0), (448.0, 448.0), (449.0, 448.0), (600.0, 448.0),
             (-1e4, -448.0), (2.0 ** -9, 2.0 ** -9), (2.0 ** -10, 0.0), (3 * 2.0 ** -10, 2.0 ** -8), (0.0, 0.0)]
    c = next(c for c in OF["fp8"] if c.epi == EPI_F8)
    for x, want in table:
        assert sc.values_of(c, "f8", sc.bits_of(c, "f8", np.array([x])))[0] == want, x
    ties = sat = 0
    for c in OF["fp8"]:
        if c.epi == EPI_F8 and c.act == ACT_NONE:
            V, _ = sc.source_values(c, sc.inputs(c))
            a = np.abs(V)
            ties += int(((a > 16) & (a < 32) & (a % 2 == 1)).sum())
            sat += int((a > 448).sum())
    assert ties > 100 and sat > 100, (ties, sat)


# ------------------------------------------------------------------------------------------------ the checker
def _good(c, dest, vals, written):
    shape, kind = sc.dest_shapes(c)[dest]
    it, sentinel = sc.int_type(kind)
    good = np.full(vals.size + 2 * GUARD, sentinel, dtype=it)
    good[GUARD:GUARD + vals.size][written] = sc.bits_of(c, kind, vals)[written]
    return good


WRONG = {  # feature -> the wrong variants that apply to it
    "fold": ("row+1", "row-1", "part_dropped", "part_doubled", "colsum_quad", "bias_quad"),
    "rln": ("row+1", "row-1", "part_dropped", "part_doubled", "gamma_quad", "beta_quad", "bias_quad"),
    "fp8": ("scale_quad", "bias_quad"),
    "prod": ("bias_quad",),
    "split3": ("bias_quad",),
}
PROBES = ["fold_f16_K1024_sweep_M129_f16", "fold_f16_K832_sweep_M257_bf16", "fold_f16_K192_none_M127_N72_f16",
          "fold_heads_K128_T9_H1_p0x3_tiled_M126_bf16", "fold_heads_K320_T9_H1_p0x3_vt_M261_f16", "fold_arena_K256_T1_s1_p0_M129_f16",
          "fold_f16_K576_gelu_M255_N72_bf16", "rln_N512_alias_M257_f16", "rln_N768_own_M300_bf16", "rln_N64_own_M31_bf16",
          "prod_N192_K128_M127_f16", "prod_copy_N260_M257_bf16", "split3_v2_none_ldo16+12_M257_N520_f16", "split3_c3_v1_none_ldo16+0_M31_N12_bf16",
          "fp8_f8_N80_ldo+16_none_M31_f16", "fp8_f32_K384_lda+0_M33_bf16", "fp8_heads_T9_H1_p0x3_vt_M261_f16"]


def test_the_probes_exist_and_span_the_features_and_tiers():
    cs = [sc.BY_NAME[n] for n in PROBES]
    assert {c.feature for c in cs} == set(sc.FEATURES) and {c.tier for c in cs} == {"exact", "bound"}
    assert any(c.act != ACT_NONE for c in cs) and any(c.split3 == 2 for c in cs) and any(c.split3 == 1 for c in cs)


@pytest.mark.parametrize("name", PROBES)
def test_the_verdict_accepts_the_reference_and_reports_every_wrong_variant(name):
    """`verdict` is what the GPU test asserts.  Fed the reference it is silent.  Each wrong variant — statistics of row m +- 1, one
    part dropped or doubled, a colsum / bias / scale / gamma / beta quad shifted by 4 columns — is built as the expected array of a
    kernel with that mistake and must be reported; in the bound tier it must move an affected element by at least 16 bounds.
    A store at column N, at row M, into plane 2 when out16_split3 == 2, into the padding between planes and into either guard is
    reported as a store outside the written region."""
    c = sc.BY_NAME[name]
    d = sc.inputs(c)
    exp = sc.expected(c, d)
    goods = {dest: _good(c, dest, vals, written) for dest, (vals, written, _) in exp.items()}
    for dest, (vals, written, bound) in exp.items():
        if bound is not None and not np.isfinite(bound[written]).all():
            continue                    # (derived from the launch's own rows on the GPU)
        assert sc.verdict(c, dest, goods[dest], vals, written, bound)[0] is None, dest
    for kind in WRONG[c.feature]:
        key = {"colsum": "colsum", "bias": "bias", "scale": "w_scale", "gamma": "gamma", "beta": "beta"}.get(kind.split("_")[0])
        if key is not None and d[key] is None:
            continue
        bad = sc.expected(c, sc.wrong_inputs(c, d, kind))
        reported = 0
        for dest, (vals, written, bound) in exp.items():
            if bound is not None and not np.isfinite(bound[written]).all():
                continue
            bvals = bad[dest][0]
            msg, worst = sc.verdict(c, dest, _good(c, dest, bvals, written), vals, written, bound)
            if msg is not None:
                reported += 1
                if bound is not None:
                    assert worst >= 16.0, (kind, dest, worst)
        assert reported, (name, kind)
    # stores that escape
    one = lambda k: sc.bits_of(c, k, np.ones(1))[0]
    for dest, (vals, written, bound) in exp.items():
        shape, k = sc.dest_shapes(c)[dest]
        w = written.reshape(shape)
        spots = {"guard in front": 0, "guard in front ": GUARD - 1, "guard behind": GUARD + vals.size, "guard behind ": goods[dest].size - 1}
        if dest in ("out", "out16", "stats"):
            spots["row M"] = GUARD + int(np.ravel_multi_index((c.out_rows,) + (0,) * (len(shape) - 1), shape))
        if dest == "out" and c.ldo > c.N:
            spots["column N"] = GUARD + c.N
        if dest == "out16":
            if c.split3 == 2:
                spots["plane 2"] = GUARD + 2 * c.plane
                assert not w[:, 2 * c.plane:].any()
            if c.ldo16_pad:
                spots["plane padding"] = GUARD + c.N
        for what, pos in spots.items():
            brk = goods[dest].copy()
            brk[pos] = one(k)
            msg = sc.verdict(c, dest, brk, vals, written, bound)[0]
            assert msg is not None and ("guard" in msg if "guard" in what else "outside the written region" in msg), (dest, what, msg)
    # a value one unit in the last place off, and a store that never happened, in the exact tier
    if c.exact:
        for dest, (vals, written, bound) in exp.items():
            pos = GUARD + int(np.flatnonzero(written)[-1])
            for v in (goods[dest][pos] ^ 1, sc.int_type(sc.dest_shapes(c)[dest][1])[1]):
                brk = goods[dest].copy()
                brk[pos] = v
                assert "differ from the exact result" in sc.verdict(c, dest, brk, vals, written, bound)[0], dest


def test_split3_without_out_expects_untouched_f32_rows():
    c = sc.BY_NAME["split3_v2_none_ldo16+12_M257_N520_f16"]
    exp = sc.expected(c, out_null=True)
    assert not exp["out"][1].any() and exp["out16"][1].any()
    good = _good(c, "out", *exp["out"][:2])
    assert sc.verdict(c, "out", good, *exp["out"])[0] is None
    good[GUARD + 5] = 0
    assert "outside the written region" in sc.verdict(c, "out", good, *exp["out"])[0]
