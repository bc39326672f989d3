"""The preconditions of tests/test_gemm_forms_gpu.py, asserted without a GPU: the table reaches every (kernel form, epilogue,
activation) the dispatcher can produce and every listed edge on every form it applies to; every expected value is exact in its
output type; no two source elements share a destination; every destination leaves room, in every direction, for a store that
escapes; the scatter maps agree with a second formulation."""
import numpy as np
import pytest
import torch

import gemm_cases as gc
from gemm_cases import (ACT_GELU_ERF, ACT_NONE, ACT_QUICK_GELU, C3_128, C3_256, EPI_ARENA, EPI_F16, EPI_F32, EPI_HEADS, EPI_PATCH, G256,
                        S64, S128_2, S128_3, S128x64, SMALL, W4, W4_128)

IDS = [c.name for c in gc.CASES]
MINE = {f: [c for c in gc.CASES if c.kernel == f] for f in gc.FORMS}


def _pair(c):
    return gc.form_of(gc.expected_kernel(c)), c.epi, c.act


def test_every_case_reaches_the_form_it_names():
    for c in gc.CASES:
        assert gc.form_of(gc.expected_kernel(c)) == c.kernel, (c.name, gc.expected_kernel(c))
        assert set(c.env) <= set(gc.ENV_KEYS)


def test_every_reachable_form_epilogue_activation_triple_has_a_case():
    """The reachable set comes from `expected_kernel` on a probe grid: every epilogue and activation x every switch setting x
    split_k x shapes on both sides of every threshold of the dispatcher (tile counts, K, N <= 1024, vector alignment)."""
    shapes = [(M, N) for M in (5, 300, 4900, 5300, 7300, 8500, 41000) for N in (64, 192, 576, 1001, 1088, 1152, 1288, 163912, 163968)]
    envs = [{}, {"VIDIL_GEMM4W": "0"}, {"VIDIL_GEMM4W": "1"}, {"VIDIL_GEMM4W128": "1"}, {"VIDIL_GEMM4W128": "0"}]
    reachable = set()
    for M, N in shapes:
        for K, split_k in ((64, 0), (128, 0), (192, 1), (1536, 0)):
            for epi in (EPI_F16, EPI_F32, EPI_HEADS, EPI_PATCH, EPI_ARENA):
                for act in ((ACT_NONE, ACT_GELU_ERF, ACT_QUICK_GELU) if epi in (EPI_F16, EPI_F32) else (ACT_NONE,)):
                    for T in (1, 20):
                        if epi in (EPI_HEADS, EPI_ARENA) and N % 64:
                            continue
                        for env in envs:
                            p = gc.Case(name="probe", kernel="", epi=epi, act=act, M=M, N=N, K=K, split_k=split_k, T=T, H=1, tpi=1, env=env)
                            reachable.add(_pair(p))
    assert {f for f, _, _ in reachable} == set(gc.FORMS)
    covered = {_pair(c) for c in gc.CASES}
    assert reachable <= covered, sorted(reachable - covered)
    assert covered <= reachable, sorted(covered - reachable)      # (and the probe grid finds every triple the table has)
    # routes, not only triples: every branch of choose_tile that returns a small tile is taken by a probe AND by a case
    def route(c):
        big, bm, bn, st = gc._choose_tile(c, 256)
        n128 = gc._cdiv(c.M, 128) * gc._cdiv(c.N, 128)
        return (bm, bn, st, n128 >= 200 and c.N <= 1024) if not big and not gc._c3_serves(c, 256) else None
    want = {(128, 128, 3, True), (128, 128, 2, True), (64, 64, 3, False), (128, 64, 2, False), (128, 128, 2, False)}
    probes = {route(gc.Case(name="probe", kernel="", M=M, N=N, K=64)) for M, N in shapes} - {None}
    assert probes == want, probes
    assert {route(c) for c in gc.CASES} - {None} == want


def test_every_listed_edge_is_present_on_every_form_it_applies_to():
    for f, mine in MINE.items():
        bm, bn = gc.TILE[f]
        plain = [c for c in mine if c.epi in (EPI_F16, EPI_F32)]
        assert {"f16", "bf16"} <= {c.dtype for c in mine}, f
        # rows: below one tile (not on <128,128,3>: 200 .. 256 tiles within N <= 1024 are at least 25 tile rows), M % BM = 1, 3, BM - 1
        if f != S128_3:
            assert {1, 5} <= {c.M for c in plain}, f
            assert {"f16", "bf16"} <= {c.dtype for c in plain if c.M in (1, 5)}, f
        if f == S128_2:                 # both routes of choose_tile into the kernel, a row tail on each
            for wide in (False, True):
                assert {1, 3, bm - 1} & {c.M % bm for c in plain if c.M > bm and (c.N > 1024) == wide}, (f, wide)
        assert {1, 3, bm - 1} <= {c.M % bm for c in plain if c.M > bm}, f
        # columns: 8 into a tile, 8 short of one, no multiple of 64; ldo > N
        assert {8, bn - 8} <= {c.N % bn for c in plain}, f
        assert any(c.N % 64 not in (0, 8, 56) for c in plain) and any(c.ldo_pad for c in plain), f
        # the plain rows: 16-bit without activation (not in the C3 form), f32 with resid aliasing out / its own / none, no bias
        if f not in (C3_256, C3_128):
            assert any(c.epi == EPI_F16 and c.act == ACT_NONE for c in plain), f
        f32 = [c for c in plain if c.epi == EPI_F32 and c.exact]
        assert {"alias", "own", "none"} <= {c.resid for c in f32} and any(not c.bias for c in f32), f
        assert sum(not c.exact for c in plain) >= 3, f
        if f in SMALL:
            assert any(c.N % 2 for c in plain) and any(c.ldo % 4 for c in plain if c.epi == EPI_F32), f
            assert any(c.ldo % 8 for c in plain if c.epi == EPI_F16), f
            assert {1, 2, 3, 5} <= {c.K // 64 for c in plain}, f
            assert {8, 64} <= {c.lda_pad for c in plain}, f
            assert 1 < gc.RING[f] <= 3                       # K / 64 = 1: fewer tiles than either ring's prologue
        else:
            assert any(c.lda_pad for c in plain), f
        tiles = {gc._cdiv(c.M, bm) * gc._cdiv(c.N, 256) for c in plain}
        if f in (W4_128, C3_128):
            assert {1, 9} <= tiles and any(t > 256 and t % 8 for t in tiles), f
        if f in (G256, W4, C3_256):
            assert any(t > 256 and t % 8 for t in tiles) and any(t < 256 and t % 8 for t in tiles), f
        if f == C3_256:                 # (the patch epilogue alone brings 256-row tiles to small grids)
            ptiles = {gc._cdiv(c.M, 256) * gc._cdiv(c.N, 256) for c in mine if c.epi == EPI_PATCH}
            assert {1, 9} <= ptiles and any(t < 8 and t != 1 for t in ptiles), f
            assert any(c.M < 256 and c.M % c.tpi == 0 and c.B > 1 for c in mine if c.epi == EPI_PATCH), f
        # heads
        heads = [c for c in mine if c.epi == EPI_HEADS]
        want_T = {8, 9, 17, 33, 300} | (set() if f in (W4, W4_128, C3_256, C3_128) else {1, 7})
        assert want_T <= {c.T for c in heads}, f
        if f != S128x64:                                     # (N > 1024 there: 6 heads and more)
            assert {1, 3} <= {c.H for c in heads}, f
        assert {(0, 3), (0, 1), (1, 2)} <= {(c.part0, c.nparts) for c in heads}, f
        kv = [c for c in heads if c.part0 + c.nparts > 1]
        assert any(c.t_off > 0 and c.Tk_cap > c.t_off + c.T for c in kv) and all(c.Tq_cap > c.T for c in heads), f
        v = [c for c in heads if c.part0 + c.nparts == 3]
        assert any(c.NP and c.NP % 16 == 0 and c.NP > c.t_off + c.T and not c.tiled for c in v), f
        assert any(c.NP and c.t_off % 4 for c in v), f           # vt(t_off + t) shifted into the middle of a 4-key group
        assert any(c.NP == 0 and not c.tiled for c in v) and any(c.tiled and c.Tk_cap % 32 == 0 for c in v), f
        # arena
        arena = [c for c in mine if c.epi == EPI_ARENA]
        if f in (C3_256, C3_128):
            assert not arena
        else:
            assert {(1, 1), (5, 3)} <= {(c.T, c.slot_stride) for c in arena} and {0, 1} <= {c.part0 for c in arena}, f
            assert all(c.t_off > 0 and c.arena_rows > (c.B - 1) * c.slot_stride + 1 for c in arena), f
        # patch
        patch = [c for c in mine if c.epi == EPI_PATCH]
        if f in (W4_128, C3_128):
            assert not patch
        else:
            assert {1, 4, 49} <= {c.tpi for c in patch} and all(c.ldo_pad for c in patch), f
    c3 = MINE[C3_256] + MINE[C3_128]
    for f in (C3_256, C3_128):
        assert {64, 128} <= {c.K // 3 for c in MINE[f]}, f
        assert {8, 33} <= {c.T for c in MINE[f] if c.epi == EPI_HEADS}, f
    assert all(c.split_k == 1 and c.K % 96 == 0 for c in c3)


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_values_are_exact_destinations_are_distinct_and_every_view_leaves_room(c):
    d = gc.inputs(c)
    dt = gc.T16[c.dtype]
    # operands are exact in the operand type
    for k in ("A", "W"):
        x = torch.from_numpy(d[k])
        assert torch.equal(x.to(dt).double(), x), k
    assert gc.magnitude(c, d) < 2 ** 24
    if not c.exact:
        P = gc.pre_activation(c, d)
        assert np.array_equal(P * 8, np.round(P * 8)) and np.abs(P).max() <= 6.0 and np.unique(P).size >= 60
    exp = gc.expected(c, d)
    shapes = gc.dest_shapes(c)
    assert set(exp) == set(shapes)
    total = 0
    for name, (vals, written, count) in exp.items():
        shape, kind = shapes[name]
        total += int(written.sum())
        assert count.max() == 1, f"{name}: two source elements share a destination"
        if c.exact:                             # bit-exact in the output type: a round trip through it
            x = torch.from_numpy(vals)
            assert torch.equal(x.to(dt if kind == "t16" else torch.float32).double(), x), name
        assert written.mean() <= 0.9, (name, written.mean())
        w = written.reshape(shape)
        if name == "out" or (name == "q" and c.epi == EPI_ARENA):
            assert w[:c.out_rows].any(axis=1).all() or c.epi == EPI_PATCH
            assert shape[0] > c.out_rows and not w[c.out_rows:].any()              # rows behind M
            if name == "out":
                assert not w[:, c.N:].any() and w[:, :c.N].any(axis=0).all()       # columns behind N
            if c.epi == EPI_PATCH:
                cls = np.arange(c.B) * (c.tpi + 1)
                assert not w[cls].any() and w[:c.out_rows].any(axis=1).sum() == c.M
        elif c.epi == EPI_HEADS:
            if name == "q":
                assert w[:, :, :c.T].all() and c.Tq_cap > c.T and not w[:, :, c.T:].any()
            elif c.tiled:
                off = (gc.ktile_off, gc.vtile_off)[name == "vt"]
                rows = np.zeros(c.Tk_cap, dtype=bool)
                rows[c.t_off:c.t_off + c.T] = True
                for t in range(c.Tk_cap):       # token rows on both sides of t_off .. t_off + T stay untouched
                    at = w.reshape(c.B, c.H, -1)[:, :, [off(t, dd) for dd in range(64)]]
                    assert at.all() if rows[t] else not at.any(), (name, t)
                assert c.Tk_cap > c.t_off + c.T
            elif name == "vt" and c.NP:
                cols = sorted(gc.vt_col(c.t_off + t) for t in range(c.T))
                assert w[:, :, :, cols].all() and w.sum() == c.B * c.H * 64 * c.T and c.NP > c.t_off + c.T      # unused V^T columns
            else:
                assert w[:, :, c.t_off:c.t_off + c.T].all() and not w[:, :, :c.t_off].any() and not w[:, :, c.t_off + c.T:].any()
                assert c.Tk_cap > c.t_off + c.T
        else:                                   # the arenas [position][slot][H * 64]
            slots = np.arange(c.B) * c.slot_stride
            assert w[c.t_off:c.t_off + c.T][:, slots].all() and w.sum() == c.M * c.HD
            assert c.t_off > 0 and c.Tk_cap > c.t_off + c.T and c.arena_rows > slots[-1] + 1                  # spare positions and slots
    assert total == c.M * c.N


def test_nan_padding_surrounds_the_operands():
    c = gc.BY_NAME["s64_k2_lda+8"]
    A, W = gc.operand_tensors(c, gc.inputs(c))
    assert A.shape == (c.M + gc.NAN_ROWS, c.K + 8) and torch.isnan(A[:, c.K:]).all() and torch.isnan(A[c.M:]).all()
    assert torch.isnan(W[c.N:]).all() and torch.isfinite(A[:c.M, :c.K]).all() and torch.isfinite(W[:c.N]).all()
    for s in (gc.SENTINEL16, gc.SENTINEL32):
        kinds = ((torch.int16, torch.float16), (torch.int16, torch.bfloat16)) if s == gc.SENTINEL16 else ((torch.int32, torch.float32),)
        for it, ft in kinds:
            assert torch.isnan(torch.tensor([s], dtype=it).view(ft)).all()


# ------------------------------------------------------------------------------------------------ the maps, a second time
VT_ORDER = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)      # include/vidil_hip.h: keys of a 16-key block, in storage order

TINY = [
    gc.Case(name="tiny_heads_vt", kernel=S64, epi=EPI_HEADS, M=3 * 21, N=3 * 128, T=21, H=2, part0=0, t_off=13, Tq_cap=23, Tk_cap=40, NP=48),
    gc.Case(name="tiny_heads_tiled", kernel=S64, dtype="bf16", epi=EPI_HEADS, M=2 * 9, N=2 * 192, T=9, H=3, part0=1, t_off=28, Tk_cap=64,
            tiled=True),
    gc.Case(name="tiny_arena", kernel=S64, epi=EPI_ARENA, M=4 * 5, N=3 * 128, T=5, H=2, part0=0, t_off=3, Tk_cap=10, arena_rows=12,
            slot_stride=3),
    gc.Case(name="tiny_patch", kernel=S64, epi=EPI_PATCH, M=5 * 4, N=24, tpi=4, ldo_pad=8),
]


@pytest.mark.parametrize("c", TINY, ids=[c.name for c in TINY])
def test_scatter_maps_agree_with_the_headers_formulas_evaluated_per_element(c):
    """The header's prose, evaluated per element as an index into an array of the shape the header gives — not as a flat offset."""
    from vidil_amd import kernels

    d = gc.inputs(c)
    V = gc.source_values(c, d)
    shapes = gc.dest_shapes(c)
    want = {n: np.full(s, np.nan) for n, (s, _) in shapes.items()}
    if c.tiled:
        nt = c.Tk_cap // 32
        want["k"] = np.full((c.B, c.H, nt, 8, 32, 8), np.nan)
        want["vt"] = np.full((c.B, c.H, nt, 2, 2, 2, 32, 8), np.nan)
    for m in range(c.M):
        for n in range(c.N):
            v = V[m, n]
            if c.epi == EPI_PATCH:
                want["out"][m + m // c.tpi + 1, n] = v
                continue
            part, h, dd = c.part0 + n // c.HD, (n % c.HD) // 64, n % 64
            b, t = divmod(m, c.T)
            key = c.t_off + t
            if c.epi == EPI_ARENA:
                if part == 0:
                    want["q"][m, n % c.HD] = v
                else:
                    want[("k", "vt")[part - 1]][key, b * c.slot_stride, n % c.HD] = v
            elif part == 0:
                want["q"][b, h, t, dd] = v
            elif c.tiled and part == 1:
                want["k"][b, h, key // 32, dd // 8, key % 32, dd % 8] = v
            elif c.tiled:
                g = (key % 16) // 4
                want["vt"][b, h, key // 32, (key % 32) // 16, dd // 32, g % 2, dd % 32, (g // 2) * 4 + key % 4] = v
            elif part == 1 or c.NP == 0:
                want[("k", "vt")[part - 1]][b, h, key, dd] = v
            else:
                want["vt"][b, h, dd, 16 * (key // 16) + VT_ORDER.index(key % 16)] = v
    for name, (vals, written, _) in gc.expected(c, d).items():
        w = want[name].reshape(-1)
        assert np.array_equal(written, ~np.isnan(w)), name
        assert np.array_equal(vals[written], w[written]), name
    # ... and the helpers of vidil_amd.kernels that other tests build these buffers with
    for t in range(64):
        assert kernels.vt_pos(t) == gc.vt_col(t) == 16 * (t // 16) + VT_ORDER.index(t % 16)
    ko, vo = kernels.kv_tile_offsets(70)
    for t in range(70):
        for dd in range(64):
            assert ko[t, dd].item() == gc.ktile_off(t, dd) and vo[t, dd].item() == gc.vtile_off(t, dd)


def test_tiny_cases_cover_what_their_maps_exist_for():
    hv, ht, ar, pa = TINY
    assert hv.t_off % 16 and (hv.t_off + hv.T) // 16 > hv.t_off // 16           # vt(t): blocks entered in the middle
    assert ht.t_off // 32 != (ht.t_off + ht.T - 1) // 32                        # tiles: a sequence that crosses a 32-key tile
    assert ar.slot_stride > 1 and ar.t_off and pa.tpi > 1


# ------------------------------------------------------------------------------------------------ the activation bounds
@pytest.mark.parametrize("key,act", [("gelu_erf_f32", ACT_GELU_ERF), ("quick_gelu_f32", ACT_QUICK_GELU)])
def test_an_f32_activation_bound_is_four_times_the_error_of_torchs_own_f32_evaluation(key, act):
    bound, recorded = gc.BOUNDS[key]
    m = gc.measure_f32_activation(act)
    print(f"{key}: torch f32 against float64 on the grid: {m:.3e} (recorded {recorded:.3e}), bound {bound:.3e}")
    assert bound <= 4 * recorded * 1.001
    assert 0.5 * recorded <= m <= 2 * recorded          # (another host's vector math library may differ in the last place)
    # the grid is what the activation cases feed: every multiple of 1/8 in [-6, 6]
    assert gc.GRID[0] == -6.0 and gc.GRID[-1] == 6.0 and len(gc.GRID) == 97


def test_bound_of_16bit_activation_rows_is_the_polynomials_bound_plus_half_an_ulp():
    for name in ("s64_gelu16_f16", "s64_gelu16_bf16", "s64_quick16_bf16"):
        c = gc.BY_NAME[name]
        ref = np.array([1.0, 1.5, -0.17, 5.9, 1e-6])
        b = gc.act_bound(c, ref)
        mant = 10 if c.dtype == "f16" else 7
        base = gc.GELU16_ABS[c.dtype] if c.act == ACT_GELU_ERF else gc.BOUNDS["quick_gelu_f32"][0]
        assert np.allclose(b[:2], base + 0.5 * 2.0 ** -mant) and np.isclose(b[3], base + 0.5 * 2.0 ** (2 - mant))
        assert np.isclose(b[4], base + 0.5 * 2.0 ** ((-14 if c.dtype == "f16" else -20) - mant))     # (1e-6: subnormal in f16 only)
    assert gc.GELU16_ABS == {"f16": 4.5e-5, "bf16": 2.0e-4}


# ------------------------------------------------------------------------------------------------ the verdict itself
PROBES = ["s64_m1_n+8", "s64_m3_n-8_ldo+8_resid_alias", "s64_heads_T9_H1_p0x3_row", "s64_heads_T33_H3_p0x3_vt_shifted",
          "s64_heads_T8_H3_p1x2_tiled", "s64_arena_T5_s3_p0", "s64_patch_tpi4", "s64_gelu16_bf16", "s64_quick32_bf16"]


@pytest.mark.parametrize("name", PROBES)
def test_the_verdict_accepts_a_faithful_result_and_names_every_kind_of_wrong_store(name):
    """`verdict` is what the GPU test asserts: fed the reference itself it is silent; a store into either guard, into a capacity
    row / column / slot, a value one unit in the last place off and a store that never happened are each reported."""
    c = gc.BY_NAME[name]
    d = gc.inputs(c)
    for dest, (vals, written, _) in gc.expected(c, d).items():
        shape, kind = gc.dest_shapes(c)[dest]
        it, sentinel = gc.int_type(kind)
        good = np.full(vals.size + 2 * gc.GUARD, sentinel, dtype=it)
        inside = good[gc.GUARD:gc.GUARD + vals.size]
        inside[written] = gc.bits_of(c, kind, vals)[written]
        assert gc.verdict(c, dest, good, vals, written) is None
        first, last = np.flatnonzero(written)[[0, -1]]
        free = np.flatnonzero(~written)
        one = gc.bits_of(c, kind, np.ones(1))[0]

        def broken(pos, value):
            bad = good.copy()
            bad[pos] = value
            return gc.verdict(c, dest, bad, vals, written)

        assert "guard in front" in broken(gc.GUARD - 1, one) and "guard in front" in broken(0, one)
        assert "guard behind" in broken(gc.GUARD + vals.size, one) and "guard behind" in broken(good.size - 1, one)
        for pos in (free[0], free[-1], free[free > last][0] if (free > last).any() else free[-1]):
            assert "outside the written region" in broken(gc.GUARD + pos, one), (dest, pos)
        for pos in (first, last):
            if c.exact:
                assert "differ from the exact result" in broken(gc.GUARD + pos, good[gc.GUARD + pos] ^ 1), (dest, pos)   # one ulp
                assert "differ from the exact result" in broken(gc.GUARD + pos, sentinel), (dest, pos)                  # never stored
            else:
                assert "not finite" in broken(gc.GUARD + pos, sentinel), (dest, pos)
                assert "of the bound" in broken(gc.GUARD + pos, gc.bits_of(c, kind, vals[pos:pos + 1] + 0.07)[0]), (dest, pos)
