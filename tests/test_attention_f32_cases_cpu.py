"""The preconditions of tests/test_attention_f32_forms_gpu.py, asserted without a GPU, and the refusals of `vidil_attention_f32`
(host-side checks: the library is called with a null stream and launches nothing)."""
import ctypes

import pytest
import torch

import attention_f32_cases as ac

IDS = [c.name for c in ac.CASES]


def test_every_kernel_of_the_family_is_reached_in_both_16bit_types_and_each_case_reaches_the_kernel_it_names():
    for c in ac.CASES:
        assert ac.expected_kernel(c) == f"{c.kernel}<{c.t16}>", c.name
    reached = {ac.expected_kernel(c) for c in ac.CASES}
    assert reached == {f"{k}<{t}>" for k in ac.KERNELS for t in ("f16", "bf16")}
    # ... and what the issue names of each: unit forms, output forms, a kv_rows beyond Nk, a spiked case
    for k in (ac.VALU, ac.MFMA, ac.SPLIT, ac.RELB):
        mine = [c for c in ac.CASES if c.kernel == k]
        assert {"group", "index", "start"} <= {c.unit for c in mine}, k
    for k in ac.KERNELS:
        mine = [c for c in ac.CASES if c.kernel == k]
        assert {("f16", 3), ("bf16", 3), ("f16", 2)} <= {(c.out, c.planes) for c in mine}, k
        assert k == ac.KV16 or any(c.out == "f32" for c in mine), k
        assert k in (ac.ARENA, ac.GATHER) or any(c.kv_pad for c in mine), k
        assert k in (ac.ARENA, ac.GATHER) or any(c.spiked for c in mine), k
    assert all(c.Bq <= 8 and c.H in (2, 3) for c in ac.CASES)
    # the VALU kernel beyond wave 0 / workgroup 0 is reachable through the fallback alone
    assert sum(c.kernel == ac.VALU and ac.max_rows(c) > 32 for c in ac.CASES) >= 2
    assert set(ac.BOUNDS) == {c.name for c in ac.CASES if c.measured}


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_inputs_and_reference_are_well_formed(c):
    d = ac.inputs(c)
    ref, written, nokey = ac.reference(c)
    assert ref.shape == (c.Bq * c.Nq, c.C) and torch.isfinite(ref).all()
    assert d["q"].stride(0) == 3 * c.C and d["q"].storage_offset() == c.C              # a column slice
    assert not ref[~written].any() and not ref[nokey].any()
    assert written.any() and (nokey.sum() == written.sum() or ref[written & ~nokey].abs().max() > 0.1)
    if c.form == "dense":
        assert d["k"].stride(0) == 2 * c.C and d["v"].storage_offset() == c.C
    if c.unit == "start":
        assert not written.all()                                                        # query batches that no group names
    if c.kv_len is not None:
        assert len(c.kv_len) == c.Bq
        if c.unit != "index" and not c.causal:
            assert {c.Nk, 1, 0} <= set(c.kv_len)
    if c.causal_off < 0 or (c.kv_len is not None and 0 in c.kv_len):
        assert nokey.any()


@pytest.mark.parametrize("c", [c for c in ac.CASES if c.spiked], ids=[c.name for c in ac.CASES if c.spiked])
def test_spiked_scores_move_every_rows_maximum_late_by_more_and_by_less_than_klazy(c):
    named = torch.from_numpy(ac.unit_map(c)[0] >= 0)
    if c.spiked == 2:
        named &= torch.arange(c.Bq) % 2 == 1
    s = ac.scores64(c)[named]                                                          # [spiked batches, H, Nq, Nk]
    assert s.abs().max() <= 20.0
    tile = ac.KEY_TILE[c.kernel]
    tmax = torch.stack([s[..., k0:k0 + tile].max(-1).values for k0 in range(0, c.Nk, tile)], -1)       # [.., tiles]
    run = torch.cummax(tmax, -1).values
    raise_ = tmax[..., 1:] - run[..., :-1]                                             # of every later tile over the maximum before it
    assert ((raise_ > ac.KLAZY).any(-1)).all()
    assert (((raise_ > 0) & (raise_ < ac.KLAZY)).any(-1)).all()


EMULATED = [c for c in ac.CASES if ac.emulation_applies(c)]


@pytest.mark.parametrize("c", EMULATED, ids=[c.name for c in EMULATED])
def test_the_split_arithmetic_written_down_on_the_cpu_stays_within_half_of_the_tolerance(c):
    ref, written, nokey = ac.reference(c)
    tol = ac.tolerance(c, ref)
    assert isinstance(tol, float)                   # (the elementwise bound belongs to f32 arithmetic)
    for lazy in (False, True):
        out = ac.emulate(c, lazy)
        assert not out[nokey].any()
        e = (out - ref)[written].abs().max().item()
        assert e <= 0.5 * tol, (c.name, lazy, e, tol)


MEASURED = [c for c in ac.CASES if c.measured]


@pytest.mark.parametrize("c", MEASURED, ids=[c.name for c in MEASURED])
def test_a_measured_bound_is_at_most_four_times_its_cpu_measurement(c):
    bound, recorded = ac.BOUNDS[c.name]
    m = ac.measured_error(c)
    print(f"{c.name}: emulation (exact maximum, stale reference) and f32 errors {ac.cpu_errors(c)}, recorded {recorded:.2e}, bound {bound:.2e}")
    assert bound <= 4 * m and bound <= 4 * recorded
    assert bound >= 2 * m                           # (and not so tight that the emulation itself would miss half of it)


# ------------------------------------------------------------------------------------------------ refusals (no launch)
def test_arguments_outside_the_contract_are_refused_before_any_launch():
    from vidil_amd import _lib

    lib = _lib.load()
    table = (ctypes.c_float * 64)()
    idx = (ctypes.c_int32 * 8)()

    def args(**kw):
        a = _lib.AttnF32Args()
        a.q = a.k = a.v = a.out = 4096
        a.ldq = a.ldk = a.ldv = 384
        a.ldo, a.Bq, a.H, a.Nq, a.Nk, a.kv_rows, a.kv_group, a.scale = 128, 2, 2, 8, 12, 12, 1, 0.125
        a.dtype16 = _lib.DT_F16
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(text, **kw):
        assert lib.vidil_attention_f32(ctypes.byref(args(**kw)), None) == -1, (text, kw)         # VIDIL_EINVAL
        assert text in lib.vidil_last_error(), (lib.vidil_last_error(), kw)

    pi = ctypes.addressof(idx)
    refused(b"kv_rows=11 < Nk=12", kv_rows=11)
    refused(b"Bq=2 not a multiple of kv_group=3", kv_group=3)
    refused(b"group_start needs n_kv and max_group (and no kv_index)", group_start=pi, kv_index=pi, n_kv=1, max_group=2)
    refused(b"group_start needs n_kv and max_group", group_start=pi, n_kv=0, max_group=2)
    refused(b"group_start needs n_kv and max_group", group_start=pi, n_kv=1, max_group=0)
    for arith in (0, 1):
        refused(b"out_mode 0 (f32 rows), 2 (", out_mode=2, ldo=3 * 128 + 1, arith=arith)          # ldo % 3 != 0
        refused(b"out_mode 0 (f32 rows), 2 (", out_mode=3, ldo=3 * 124, arith=arith)              # planes narrower than H * 64
        refused(b"out_mode 0 (f32 rows), 2 (", out_mode=1, arith=arith)
        refused(b"ldo=124 < H*64", ldo=124, arith=arith)
    # the split-operand MFMA kernel stores 16 / 8 bytes at a time: refused, not demoted to the VALU kernel as arith 0 is
    rel = dict(rel_bias=ctypes.addressof(table), rel_bias_ld=32, rel_off=7)
    for kw in (dict(arith=1), dict(arith=2, **rel), dict(arith=1, group_start=pi, n_kv=2, max_group=1, Nq=1)):
        refused(b"(split): output rows must allow 8-byte (split3) / 16-byte (f32) stores", ldo=130, **kw)
        refused(b"(split): output rows must allow", out_mode=2, ldo=3 * 130, **kw)                # 390 % 12 != 0
        refused(b"(split): output rows must allow", out=4096 + 8, **kw)
        refused(b"(split): output rows must allow", out_mode=2, ldo=3 * 128, out=4096 + 8, **kw)
    # kv16: the decode cross-attention's form alone
    kv16 = dict(arith=1, kv16=1, out_mode=2, ldo=3 * 128, kv_rows=32, ldk=0, ldv=0)
    refused(b"kv16 needs arith == 1", **dict(kv16, arith=0))
    refused(b"kv16 must be 0", **dict(kv16, arith=2, **rel))
    refused(b"at most 32 query rows per unit (got 33)", **dict(kv16, Nq=33))
    refused(b"at most 32 query rows per unit (got 36)", **dict(kv16, Nq=9, kv_group=2, kv_index=None, group_start=pi, n_kv=1, max_group=4))
    refused(b"Nk=769 <= 768", **dict(kv16, Nk=769, kv_rows=800))
    refused(b"kv_rows=40 a multiple of 32", **dict(kv16, kv_rows=40))
    refused(b"(kv16): no q_off / causal / kv_len", **dict(kv16, kv_len=pi))
    refused(b"(kv16): no q_off / causal / kv_len", **dict(kv16, causal=1))
    refused(b"(kv16): no q_off / causal / kv_len", **dict(kv16, q_off=64))
    refused(b"(kv16): out_mode 2 / 3", **dict(kv16, out_mode=0, ldo=128))
    refused(b"(kv16): out_mode 2 / 3", **dict(kv16, ldo=3 * 132))                                 # planes no multiple of 8
    # the arena form
    arena = dict(anc=pi, anc_ld=12, arena_rows=4, Nq=1)
    refused(b"one query row per batch (Nq=2)", **dict(arena, Nq=2))
    refused(b"anc_ld=11 >= Nk=12", **dict(arena, anc_ld=11))
    refused(b"arena_rows=0 > 0", **dict(arena, arena_rows=0))
    refused(b"arena_rows=-1 > 0", **dict(arena, arena_rows=-1))
    refused(b"arith=3 (0: f32", arith=3)
