"""The preconditions of tests/test_attention_forms_gpu.py, asserted without a GPU: the case table of tests/attention_cases.py
reaches every instantiation, launch property, unit form, mask value and output form that the staged and the direct kernel of
`vidil_attention` branch on (the required list is spelled out here as data, not derived from the cases), every case reaches the
kernel it names, the inputs are what the GPU assertions assume, and the kernels' arithmetic written down on the CPU stays within
half of the bound."""
from dataclasses import replace

import pytest
import torch

import attention_cases as ac
from attention_cases import DIRECT, LDS, Launch

IDS = [c.name for c in ac.CASES]
AIDS = [c.name for c in ac.AIMED]
EK = {c.name: ac.expected_kernel(c) for c in ac.CASES + ac.AIMED}


def _of(kernel):
    return [c for c in ac.CASES if c.kernel == kernel]


def test_every_case_reaches_the_kernel_it_names():
    for c in ac.CASES + ac.AIMED:
        assert EK[c.name].kernel == c.kernel and EK[c.name].dt == c.dt, (c.name, EK[c.name])
        assert c.Bq <= 8 and c.H == 3 and c.Nk <= 768
    assert ac.lds_bytes(7) == 61952 and ac.lds_bytes(9) == 79360


def test_the_launches_whose_bits_are_compared_are_in_one_family():
    for c in ac.BITS_LDS:
        assert ac.expected_kernel(c).kernel == LDS and ac.expected_kernel(c).nw == 4 and c.Nq >= 33
        var = {n: ac.expected_kernel(v) for n, v in ac.bits_variants(c).items()}
        assert all(v.kernel == LDS and v.nkt == ac.expected_kernel(c).nkt for v in var.values()), c.name
        assert [var[n].nw for n in ("alone", "index", "start", "start_two_rounds", "start_third_group")] == [4, 4, 4, 8, 8]
        assert var["start_two_rounds"].rb == (2 if c.Nk <= 224 else 1) and var["start_third_group"].rb == 1
    assert {(c.Nk > ac.CHUNK, c.dt, c.vt) for c in ac.BITS_LDS} == {(ch, dt, vt) for ch in (False, True) for dt in ("f16", "bf16") for vt in (True, False)}
    # the streamed kernel's comparison: streamed, staged by the switch, staged by a kv_len table
    c = ac.STREAM_CASE
    assert ac.expected_kernel(c).kernel == ac.expected_kernel(c, "1").kernel == ac.STREAM and ac.family(c) == LDS
    assert ac.expected_kernel(c, "0") == Launch(LDS, "f16", 7, 8, 1, "store_rows_lds")
    assert ac.expected_kernel(replace(c, kv_len=(c.Nk,) * c.Bq)) == Launch(LDS, "f16", 7, 8, 1, "store_rows_lds")


def test_the_staged_kernel_is_reached_in_every_instantiation_with_every_launch_property():
    lds = _of(LDS)
    inst = {(EK[c.name].nkt, EK[c.name].nw, c.dt) for c in lds}
    # 1. all 36 single-chunk instantiations, at the smallest Nk of each NKT, in both V forms
    for nkt in range(1, 10):
        for nw in (4, 8):
            for dt in ("f16", "bf16"):
                assert (nkt, nw, dt) in inst
                mine = [c for c in lds if (EK[c.name].nkt, EK[c.name].nw, c.dt) == (nkt, nw, dt) and c.Nk == 32 * nkt - 13]
                assert {c.vt for c in mine} == {True, False}, (nkt, nw, dt)
    assert {c.Nk for c in lds} >= {32, 224, 288}
    for Nk in (32, 224, 288):
        assert {(EK[c.name].nw, c.vt) for c in lds if c.Nk == Nk} == {(4, True), (4, False), (8, True), (8, False)}
    # rows per unit of each wave count, and what they reach
    plain1 = [c for c in lds if c.Nk <= 288 and c.out == "plain" and c.kv_len is None and not c.causal and not c.spiked]
    assert {ac.max_rows(c) for c in plain1 if EK[c.name].nw == 4} >= {33, 128}
    assert {ac.max_rows(c) for c in plain1 if EK[c.name].nw == 8} >= {129, 256, 257, 384, 385}
    for c in plain1:
        want = 2 if ac.max_rows(c) in (257, 384) or (c.unit == "group" and 256 < ac.max_rows(c) <= 384) else None
        if ac.max_rows(c) in (33, 128, 129, 256, 385):
            want = 1
        assert want is None or EK[c.name].rb == want, c.name
    for dt in ("f16", "bf16"):
        for vt in (True, False):
            assert {EK[c.name].rb for c in plain1 if c.dt == dt and c.vt == vt} == {1, 2}
    # both store paths for plain rows; store_rows through the LDS budget (NKT 8 with 8 waves, NKT 9) and through the pointer
    for c in plain1:
        if c.shift == 0 and c.pad == 0:
            budget = (EK[c.name].nkt, EK[c.name].nw) in ((8, 8), (9, 4), (9, 8))
            assert EK[c.name].store == ("store_rows" if budget else "store_rows_lds"), c.name
    assert {(EK[c.name].nkt, EK[c.name].nw) for c in plain1 if EK[c.name].store == "store_rows" and c.shift == 0} == {(8, 8), (9, 4), (9, 8)}
    assert any(EK[c.name].store == "store_rows" and c.shift == 1 and c.out == "plain" for c in lds)
    # 2. the chunked form
    want = {(Nk, nw, vt, dt) for Nk in (289, 449, 577, 768) for nw in (4, 8) for vt in (True, False)
            for dt in (("f16", "bf16") if Nk in (449, 768) else ("f16",))}
    got = {(c.Nk, EK[c.name].nw, c.vt, c.dt) for c in lds if EK[c.name].nkt == "chunked" and c.name.startswith("chunked_k")}
    assert got == want
    assert all(EK[c.name].rb == 1 for c in lds if EK[c.name].nkt == "chunked")


def test_the_direct_kernel_is_reached_at_every_key_count_row_count_and_layout():
    d = _of(DIRECT)
    # 3. plain rows + V^T
    rows_form = {(c.Nk, ac.max_rows(c), c.dt) for c in d if EK[c.name].nkt == "rows"}
    assert rows_form >= {(Nk, r, dt) for Nk in (33, 64, 65, 96, 97, 197, 577, 768) for r in (1, 3, 32) for dt in ("f16", "bf16")}
    # 4. fragment tiles, both capacities
    tiles = {(c.Nk, c.tk_extra, c.dt) for c in d if EK[c.name].nkt == "tiled"}
    assert tiles >= {(Nk, e, dt) for Nk in (1, 17, 32, 33, 65, 197, 768) for e in (0, 32) for dt in ("f16", "bf16")}
    assert {ac.max_rows(c) for c in d if c.tiled} >= {1, 3, 32}
    # odd and even tile counts of the two-set ring, one tile to twenty-four
    assert {(c.Nk + 31) // 32 for c in d} >= {1, 2, 3, 4, 7, 19, 24}
    for c in d:
        assert c.vt and c.out != "fp8"
        # kv_tiled 1 and 2 are one dispatch up to 768 keys; the row-major twin of a tiled case over 32 keys is in the same family
        if c.tiled:
            assert ac.expected_kernel(replace(c, tiled=2)) == EK[c.name] == ac.expected_kernel(replace(c, tiled=1))
            if c.Nk > 32:
                assert ac.family(replace(c, tiled=0)) == DIRECT


REQUIRED_FORMS = {          # shape -> unit forms, masks and output forms that must be present on it
    "lds4": dict(nw=4), "lds8": dict(nw=8), "direct": dict(nw=1), "chunked": dict(nw=4),
}


def test_unit_forms_masks_and_output_forms_are_reached_on_the_named_shapes():
    for sh, want in REQUIRED_FORMS.items():
        mine = [c for c in ac.CASES if c.name.startswith(sh + "_")]
        kernel = ac.SHAPES[sh][0]
        assert all(c.kernel == kernel for c in mine)
        if sh != "chunked":
            # 5. unit forms
            units = {(c.unit, c.kv_group > 1, c.max_group) for c in mine if c.kv_len is None and not c.causal and c.out == "plain" and not c.pad and not c.shift}
            assert units >= {("group", False, 2), ("group", True, 2), ("index", False, 2), ("start", False, 2), ("start", False, 3)}, sh
            for c in mine:
                if c.unit == "index":
                    assert kernel == DIRECT or c.Nq >= 33
                    idx = ac.unit_map(c)[2]
                    assert sorted(set(idx)) == list(range(c.Bq - 1)) and len(idx) == c.Bq       # a permutation + one batch twice
                if c.unit != "group" or c.kv_len is None:
                    assert EK[c.name].nw == want["nw"] or c.unit == "start" or c.causal, c.name
            # 7. output forms
            outs = {(c.out, c.pad, c.shift) for c in mine}
            assert outs >= {(o, p, s) for o in ("plain", "planes") for p in (0, 8) for s in (0, 1)}, sh
            assert {EK[c.name].store for c in mine} >= {"store_rows", "store_rows/planes"}
        # 6. masks
        lens = [c for c in mine if c.kv_len is not None and not c.causal]
        Nk = ac.SHAPES[sh][1]
        assert any(set(c.kv_len) == {0, 1, 31, 32, 33, Nk - 1, Nk, Nk + 3} for c in lens), sh
        assert all(0 in c.kv_len and len(c.kv_len) == c.Bq for c in mine if c.kv_len is not None)
        assert {c.causal_off for c in mine if c.causal and c.kv_len is None} == {0, 3, -2}
        assert all(c.Nq != c.Nk for c in mine if c.causal)
        assert any(c.causal and c.kv_len is not None for c in mine)
    chunk = [c for c in ac.CASES if c.name.startswith("chunked_len_chunk_edges")]
    assert all({100, 224, 225, 0} <= set(c.kv_len) and EK[c.name].nkt == "chunked" for c in chunk)
    assert {EK[c.name].nw for c in chunk} == {4, 8}
    assert ac.START_GROUPS == (1, 3, 3, 4)
    # group_start on the 8-wave shape with the bound above the largest group: two row tiles of 256, the second of which returns
    # at once for the group of one batch (and for the empty group so does the first)
    c = ac.BY_NAME["lds8_group_start_bound3"]
    assert ac.max_rows(c) == 420 and EK[c.name] == Launch(LDS, "f16", 3, 8, 1, "store_rows_lds") and c.Nq <= 8 * 32 < 2 * c.Nq
    # fp8 rows from NKT 2, 7, 9 and the chunked form, with and without spare columns
    fp8 = {(EK[c.name].nkt, c.pad) for c in ac.CASES if c.out == "fp8"}
    assert fp8 == {(n, p) for n in (2, 7, 9, "chunked") for p in (0, 16)}
    assert all(EK[c.name].store == "store_rows/fp8" and c.kernel == LDS and c.ldo % 16 == 0 for c in ac.CASES if c.out == "fp8")
    assert any(c.out == "planes" and EK[c.name].nkt == "chunked" for c in ac.CASES)
    assert any(c.out == "planes" and c.tiled for c in ac.CASES)
    assert all(c.ldo % 24 == 0 for c in ac.CASES if c.out == "planes") and all(c.ldo % 8 == 0 for c in ac.CASES)
    # 8. spiked scores
    sp = {(c.spiked, EK[c.name].nkt == "chunked", c.dt) for c in ac.CASES if c.spiked}
    assert sp == {(s, ch, dt) for s in (1, 2) for ch in (False, True) for dt in ("f16", "bf16")}
    assert all(c.kernel == LDS and c.Nq < 32 < ac.max_rows(c) for c in ac.CASES if c.spiked == 2 and c.Nk <= 224)


@pytest.mark.parametrize("c", ac.CASES + ac.AIMED, ids=IDS + AIDS)
def test_inputs_and_reference_are_well_formed(c):
    d = ac.inputs(c)
    ref, A, written, nokey = ac.reference(c)
    assert ref.shape == A.shape == (c.Bq * c.Nq, c.C) and torch.isfinite(ref).all() and torch.isfinite(A).all()
    assert (A >= ref.abs() - 1e-12).all()
    assert not ref[~written].any() and not ref[nokey].any()
    assert written.any() and (nokey.sum() == written.sum() or ref[written & ~nokey].abs().max() > 0.1)
    # what the launch must not read is NaN; what it reads is the values
    dt = ac.T16[c.dt]
    assert d["q"].shape == (c.Bq, c.H, c.Tq_cap, 64) and d["q"][:, :, c.Nq:].isnan().all() and c.Tq_cap == c.Nq + 3
    assert d["k"].dtype == d["v"].dtype == d["q"].dtype == dt
    n_kv = d["n_kv"]
    assert d["k"].isnan().sum() == n_kv * c.H * 64 * (c.Tk_cap - c.Nk)
    assert d["v"].isnan().sum() == n_kv * c.H * 64 * ((c.NP if c.NP else c.Tk_cap) - c.Nk)
    if c.tiled:
        assert c.Tk_cap == (c.Nk + 31) // 32 * 32 + c.tk_extra and d["k"].shape == (n_kv, c.H, c.Tk_cap, 64)
    else:
        assert c.Tk_cap == c.Nk + 5 and c.NP == ((c.Nk + 15) // 16 * 16 + 16 if c.vt else 0)
        assert torch.equal(d["k"][:, :, :c.Nk].float(), d["k_vals"])
    if not c.aimed:
        assert (d["v_vals"] != 0).all()
    if c.unit == "start":
        assert not written.all() and written.sum() == 3 * c.Nq                         # query batches 0 and 4 are unnamed
    # a kv_len of 0 (or a negative causal_off) really leaves rows without a key, and nothing else does
    expect = (c.kv_len is not None and any(L == 0 and ac.unit_map(c)[0][b] >= 0 for b, L in enumerate(c.kv_len))) or (c.causal and c.causal_off < 0)
    assert bool(nokey.any()) == bool(expect), c.name


SPIKED = [c for c in ac.CASES if c.spiked]


@pytest.mark.parametrize("c", SPIKED, ids=[c.name for c in SPIKED])
def test_spiked_scores_move_every_spiked_rows_reference_late_by_more_and_by_less_than_klazy(c):
    sel = torch.arange(c.Bq) % 2 == 1 if c.spiked == 2 else torch.ones(c.Bq, dtype=torch.bool)
    s = ac.scores64(c)[sel]                                                            # [spiked batches, H, Nq, Nk]
    assert s.abs().max() <= 20.0
    tmax = torch.stack([s[..., k0:k0 + 32].max(-1).values for k0 in range(0, c.Nk, 32)], -1)           # [.., tiles]
    run = torch.cummax(tmax, -1).values
    raise_ = tmax[..., 1:] - run[..., :-1]                                             # of every later tile over the maximum before it
    late = torch.arange(1, tmax.shape[-1]) >= tmax.shape[-1] // 2
    assert ((raise_ > ac.KLAZY) & late).any(-1).all()
    assert ((raise_ > 0) & (raise_ < ac.KLAZY) & late).any(-1).all()
    if c.spiked == 2:       # the even batches keep their reference from the first tile on: their scores stay N(0, 1)
        e = ac.scores64(c)[~sel]
        emax = torch.stack([e[..., k0:k0 + 32].max(-1).values for k0 in range(0, c.Nk, 32)], -1)
        assert (emax[..., 1:] - emax[..., :1] < ac.KLAZY).all() and e.abs().max() < 2 * ac.KLAZY
    if c.Nk > ac.CHUNK:     # the steps straddle a chunk edge
        t0 = ac.spike_tile0(c.Nk)
        assert t0 * 32 < 2 * ac.CHUNK < (t0 + 3) * 32 and (t0 + 4) * 32 <= c.Nk


@pytest.mark.parametrize("c", ac.CASES, ids=IDS)
def test_the_kernels_arithmetic_written_down_on_the_cpu_stays_within_half_of_the_bound(c):
    ref, A, written, nokey = ac.reference(c)
    bound = ac.bounds(c)
    worst = 0.0
    for stale in (0.0, ac.KLAZY):
        out = ac.emulate(c, stale)
        assert len(out) == len(bound)
        for o, b in zip(out, bound):
            assert not o[nokey].any()
            worst = max(worst, ((o - ref).abs() / b)[written].max().item())
    print(f"{c.name}: emulation at {worst:.2f} of the bound")
    assert worst <= 0.5, (c.name, worst)


RANDOM = [c for c in ac.CASES if not c.spiked and c.out != "fp8"]


@pytest.mark.parametrize("c", RANDOM, ids=[c.name for c in RANDOM])
def test_the_old_tolerance_was_at_least_three_times_the_bound_at_the_median_element(c):
    """rtol = atol = 3e-3 (f16) / 2e-2 (bf16) of tests/test_kernels_gpu.py against bound (a): the gap this file closes."""
    ref, A, written, nokey = ac.reference(c)
    live = written & ~nokey
    old = ac.OLD_TOL[c.dt] * (1.0 + ref.abs())
    ratio = (old / ac.bounds(c)[0])[live].median().item()
    print(f"{c.name}: old tolerance / bound at the median element: {ratio:.1f}")
    assert ratio >= 3.0, (c.name, ratio)


# ---------------------------------------------------------------------------------------------- "every key is read"
def test_targets_are_every_key_or_the_tile_and_chunk_edges():
    assert ac.aimed_targets(51, True) == list(range(51))
    # 449 keys: the first 16-key block, both sides of every 32-key tile edge (224 and 448 are the chunk edges too), and the last
    # 16-key block, which is the last key alone
    assert ac.aimed_targets(449, False) == list(range(16)) + [31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255, 256,
                                                              287, 288, 319, 320, 351, 352, 383, 384, 415, 416, 447, 448]
    t = ac.aimed_targets(768, False)
    assert set(range(752, 768)) <= set(t) and {223, 224, 447, 448, 671, 672, 767} <= set(t) and 768 not in t
    assert ac.aimed_targets(97, False) == list(range(16)) + [31, 32, 63, 64, 95, 96]
    kinds = {(c.kernel, ac.aimed_every(c), c.dt, c.vt, bool(c.tiled)) for c in ac.AIMED}
    for dt in ("f16", "bf16"):
        assert {(LDS, True, dt, True, False), (LDS, True, dt, False, False), (LDS, False, dt, True, False), (LDS, False, dt, False, False),
                (DIRECT, False, dt, True, False), (DIRECT, False, dt, True, True)} <= kinds
    assert {EK[c.name].nkt for c in ac.AIMED if ac.aimed_every(c)} == set(range(1, 10))
    assert {EK[c.name].nw for c in ac.AIMED if c.kernel == LDS} == {4, 8}


@pytest.mark.parametrize("c", ac.AIMED, ids=AIDS)
def test_an_aimed_row_scores_its_target_25_above_every_other_key(c):
    s = ac.scores64(c)
    top2 = s.topk(2, dim=-1)
    assert (top2.values[..., 0] - top2.values[..., 1]).min().item() >= 25.0
    pos = ac.aimed_pos(c)
    units, H, rows = pos.shape
    hit = top2.indices[..., 0].view(units, c.kv_group, H, c.Nq).permute(0, 2, 1, 3).reshape(units, H, rows)
    assert torch.equal(hit, pos)
    assert set(pos.reshape(-1).tolist()) == set(ac.aimed_targets(c.Nk, ac.aimed_every(c)))
    # the reference is that pattern, far inside the bound
    ref = ac.reference(c)[0]
    assert ((ref - ac.aimed_want(c)).abs() <= 0.01 * ac.bounds(c)[0]).all()
