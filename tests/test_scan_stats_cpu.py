"""The preconditions of tests/test_scan_stats_gpu.py, asserted without a GPU, and the refusals of the paired softmax-statistics
form of `vidil_scan_topk` (`topk == 0`; host-side checks: the library is called with a null stream and launches nothing)."""
import ctypes

import pytest
import torch

import scan_stats_cases as sc

IDS = [c.name for c in sc.CASES]


def test_the_cases_cover_the_shapes_the_form_can_go_wrong_at():
    one = [c for c in sc.CASES if not c.batch]
    assert {c.D for c in sc.CASES} == {8, 64, 256}
    assert {c.P for c in sc.CASES} == {1, 16, 17, 33}
    assert {c.classes for c in one} == {1, 31, 32, 33, 256, 257}          # class-tile edge, chunk edge
    assert {c.temp for c in sc.CASES} == {0.07, 0.001}
    assert any(c.spiked and c.temp == t for c in sc.CASES for t in (0.07,)) and any(c.spiked and c.temp == 0.001 for c in sc.CASES)
    assert sum(c.batch for c in sc.CASES) >= 2 and any(c.batch and c.spiked for c in sc.CASES)
    assert all(c.classes == 257 for c in sc.CASES if c.batch)
    assert set(sc.BOUNDS) == set(IDS) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_inputs_and_reference_are_well_formed(c):
    val, wgt, keys, seg_start, seg_len = sc.inputs(c)
    assert val.dtype == wgt.dtype == keys.dtype == torch.float32
    assert val.shape == wgt.shape == (c.P, c.D) and keys.shape[1] == c.D
    assert torch.allclose(val.norm(dim=1) * c.temp, torch.ones(c.P), atol=1e-5)
    assert torch.allclose(wgt.norm(dim=1) * c.temp, torch.ones(c.P), atol=1e-5)
    used = torch.zeros(keys.shape[0], dtype=torch.bool)
    for s0, n in zip(seg_start, seg_len):
        assert s0 % 32 == 0 and not used[s0:s0 + n].any()
        used[s0:s0 + n] = True
    assert torch.isfinite(keys[used]).all() and torch.isnan(keys[~used]).all()        # whatever lies between segments is NaN
    if c.batch:
        assert seg_len == [c.P, 257] and (c.P % 32 == 0 or (~used).any())
    ref, idx, _ = sc.reference(c)
    assert ref.shape == (c.P, len(seg_start), 5) and torch.isfinite(ref).all()
    assert (ref[..., 1] >= 1).all() and (ref[..., 3] >= 1).all()
    assert not sc.undecided_argmax(c).any()


SPIKED = [c for c in sc.CASES if c.spiked]


@pytest.mark.parametrize("c", SPIKED, ids=[c.name for c in SPIKED])
def test_spiked_keys_raise_every_lanes_maximum_from_tile_to_tile_by_a_factor_that_is_neither_0_nor_1(c):
    """A lane of the kernel holds one row and, of every class tile it visits, the 16 classes of its half (class offset & 4).
    Both halves' maxima must rise from every tile to the next (hence also across a lane's tiles wave, wave + 4, across the eight
    merged states and across chunks), by a step whose exp(-step) is a normal f32 below 1."""
    val, wgt, keys, seg_start, seg_len = sc.inputs(c)
    s0, n = seg_start[-1], seg_len[-1]
    assert n > sc.CHUNK - 1
    k = keys[s0:s0 + n].double()
    half = (torch.arange(n) & 4) != 0
    for rows in (val, wgt):
        s = rows.double() @ k.T
        tmax = []
        for t0 in range(0, n, sc.TILE):
            for h in (False, True):
                sel = (half == h)[t0:t0 + sc.TILE]
                if sel.any():
                    tmax.append(s[:, t0:t0 + sc.TILE][:, sel].max(1).values)
        step = torch.stack(tmax, 1).diff(dim=1)
        full = step[:, :2 * (n // sc.TILE) - 1]                              # a ragged last tile may hold no spike
        assert (full > 0.01).all() and (full < 80).all(), (full.min().item(), full.max().item())


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_a_bound_is_at_most_four_times_its_cpu_measurement(c):
    bound, recorded = sc.BOUNDS[c.name]
    m = sc.measured_error(c)
    print(f"{c.name}: plain f32 errors {['%.3e' % e for e in m]}, recorded {recorded}, bounds {bound}")
    for q in range(5):
        assert bound[q] <= 4 * m[q] and bound[q] <= 4 * recorded[q], sc.OUTPUTS[q]
        assert bound[q] >= 2 * m[q], sc.OUTPUTS[q]       # (and the recorded measurement is not stale the other way)


# ------------------------------------------------------------------------------------------------ refusals (no launch)
def _call(lib, NF=4, D=64, ncat=1, start=(0,), length=(40,), topk=0, img=4096, txt=4096, ws=4096, oi=4096, os_=4096, segs=True):
    ss = (ctypes.c_int32 * max(1, len(start)))(*start)
    sl = (ctypes.c_int32 * max(1, len(length)))(*length)
    return lib.vidil_scan_topk(img, txt, NF, D, ncat, ss if segs else None, sl if segs else None, topk, ws, oi, os_, None)


def test_the_statistics_form_refuses_what_lies_outside_its_contract_before_any_launch():
    from vidil_amd import _lib

    lib = _lib.load()

    def refused(text, **kw):
        assert _call(lib, **kw) == -1, (text, kw)                                    # VIDIL_EINVAL
        assert text in lib.vidil_last_error(), (lib.vidil_last_error(), kw)

    refused(b"needs an even NF", NF=5)
    refused(b"needs an even NF", NF=1)
    refused(b"NF=5", NF=5)
    for D in (0, 4, 12, 1032):
        refused(b"(D%8==0, D<=1024)", D=D)
    refused(b"NF=0", NF=0)
    refused(b"ncat=0 (1..8)", ncat=0)
    refused(b"ncat=9 (1..8)", ncat=9)
    refused(b"category 0: start=16 (must be a multiple of 32)", start=(16,))
    refused(b"category 1: start=48 (must be a multiple of 32)", ncat=2, start=(0, 48), length=(6, 40))
    refused(b"category 0: start=0 (must be a multiple of 32) len=0", length=(0,))
    refused(b"category 0: start=-32", start=(-32,))
    for null in ("img", "txt", "ws", "oi", "os_"):
        refused(b"scan_topk: null pointer", **{null: None})
    refused(b"scan_topk: null pointer", segs=False)
    refused(b"16-byte aligned workspace", ws=4096 + 8)


def test_the_topk_forms_refusals_are_unchanged():
    from vidil_amd import _lib

    lib = _lib.load()
    for topk in (-1, 9):
        assert _call(lib, topk=topk) == -1
        assert b"scan_topk: topk=%d (1..8)" % topk in lib.vidil_last_error()
    for NF in (5, 4):                                                                # an odd NF is the top-k form's to take
        assert _call(lib, NF=NF, topk=3, D=12) == -1
        assert b"scan_topk: NF=%d D=12 (D%%8==0, D<=1024)" % NF in lib.vidil_last_error()
    assert _call(lib, topk=3, start=(16,)) == -1
    assert b"category 0: start=16 (must be a multiple of 32) len=40" in lib.vidil_last_error()
    assert _call(lib, topk=3, img=None) == -1 and b"scan_topk: null pointer" in lib.vidil_last_error()
    assert lib.vidil_scan_topk_ws_bytes(5, 1000, -1) == 0
    assert lib.vidil_scan_topk_ws_bytes(5, 1000, 5) == (1000 // 256 + 9) * 32 * 5 * 8


def test_workspace_size_of_the_statistics_form_and_an_unchanged_abi():
    from vidil_amd import _lib

    lib = _lib.load()
    assert lib.vidil_scan_topk_ws_bytes(2, 32, 0) > 0
    # one 16-byte state per (chunk, padded row); chunks are at most NCpad / 256 plus one ragged chunk per category
    assert lib.vidil_scan_topk_ws_bytes(66, 57600 + 64, 0) >= ((57600 + 255) // 256 + 1) * 96 * 16
    assert lib.vidil_scan_topk_ws_bytes(0, 32, 0) == 0 and lib.vidil_scan_topk_ws_bytes(2, 0, 0) == 0
    assert lib.vidil_num_entry_points() == 28 == len(_lib.SIGNATURES)
    assert lib.vidil_abi_version() == 13 == _lib.ABI_VERSION


def test_the_wrapper_refuses_host_tensors_and_mismatched_shapes():
    from vidil_amd import kernels as K

    val, wgt, keys, ss, sl = sc.inputs(sc.CASES[1])
    with pytest.raises(K.VidilHipError, match="expected a CUDA/HIP tensor"):
        K.scan_softmax_stats(val, wgt, keys, ss, sl)
    with pytest.raises(K.VidilHipError, match=r"values and weights must both be \[P,D\]"):
        K.scan_softmax_stats(val, wgt[:-1], keys, ss, sl)
    with pytest.raises(K.VidilHipError, match=r"keys must be \[NCpad,64\]"):
        K.scan_softmax_stats(val, wgt, keys[:, :32], ss, sl)
    with pytest.raises(K.VidilHipError, match="outside the 31 key rows"):
        K.scan_softmax_stats(val, wgt, keys, [0], [32])
