"""The paired softmax-statistics form of the scan (`vidil_scan_topk` with `topk == 0`) on the GPU: every case of
tests/scan_stats_cases.py against fp64 on the same f32 inputs, in f32 sentinel-filled outputs with room behind the stated extents;
output 1 and the index bit-equal to the top-k form; a pair alone gives the bits it gives inside the batch."""
import ctypes

import pytest
import torch

import scan_stats_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [c.name for c in sc.CASES]
SENTINEL_F, SENTINEL_I = -7.25e30, -77777777
TAIL = 64


def raw_stats(val, wgt, keys, seg_start, seg_len):
    """The entry point itself on sentinel-filled outputs with TAIL elements to spare -> (stats [P,ncat,5], index [P,ncat]) on the
    device, after asserting that the tails still hold the sentinel."""
    from vidil_amd import _lib, kernels as K

    lib = _lib.load()
    P, D = val.shape
    ncat = len(seg_start)
    rows = torch.cat([val, wgt], 0).contiguous()
    ws = torch.empty(K.scan_topk_ws_bytes(2 * P, keys.shape[0], 0), dtype=torch.uint8, device=DEV)
    out_s = torch.full((P * ncat * 5 + TAIL,), SENTINEL_F, dtype=torch.float32, device=DEV)
    out_i = torch.full((P * ncat + TAIL,), SENTINEL_I, dtype=torch.int32, device=DEV)
    ss, sl = (ctypes.c_int32 * ncat)(*seg_start), (ctypes.c_int32 * ncat)(*seg_len)
    rc = lib.vidil_scan_topk(rows.data_ptr(), keys.data_ptr(), 2 * P, D, ncat, ss, sl, 0, ws.data_ptr(), out_i.data_ptr(),
                             out_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vidil_last_error()
    torch.cuda.synchronize()
    assert (out_s[P * ncat * 5:] == SENTINEL_F).all() and (out_i[P * ncat:] == SENTINEL_I).all()
    assert (out_s[:P * ncat * 5] != SENTINEL_F).all() and (out_i[:P * ncat] != SENTINEL_I).all()
    return out_s[:P * ncat * 5].view(P, ncat, 5), out_i[:P * ncat].view(P, ncat)


def on_device(c):
    val, wgt, keys, ss, sl = sc.inputs(c)
    return val.to(DEV), wgt.to(DEV), keys.to(DEV), ss, sl


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_the_five_numbers_stay_within_four_times_the_f32_error_and_nothing_else_is_written(c):
    stats, idx = raw_stats(*on_device(c))
    assert torch.isfinite(stats).all()                                   # (no NaN row between the segments reached a result)
    err = sc.errors(c, stats)
    bound = sc.BOUNDS[c.name][0]
    print(f"{c.name}: errors {['%.3e' % e for e in err]} bounds {['%.3e' % b for b in bound]}")
    for q in range(5):
        assert err[q] <= bound[q], (sc.OUTPUTS[q], err[q], bound[q])
    assert torch.equal(idx.cpu().long(), sc.reference(c)[1])


@pytest.mark.parametrize("c", sc.CASES, ids=IDS)
def test_maximum_and_index_are_the_bits_of_the_topk_form_and_the_wrapper_returns_the_same(c):
    from vidil_amd import kernels as K

    val, wgt, keys, ss, sl = on_device(c)
    stats, idx = raw_stats(val, wgt, keys, ss, sl)
    ti, ts = K.scan_topk(val, keys, ss, sl, 1)
    assert torch.equal(stats[..., 0].view(torch.int32), ts[..., 0].view(torch.int32))
    assert torch.equal(idx, ti[..., 0])
    wi, wsc = K.scan_topk(wgt, keys, ss, sl, 1)
    assert torch.equal(stats[..., 2].view(torch.int32), wsc[..., 0].view(torch.int32))
    s2, i2 = K.scan_softmax_stats(val, wgt, keys, ss, sl)
    assert s2.shape == stats.shape and i2.shape == idx.shape
    assert torch.equal(s2.view(torch.int32), stats.view(torch.int32)) and torch.equal(i2, idx)


ALONE = [c for c in sc.CASES if c.P > 1]


@pytest.mark.parametrize("c", ALONE, ids=[c.name for c in ALONE])
def test_a_pair_run_alone_gives_the_bits_it_gives_inside_the_batch(c):
    val, wgt, keys, ss, sl = on_device(c)
    stats, idx = raw_stats(val, wgt, keys, ss, sl)
    for p in sorted({0, 15, 16, c.P - 1} & set(range(c.P))):
        s1, i1 = raw_stats(val[p:p + 1], wgt[p:p + 1], keys, ss, sl)
        assert torch.equal(s1[0].view(torch.int32), stats[p].view(torch.int32)), p
        assert torch.equal(i1[0], idx[p]), p
    # ... and in another position of a launch of another size: the pairs in reverse order
    sr, ir = raw_stats(val.flip(0).contiguous(), wgt.flip(0).contiguous(), keys, ss, sl)
    assert torch.equal(sr.flip(0).view(torch.int32), stats.view(torch.int32)) and torch.equal(ir.flip(0), idx)
