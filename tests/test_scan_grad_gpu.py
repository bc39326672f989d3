"""The gradient form of the scan (`vidil_scan_topk` with `topk == VIDIL_SCAN_FORM_GRAD`) on the GPU: every case of
tests/scan_grad_cases.py against fp64 on the same f32 inputs, in sentinel-filled outputs with room behind the stated extents; two
calls, a pair alone, the pairs in reverse order and the pairs inside a larger launch give the same bits; the wrapper returns the
entry point's bits."""
import ctypes

import pytest
import torch

import scan_grad_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [c.name for c in gc.CASES]
SENTINEL_F, SENTINEL_I = -7.25e30, -77777777
TAIL = 64


def raw_grad(val, wgt, keys, seg_start, seg_len, lv, lw, cv, cw, hard):
    """The entry point itself on sentinel-filled outputs with TAIL elements to spare -> (G [P,D], T [P], C [P]) on the device,
    after asserting that exactly the stated extents were written (out_index not at all) and that the packed inputs are unchanged."""
    from vidil_amd import _lib, kernels as K

    lib = _lib.load()
    P, D = val.shape
    ncat = len(seg_start)
    packed = torch.cat([val.reshape(-1), wgt.reshape(-1), lv, lw, cv, cw, hard.view(torch.float32)]).contiguous()
    assert torch.equal(packed[-P:].view(torch.int32), hard)                       # (the index bits survive the packing)
    before = packed.clone()
    ws = torch.empty(K.scan_topk_ws_bytes(2 * P, keys.shape[0], gc.FORM), dtype=torch.uint8, device=DEV)
    n = P * D + 2 * P
    out_s = torch.full((n + TAIL,), SENTINEL_F, dtype=torch.float32, device=DEV)
    out_i = torch.full((TAIL,), SENTINEL_I, dtype=torch.int32, device=DEV)
    ss, sl = (ctypes.c_int32 * ncat)(*seg_start), (ctypes.c_int32 * ncat)(*seg_len)
    rc = lib.vidil_scan_topk(packed.data_ptr(), keys.data_ptr(), 2 * P, D, ncat, ss, sl, gc.FORM, ws.data_ptr(), out_i.data_ptr(),
                             out_s.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vidil_last_error()
    torch.cuda.synchronize()
    assert (out_s[n:] == SENTINEL_F).all() and (out_i == SENTINEL_I).all()
    assert (out_s[:n] != SENTINEL_F).all()
    assert torch.equal(packed.view(torch.int32), before.view(torch.int32))
    return out_s[:P * D].view(P, D), out_s[P * D:P * D + P], out_s[P * D + P:n]


def on_device(c):
    val, wgt, keys, ss, sl, lv, lw, cv, cw, hard = gc.inputs(c)
    return (val.to(DEV), wgt.to(DEV), keys.to(DEV), ss, sl) + tuple(t.to(DEV) for t in (lv, lw, cv, cw, hard))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_gradient_weighted_sum_and_coefficient_sum_stay_within_four_times_the_f32_error_and_nothing_else_is_written(c):
    args = on_device(c)
    out = raw_grad(*args)
    assert all(torch.isfinite(t).all() for t in out)                     # (no NaN row between the segments reached a result)
    err, bound = gc.errors(c, *out), gc.bounds(c)
    print(f"{c.name}: errors {['%.3e' % e for e in err]} bounds {['%.3e' % b for b in bound]}")
    for q in range(3):
        assert err[q] <= bound[q], (gc.OUTPUTS[q], err[q], bound[q])
    assert same(raw_grad(*args), out)                                    # a second call: the same bits


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_the_wrapper_returns_the_entry_points_bits(c):
    from vidil_amd import kernels as K

    args = on_device(c)
    G, T, C = raw_grad(*args)
    P, D = args[0].shape
    if c.hard:
        G2, T2, C2 = K.scan_softmax_grad(*args[:9], hard=args[9])
        assert C2.shape == (P,) and torch.equal(bits(C2), bits(C))
    else:
        G2, T2 = K.scan_softmax_grad(*args[:9])
    assert G2.shape == (P, D) and T2.shape == (P,) and G2.dtype == T2.dtype == torch.float32
    assert torch.equal(bits(G2), bits(G)) and torch.equal(bits(T2), bits(T))


ALONE = [c for c in gc.CASES if c.base.P > 1]


def _rows(args, sel):
    """The call's arguments restricted to / reordered by the pair indices ``sel``."""
    val, wgt, keys, ss, sl = args[:5]
    return (val[sel].contiguous(), wgt[sel].contiguous(), keys, ss, sl) + tuple(t[sel].contiguous() for t in args[5:])


@pytest.mark.parametrize("c", ALONE, ids=[c.name for c in ALONE])
def test_a_pair_gives_the_bits_it_gives_in_the_batch_alone_reversed_and_inside_a_larger_launch(c):
    args = on_device(c)
    P = c.base.P
    out = raw_grad(*args)
    for p in sorted({0, 15, 16, P - 1} & set(range(P))):
        one = raw_grad(*_rows(args, torch.tensor([p], device=DEV)))
        assert same([t[0] for t in one], [t[p] for t in out]), p
    rev = torch.arange(P - 1, -1, -1, device=DEV)
    assert same([t.flip(0) for t in raw_grad(*_rows(args, rev))], out)
    # inside a launch of another size, at another position: 19 pairs in front (another tile, another lane), 3 behind
    big = torch.cat([torch.arange(19, device=DEV) % P, torch.arange(P, device=DEV), torch.arange(3, device=DEV) % P])
    assert same([t[19:19 + P] for t in raw_grad(*_rows(args, big))], out)
