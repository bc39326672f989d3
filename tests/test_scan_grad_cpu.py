"""The preconditions of tests/test_scan_grad_gpu.py and tests/test_itc_backward_gpu.py, asserted without a GPU: the bounds of
tests/scan_grad_cases.py against their CPU measurement, the analytic ITC gradients against torch autograd in fp64 on the literal
formula, and the refusals of the gradient form of `vidil_scan_topk` (host-side checks: the library is called with a null stream
and launches nothing)."""
import ctypes

import pytest
import torch

import itc_backward_cases as ic
import scan_grad_cases as gc
import scan_stats_cases as sc

IDS = [c.name for c in gc.CASES]


def test_the_cases_cover_the_shapes_and_coefficients_the_form_can_go_wrong_at():
    bases = [c.base for c in gc.CASES]
    assert set(sc.CASES) <= set(bases)                                         # every shape of the statistics form ...
    assert {b.classes for b in bases if not b.batch} >= {31, 32, 33, 256, 257, gc.SPLIT - 1, gc.SPLIT, gc.SPLIT + 1}
    assert any(b.batch and b.classes == gc.SPLIT + 1 for b in bases)           # ... a split edge inside the queue segment
    assert {b.D for b in bases} == {8, 64, 256} and {b.P for b in bases} == {1, 16, 17, 33}
    assert {(c.cv, c.cw) for c in gc.CASES if not c.per_p} == {(1.0, 0.4), (1.0, 0.0), (1.0, 1.0)}
    assert any(c.per_p and (c.cv, c.cw) == (0.5, 0.2) for c in gc.CASES)
    assert sum(c.hard for c in gc.CASES) >= 8 and all(any(h.hard and h.base == c.base for h in gc.CASES) for c in gc.CASES if c.base.batch)
    assert set(gc.BOUNDS) == set(IDS) and len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_inputs_and_reference_are_well_formed(c):
    val, wgt, keys, seg_start, seg_len, lv, lw, cv, cw, hard = gc.inputs(c)
    P, D = val.shape
    assert hard.dtype == torch.int32 and hard.shape == (P,)
    assert ((hard >= 0) & (hard < seg_len[0])).all() if c.hard else (hard == -1).all()
    assert not (c.hard and c.base.batch) or hard.tolist() == list(range(P))
    assert all(t.dtype == torch.float32 and t.shape == (P,) for t in (lv, lw, cv, cw))
    v, w, k = gc.scores64(c)
    assert v.shape == (P, sum(seg_len)) and k.shape == (sum(seg_len), D) and torch.isfinite(k).all()
    assert (lv.double() - torch.logsumexp(v, 1)).abs().max() <= 2.0 ** -23 * lv.abs().max().clamp(min=1)
    assert (lw.double() - torch.logsumexp(w, 1)).abs().max() <= 2.0 ** -23 * lw.abs().max().clamp(min=1)
    if c.per_p:
        assert P == 1 or cv.unique().numel() > 1
        assert torch.allclose(cv * P / (1 + (torch.arange(P) % 5) / 4), torch.full((P,), c.cv))
    else:
        assert (cv == c.cv).all() and (cw == c.cw).all()
    G, T, C = gc.reference(c)
    assert G.shape == (P, D) and T.shape == C.shape == (P,) and all(torch.isfinite(t).all() for t in (G, T, C))
    assert G.abs().max() > 0 and T.abs().max() > 0


@pytest.mark.parametrize("c", gc.CASES, ids=IDS)
def test_a_bound_is_at_most_four_times_its_cpu_measurement_or_the_floor(c):
    bound, recorded = gc.BOUNDS[c.name]
    m, floor, used = gc.measured_error(c), gc.floors(c), gc.bounds(c)
    print(f"{c.name}: plain f32 errors {['%.3e' % e for e in m]}, recorded {recorded}, bounds {bound}, floors {['%.3e' % f for f in floor]}")
    for q in range(3):
        assert used[q] == max(bound[q], floor[q])
        if used[q] == floor[q] and floor[q] > bound[q]:
            continue
        assert bound[q] <= 4 * m[q] and bound[q] <= 4 * recorded[q], gc.OUTPUTS[q]
        assert bound[q] >= 2 * m[q], gc.OUTPUTS[q]       # (and the recorded measurement is not stale the other way)


# ------------------------------------------------------------------------------------------------ the mathematics
@pytest.mark.parametrize("alpha", ic.ALPHAS)
@pytest.mark.parametrize("B,D,Q", [(1, 16, 12), (6, 16, 12), (5, 32, 40)])
def test_the_analytic_gradients_equal_autograd_in_fp64_on_the_literal_formula(B, D, Q, alpha):
    feats, queues = ic.features(B, D, Q)
    temp = 0.05
    _, g_i, g_t, g_temp = ic.literal_grads(feats, queues, temp, alpha, torch.float64)
    fi, ft, fim, ftm = (t.double() for t in feats)
    qi, qt = (t.double() for t in queues)
    t64 = torch.tensor(temp, dtype=torch.float64)
    a_i, t_i, d_i, c_i = ic.analytic_direction(fi, fim, torch.cat([ftm, qt]), t64, alpha)     # image -> text
    a_t, t_t, d_t, c_t = ic.analytic_direction(ft, ftm, torch.cat([fim, qi]), t64, alpha)     # text -> image
    for got, want in ((a_i / 2, g_i), (a_t / 2, g_t), ((t_i + t_t) / 2, g_temp), ((d_i + d_t) / 2, g_temp), (c_i / 2, g_i), (c_t / 2, g_t)):
        # both sides sum terms of up to |key| / temp = 20 in fp64: 2^-53 x 20 x some hundred roundings
        assert (got - want).abs().max() <= 1e-13 / temp, (got, want)
    assert g_i.abs().max() > 1e-5 and g_t.abs().max() > 1e-5 and g_temp.abs() > 1e-5          # (far above that tolerance)


# ------------------------------------------------------------------------------------------------ refusals (no launch)
def _call(lib, NF=4, D=64, ncat=1, start=(0,), length=(40,), topk=gc.FORM, img=4096, txt=4096, ws=4096, oi=4096, os_=4096, segs=True):
    ss = (ctypes.c_int32 * max(1, len(start)))(*start)
    sl = (ctypes.c_int32 * max(1, len(length)))(*length)
    return lib.vidil_scan_topk(img, txt, NF, D, ncat, ss if segs else None, sl if segs else None, topk, ws, oi, os_, None)


def test_the_gradient_form_refuses_what_lies_outside_its_contract_before_any_launch():
    from vidil_amd import _lib, kernels as K

    assert K.SCAN_FORM_GRAD == gc.FORM and gc.FORM not in (-1, 9) and not 0 <= gc.FORM <= 8
    lib = _lib.load()

    def refused(text, **kw):
        assert _call(lib, **kw) == -1, (text, kw)                                    # VIDIL_EINVAL
        assert text in lib.vidil_last_error(), (lib.vidil_last_error(), kw)

    refused(b"needs D <= 256 (D=264)", D=264)
    refused(b"the gradient form", D=264)
    refused(b"(D%8==0, D<=1024)", D=1032)
    for D in (0, 4, 12):
        refused(b"(D%8==0, D<=1024)", D=D)
    refused(b"the gradient form needs an even NF", NF=5)
    refused(b"(NF=1)", NF=1)
    refused(b"NF=0", NF=0)
    refused(b"ncat=0 (1..8)", ncat=0)
    refused(b"ncat=9 (1..8)", ncat=9)
    refused(b"category 0: start=16 (must be a multiple of 32)", start=(16,))
    refused(b"category 1: start=48 (must be a multiple of 32)", ncat=2, start=(0, 48), length=(6, 40))
    refused(b"category 0: start=0 (must be a multiple of 32) len=0", length=(0,))
    for null in ("img", "txt", "ws", "oi", "os_"):
        refused(b"scan_topk: null pointer", **{null: None})
    refused(b"scan_topk: null pointer", segs=False)
    refused(b"the gradient form needs a 16-byte aligned workspace", ws=4096 + 8)
    refused(b"the gradient form needs a 16-byte aligned out_score", os_=4096 + 4)


def test_the_other_forms_are_refused_and_sized_as_before():
    from vidil_amd import _lib

    lib = _lib.load()
    for topk in (-1, 9, -3):
        assert _call(lib, topk=topk) == -1
        assert b"scan_topk: topk=%d (1..8)" % topk in lib.vidil_last_error()
    assert lib.vidil_scan_topk_ws_bytes(5, 1000, -1) == 0 and lib.vidil_scan_topk_ws_bytes(512, 58112, -1) == 0
    assert lib.vidil_scan_topk_ws_bytes(5, 1000, -3) == 0
    assert lib.vidil_scan_topk_ws_bytes(5, 1000, 5) == (1000 // 256 + 9) * 32 * 5 * 8
    assert lib.vidil_scan_topk_ws_bytes(4, 1000, 0) == (1000 // 256 + 9) * 32 * 16
    assert lib.vidil_num_entry_points() == 28 == len(_lib.SIGNATURES)
    assert lib.vidil_abi_version() == 13 == _lib.ABI_VERSION


def test_the_workspace_is_no_matrix():
    from vidil_amd import _lib

    lib = _lib.load()
    ws = lib.vidil_scan_topk_ws_bytes(2 * 256, 58112, gc.FORM)
    assert 0 < ws <= 256 * 58112 * 4 // 2 == 29753344, ws                           # half of ONE [256, 58,112] f32 matrix
    # one partial row of D <= 256 floats, one partial T and one partial C per (split of 1024 classes, pair padded to 16): enough for the queue layout
    splits = 1 + (57600 + gc.SPLIT - 1) // gc.SPLIT
    assert ws >= splits * 256 * (256 + 2) * 4
    assert lib.vidil_scan_topk_ws_bytes(2, 32, gc.FORM) >= 16 * 258 * 4
    assert lib.vidil_scan_topk_ws_bytes(0, 32, gc.FORM) == 0 and lib.vidil_scan_topk_ws_bytes(2, 0, gc.FORM) == 0


def test_the_wrapper_refuses_host_tensors_and_mismatched_shapes():
    from vidil_amd import kernels as K

    c = next(c for c in gc.CASES if c.base.name == "d64_p16_c31")
    val, wgt, keys, ss, sl, lv, lw, cv, cw, hard = gc.inputs(c)
    with pytest.raises(K.VidilHipError, match="expected a CUDA/HIP tensor"):
        K.scan_softmax_grad(val, wgt, keys, ss, sl, lv, lw, cv, cw)
    with pytest.raises(K.VidilHipError, match=r"values and weights must both be \[P,D\]"):
        K.scan_softmax_grad(val, wgt[:-1], keys, ss, sl, lv, lw, cv, cw)
    with pytest.raises(K.VidilHipError, match=r"keys must be \[NCpad,64\]"):
        K.scan_softmax_grad(val, wgt, keys[:, :32], ss, sl, lv, lw, cv, cw)
    with pytest.raises(K.VidilHipError, match="outside the 31 key rows"):
        K.scan_softmax_grad(val, wgt, keys, [0], [32], lv, lw, cv, cw)
    with pytest.raises(K.VidilHipError, match=r"lse_w must be f32 \[16\]"):
        K.scan_softmax_grad(val, wgt, keys, ss, sl, lv, lw[:-1], cv, cw)
    with pytest.raises(K.VidilHipError, match=r"coef_v must be f32 \[16\]"):
        K.scan_softmax_grad(val, wgt, keys, ss, sl, lv, lw, cv.double(), cw)
    with pytest.raises(K.VidilHipError, match=r"hard must be i32 \[16\]"):
        K.scan_softmax_grad(val, wgt, keys, ss, sl, lv, lw, cv, cw, hard=hard.long())
    wide = torch.zeros(2, 264)
    with pytest.raises(K.VidilHipError, match="D=264 exceeds the 256 columns"):
        K.scan_softmax_grad(wide, wide, torch.zeros(40, 264), [0], [40], *(torch.zeros(2),) * 4)


def test_itc_loss_and_the_models_grads_keyword_exist():
    import inspect

    from vidil_amd import losses
    from vidil_amd.blip_pretrain import BLIP_Pretrain, BLIP_Pretrain_Video
    from vidil_amd.blip_retrieval import QUEUE_HEAD, BLIP_Retrieval, BLIP_Retrieval_Video

    assert list(inspect.signature(losses.itc_loss).parameters) == ["image_feat", "text_feat", "image_feat_m", "text_feat_m",
                                                                   "image_store", "text_store", "temp", "alpha", "queue_size"]
    assert QUEUE_HEAD == losses.QUEUE_HEAD == 512
    for cls in (BLIP_Retrieval, BLIP_Retrieval_Video, BLIP_Pretrain, BLIP_Pretrain_Video):
        p = inspect.signature(cls.forward).parameters["grads"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    for doc in (BLIP_Retrieval.loss_forward.__doc__, BLIP_Pretrain.forward.__doc__):
        assert "of ``loss_ita`` only" in " ".join(doc.split())
