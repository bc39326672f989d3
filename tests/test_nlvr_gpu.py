"""BLIP_NLVR on the GPU against the reference's own outputs (tests/golden/nlvr_small.npz, written by
tests/golden/make_nlvr_golden.py from the reference's models/nlvr_encoder.py / vit.py; weights from ``portable_init_``, regenerated
here): the twin text encoder's hidden states (cases S, La, Lb, G17, G901 of tests/nlvr_cases.py), predictions (cases E, G),
the ViT at 901 tokens, ``nlvr.evaluation`` and the loss.  f16 and bf16.

Tolerances.
  hidden states   The yardstick is the error of the existing plain path — ``med.BertModel.encode``, 8 layers, same geometry,
                  against the reference's non-twin stack on case S — measured in the same run, in the same operand type.  The
                  twin stack gets 2 x that figure (it rounds two contexts and a folded weight per layer where the plain stack
                  rounds one), never more than the project's HIDDEN_TOL = 6e-3 (tests/test_forward_surface_gpu.py), in f16 and
                  in bf16.  Over the positions whose mask is 1.
  predictions     within the project's two-logit bound x max(1, max|golden|) — f16: 2e-3 (tests/test_models_gpu.py:174); bf16:
                  1.6e-2, the same figure as tests/test_bf16_gpu.py:265 states it for bf16 (every f16 bound there is scaled by the
                  mantissa ratio 2^11 / 2^8) — and the argmax of every sample equal to the reference's (the golden's seed keeps
                  every |p1 - p0| at 10 x the f16 bound or more, so no sample is excluded).
  ViT tokens      max|d| < 2e-2 against oracle/vit_ref (what tests/test_video_retrieval_gpu.py applies to tokens).

Measured on an MI355X, max|d| (hidden states over the masked positions):
            yardstick   S         La        Lb        G17       G901      ViT 901   pred G17  pred G901  pred E
  f16       4.58e-4     4.18e-4   4.29e-4   4.45e-4   4.76e-4   5.18e-4   1.57e-3   1.20e-3   1.48e-3    7.4e-4
  bf16      3.95e-3     3.78e-3   3.78e-3   3.93e-3   3.58e-3   3.27e-3   1.34e-2   3.40e-3   4.86e-3    3.8e-3
(the group_start form of G17 / G901 gives the same figures; evaluation against forward_u8: 0 in both types)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nlvr_cases as nc
from oracle import clip_ref, vit_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
PRED_REL = {"f16": nc.PRED_REL, "bf16": 8 * nc.PRED_REL}          # tests/test_models_gpu.py:174, tests/test_bf16_gpu.py:265


@pytest.fixture(scope="module")
def gold():
    return nc.golden()


@pytest.fixture(scope="module", params=["f16", "bf16"])
def kind(request):
    return request.param


@pytest.fixture(scope="module")
def model(kind):
    from vidil_amd.packing import set_compute_dtype

    m = nc.small_model().to(DEV)
    set_compute_dtype(kind, m)
    return m


@pytest.fixture(scope="module")
def yardstick(kind, gold):
    """max|d| of the existing plain path (med.BertModel.encode, 8 layers) against the reference's non-twin stack on case S."""
    from vidil_amd.packing import set_compute_dtype

    y = nc.yardstick_encoder().to(DEV)
    set_compute_dtype(kind, y)
    e0, _ = nc.case_states("S", 3, 17)
    cross = y.project_cross_kv(e0.reshape(-1, nc.HIDDEN).to(DEV).to(DTYPES[kind]).contiguous(), 3, 17)
    h32, _ = y.encode(dev(gold["S_ids"], torch.int32), dev(gold["S_mask"].sum(1), torch.int32), cross,
                      torch.arange(3, dtype=torch.int32, device=DEV))
    err = worst(h32.view(3, -1, nc.HIDDEN), gold["Y_hidden"], gold["S_mask"])
    print(f"\n[{kind}] yardstick (med.BertModel.encode, 8 layers, case S): max|d| = {err:.3e}")
    return err


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def worst(got, ref, mask):
    d = (got.detach().float().cpu() - torch.from_numpy(np.asarray(ref))).abs()
    return d[torch.from_numpy(np.asarray(mask)).bool()].max().item()


def hidden_tol(yardstick):
    return min(2 * yardstick, nc.HIDDEN_TOL)


def pred_bound(kind, ref):
    return PRED_REL[kind] * max(1.0, float(np.abs(ref).max()))


def check_pred(kind, got, ref, what):
    got = got.detach().float().cpu().numpy()
    err, bound = float(np.abs(got - ref).max()), pred_bound(kind, ref)
    print(f"\n[{kind}] {what}: prediction max|d| = {err:.3e} (bound {bound:.3e})")
    assert got.shape == ref.shape and err <= bound
    assert np.array_equal(got.argmax(1), ref.argmax(1))


def grouped(pair_of):
    from vidil_amd.video import group_table

    gs, mg = group_table(torch.tensor(pair_of), max(pair_of) + 1)
    return gs.to(DEV), mg


# ------------------------------------------------------------------------------------------------ hidden states
@pytest.mark.parametrize("case", [c[0] for c in nc.CASES])
def test_twin_encoder_hidden_states_vs_reference(model, kind, yardstick, gold, case):
    """The reference's call (a list of two encoder states, all-ones image masks, a padding='longest' mask); the grouped cases
    also through ``encode_twin(groups=)`` on one copy of each pair's states, which must serve the same values."""
    _, tokens, lens, pair_of = next(c for c in nc.CASES if c[0] == case)
    te = model.text_encoder
    ids, mask = gold[f"{case}_ids"], gold[f"{case}_mask"]
    e0, e1 = nc.case_states(case, nc.n_pairs(lens, pair_of), tokens)
    r0, r1 = (e0, e1) if pair_of is None else (e0[list(pair_of)], e1[list(pair_of)])
    ones = torch.ones(r0.shape[:2], dtype=torch.long, device=DEV)
    out = te(dev(ids), attention_mask=dev(mask), encoder_hidden_states=[r0.to(DEV), r1.to(DEV)],
             encoder_attention_mask=[ones, None], return_dict=True, mode="multimodal")
    last = out.last_hidden_state
    tol = hidden_tol(yardstick)
    err = worst(last, gold[f"{case}_hidden"], mask)
    print(f"\n[{kind}] case {case}: hidden max|d| = {err:.3e} (yardstick {yardstick:.3e}, tolerance {tol:.3e})")
    assert tuple(last.shape) == ids.shape + (nc.HIDDEN,) and last.dtype == torch.float32
    assert err <= tol
    if pair_of is not None:
        B = max(pair_of) + 1
        cdt = DTYPES[kind]
        c0, c1 = te.project_twin_kv(*(e.reshape(-1, nc.HIDDEN).to(DEV).to(cdt).contiguous() for e in (e0, e1)), B, tokens)
        gs, mg = grouped(pair_of)
        h32, h16 = te.encode_twin(dev(ids, torch.int32), dev(mask.sum(1), torch.int32), c0, c1, groups=gs, max_group=mg)
        err_g = worst(h32.view(last.shape), gold[f"{case}_hidden"], mask)
        print(f"[{kind}] case {case}, group_start form: hidden max|d| = {err_g:.3e}")
        assert err_g <= tol and h16.dtype == cdt
        check_pred(kind, model.classify(h16, len(lens), ids.shape[1]), gold[f"{case}_pred"], f"case {case}")


# ------------------------------------------------------------------------------------------------ ViT at 901 tokens
def test_vit_at_901_tokens_vs_the_oracle(model, kind):
    x = clip_ref.preprocess_u8(nc.pixels()[:2])
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = vit_ref.vit_forward(sd, x, depth=2, heads=nc.HEADS)
    y32, y16 = model.visual_encoder.forward_both(x.to(DEV))
    err = (y32.cpu() - ref).abs().max().item()
    print(f"\n[{kind}] ViT at 901 tokens: max|d| = {err:.3e}")
    assert tuple(y32.shape) == (2, nc.TOKENS, nc.HIDDEN) and tuple(y16.shape) == (2 * nc.TOKENS, nc.HIDDEN)
    assert err < 2e-2


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def case_e(model, gold):
    """(image f32 [4,3,480,480] = cat([image0, image1]) on the device, sentences, the device's own prediction)."""
    image = clip_ref.preprocess_u8(nc.pixels()).to(DEV)
    text = nc.sentences(gold["E_ids"], gold["E_mask"])
    return image, text, model(image, text, None, train=False)


def test_forward_end_to_end_at_480_vs_reference(model, kind, gold, case_e):
    _, text, pred = case_e
    assert np.array_equal(model.tokenize(text)[0].numpy(), gold["E_ids"])
    assert pred.dtype == torch.float32 and pred.is_cuda
    check_pred(kind, pred, gold["E_pred"], "case E (forward, 480 x 480)")


def test_forward_train_returns_the_cross_entropy_of_its_own_prediction(model, case_e):
    image, text, pred = case_e
    targets = torch.tensor([1, 0], device=DEV)
    loss = model(image, text, targets)
    assert loss.dim() == 0 and abs(loss.item() - F.cross_entropy(pred, targets).item()) <= 1e-6


def test_forward_u8_equals_forward_on_the_normalised_frames(model, kind, gold, case_e):
    _, text, pred = case_e
    u8 = torch.from_numpy(nc.pixels()).to(DEV)
    got = model.forward_u8(u8[:2], u8[2:], text)
    check_pred(kind, got, pred.cpu().numpy(), "forward_u8 against forward")
    check_pred(kind, got, gold["E_pred"], "forward_u8 against the reference")


# ------------------------------------------------------------------------------------------------ evaluation
def test_evaluation_serves_forwards_predictions_whatever_the_block_size(model, kind, gold):
    """Case G's sentences over two pairs of images, in shuffled order: the pair-major schedule (ViT once per image, K | V once
    per pair, group_start) against ``forward_u8`` in the reference's call shape (both images once per sentence)."""
    from vidil_amd import nlvr

    text = nc.sentences(gold["G901_ids"], gold["G901_mask"])
    pair = ((0, 2), (1, 3))
    shuffled = [3, 0, 4, 1, 2]
    examples = [(*pair[nc.CASES[4][3][s]], text[s], nc.G_LABELS[s]) for s in shuffled]
    u8 = torch.from_numpy(nc.pixels()).to(DEV)
    i0, i1 = (torch.tensor([e[j] for e in examples], device=DEV) for j in (0, 1))
    want = model.forward_u8(u8[i0], u8[i1], [e[2] for e in examples]).cpu().numpy()
    one, acc1 = nlvr.evaluation(model, nc.pixels(), examples, pairs_per_block=1)
    two, acc2 = nlvr.evaluation(model, u8, examples, pairs_per_block=2)
    auto, _ = nlvr.evaluation(model, u8, examples)
    assert one.dtype == np.float32 and one.shape == (5, 2)
    assert np.array_equal(one, two) and np.array_equal(one, auto)            # bit-equal: a sentence's bits ignore the block size
    check_pred(kind, torch.from_numpy(one), want, "evaluation against forward_u8")
    labels = np.asarray([e[3] for e in examples])
    assert acc1 == acc2 == pytest.approx(float((want.argmax(1) == labels).mean()))
