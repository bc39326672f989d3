"""Question answering on the GPU: the candidate form of the one-read log-softmax kernel through the C ABI against float64, its
agreement with the teacher-forced form, masked cross-attention through BertLMHeadModel.score bit for bit, BLIP_VQA (rank,
generate, train=True) against the oracle composed in vqa_cases.py in f16 and bf16, batch independence and the refusals."""
import json
import types

import numpy as np
import pytest
import torch

import caption_scoring_cases as cs
import vqa_cases as vc
from common import load_into
from test_models_gpu import PLAIN_F16_REL, _small_med_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLAIN_BF16_REL = 1e-2          # the bf16 caption-logit gate of tests/test_bf16_gpu.py

# ============================================================================ the candidate kernel, through the C ABI
KERNEL_V = [512, 30524, 38401]
KERNEL_A = [1, 7, 300, 3128]
R = 5                          # rows 0..4: with V = 30,524 the odd rows start 8 bytes off a 16-byte boundary


def _kernel_case(V, A):
    """Rows: standard deviation 1 (row 0) and 20 (row 1), all equal (2), -inf everywhere but three positions (3), std 1 with
    the FIRST candidate's logit -inf (4).  Candidates: random, with a duplicate, -1 and V where A allows."""
    g = torch.Generator().manual_seed(7000 * A + V)
    x = torch.randn(R, V, generator=g)
    x[1] *= 20.0
    x[2] = 3.25
    cand = torch.randint(0, V, (A,), generator=g, dtype=torch.int64)
    keep = torch.tensor([1, V // 2, V - 2])
    if A >= 7:
        cand[1], cand[2], cand[3], cand[4], cand[5] = cand[0], -1, V, 0, V - 1
        cand[6] = V // 2                                   # (a finite entry of row 3)
    row = torch.full((V,), float("-inf"))
    row[keep] = x[3][keep]
    x[3] = row
    x[4][cand[0]] = float("-inf")
    return x, cand


@pytest.fixture(scope="module")
def kernel_cases():
    """Inputs of every (V, A), their float64 log-softmax, and the largest error of torch's own f32 log_softmax on the CPU
    against it over ALL of them (finite entries) — the yardstick the kernel gets 4x of."""
    cases, torch_err = {}, 0.0
    for V in KERNEL_V:
        for A in KERNEL_A:
            x, cand = _kernel_case(V, A)
            lp64 = torch.log_softmax(x.double(), -1)
            lp32 = torch.log_softmax(x, -1).double()
            fin = torch.isfinite(lp64)
            torch_err = max(torch_err, (lp32 - lp64)[fin].abs().max().item())
            cases[(V, A)] = (x, cand, lp64)
    return cases, torch_err


def _abi_candidates(x, cand):
    from vidil_amd import _lib

    lib = _lib.load()
    n, A = x.shape[0], cand.numel()
    d_x, d_c = x.to(DEV), cand.to(torch.int32).to(DEV)
    guard = torch.full((n * A + 8,), 123.0, dtype=torch.float32, device=DEV)      # [n, A] followed by 8 sentinels
    out_i = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    rc = lib.vidil_logsoftmax_topk_penalty(d_x.data_ptr(), None, n, 0, A, x.shape[1], -1, d_c.data_ptr(), 0, 1, 1.0, guard.data_ptr(),
                                           out_i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vidil_last_error()
    torch.cuda.synchronize()
    assert bool((guard[n * A:] == 123.0).all()), "wrote past [rows, A]"
    return guard[:n * A].view(n, A).cpu(), out_i.cpu()


@pytest.mark.parametrize("A", KERNEL_A)
@pytest.mark.parametrize("V", KERNEL_V)
def test_candidate_kernel_vs_float64_log_softmax(kernel_cases, V, A):
    """vidil_logsoftmax_topk_penalty(num_beams=0, beams_in_logits=A) returns VIDIL_OK (the parent does not read beams_in_logits and
    writes [rows, 2]) and out[r, a] equals float64 log_softmax of the same f32 logits at cand[a] within 4x the error of torch's
    own f32 log_softmax on the CPU over these inputs; candidates -1 and V, and -inf logits, give -inf exactly; the argmax is
    the lowest index among equal maxima.
    Measured on an MI355X: torch f32 vs f64 1.391e-05 over these inputs, the kernel's worst |error| 1.391e-05 (1.00x, at
    30,524 x 3,128; 0.02x .. 0.89x elsewhere)."""
    cases, torch_err = kernel_cases
    x, cand, lp64 = cases[(V, A)]
    got, got_i = _abi_candidates(x, cand)
    tol = 4.0 * torch_err
    inside = (cand >= 0) & (cand < V)
    ref = torch.full((R, A), float("-inf"), dtype=torch.float64)
    ref[:, inside] = lp64[:, cand[inside]]
    fin = torch.isfinite(ref)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == float("-inf")).all())
    worst = (got.double() - ref)[fin].abs().max().item()
    print(f"\ncandidate_logprobs ({R} x {V}, A = {A}): torch f32 log_softmax vs f64 on these inputs {torch_err:.3e}; "
          f"kernel worst |error| {worst:.3e} = {worst / torch_err:.2f}x (allowed 4x)")
    assert worst <= tol, (worst, tol)
    assert bool(((got[2].double() + np.log(V))[fin[2]].abs() <= tol).all())          # all-equal row: -log V
    assert got[4, 0].item() == float("-inf")                                         # the candidate's own logit is -inf
    if A >= 7:
        assert got[0, 1].item() == got[0, 0].item() and got[0, 2].item() == float("-inf") and got[0, 3].item() == float("-inf")
        assert np.isfinite(got[3, 6].item())
    for r in range(R):
        assert got_i[r].item() == int((x[r] == x[r].max()).nonzero()[0]), r


def test_one_row_and_the_wrapper():
    from vidil_amd import kernels as K

    x, cand = _kernel_case(30524, 300)
    got, _ = _abi_candidates(x[1:2], cand)                      # a single row (16-byte aligned here, 8 bytes off inside the batch)
    lp64 = torch.log_softmax(x[1].double(), -1)
    tol = 4.0 * (torch.log_softmax(x[1], -1).double() - lp64).abs().max().item()
    inside = (cand >= 0) & (cand < 30524)
    assert bool(((got[0, inside].double() - lp64[cand[inside]]).abs() <= tol).all()) and bool((got[0, ~inside] == float("-inf")).all())
    am = torch.empty((R,), dtype=torch.int32, device=DEV)
    w = K.candidate_logprobs(x.to(DEV), cand.to(torch.int32).to(DEV), out_index=am)
    assert w.shape == (R, 300) and w.dtype == torch.float32
    assert bool(((w[1].cpu().double() - got[0].double())[inside].abs() <= 2.0 * tol).all())
    assert am.cpu().tolist() == [int((x[r] == x[r].max()).nonzero()[0]) for r in range(R)]
    with pytest.raises(K.VidilHipError):
        K.candidate_logprobs(x.to(DEV), cand.to(torch.int32).to(DEV), out=torch.empty((R, 2), device=DEV))


@pytest.mark.parametrize("V", KERNEL_V)
def test_one_candidate_equals_the_teacher_forced_form_bit_for_bit(V):
    """A = 1: out[b, 0] is the teacher-forced form's out_scores[2 b] for labels = cand[0] in every row, and out_index is equal
    in both forms.  The teacher-forced form (beams_in_logits = 0) still writes [rows, 2] and nothing else."""
    from vidil_amd import _lib

    lib = _lib.load()
    x, _ = _kernel_case(V, 1)
    for label in (V // 3, V - 1):
        cand = torch.tensor([label])
        got, got_i = _abi_candidates(x, cand)
        d_x = x.to(DEV)
        lab = torch.full((R,), label, dtype=torch.int32, device=DEV)
        tf = torch.full((2 * R + 8,), 123.0, dtype=torch.float32, device=DEV)
        tf_i = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        rc = lib.vidil_logsoftmax_topk_penalty(d_x.data_ptr(), None, R, 0, 0, V, -1, lab.data_ptr(), 0, 1, 1.0, tf.data_ptr(),
                                               tf_i.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.vidil_last_error()
        torch.cuda.synchronize()
        assert bool((tf[2 * R:] == 123.0).all())
        assert torch.equal(got[:, 0], tf[:2 * R].view(R, 2)[:, 0].cpu()), (got[:, 0], tf[:2 * R].view(R, 2)[:, 0])
        assert torch.equal(got_i, tf_i.cpu())


# ============================================================================ masked cross-attention through the scorer
def _decoder(dtype="f16"):
    from vidil_amd.med import BertLMHeadModel
    from vidil_amd.packing import set_compute_dtype

    _, sd_d = vc.states()
    dec = load_into(BertLMHeadModel(_small_med_cfg()), sd_d, "text_decoder.").to(DEV)
    if dtype != "f16":
        set_compute_dtype(dtype, dec)
    return dec


def _encoder(dtype="f16"):
    from vidil_amd.med import BertModel
    from vidil_amd.packing import set_compute_dtype

    sd_e, _ = vc.states()
    enc = load_into(BertModel(_small_med_cfg()), sd_e, "text_encoder.").to(DEV)
    if dtype != "f16":
        set_compute_dtype(dtype, enc)
    return enc


def _tokens(res, p):
    i = res.tokens_of(p)
    return res.lp_label[i].clone(), res.lp_mean[i].clone(), res.argmax[i].clone()


def test_keys_past_cross_kv_len_never_reach_a_result():
    """score(cross_kv_len=lens) on the oracle's question states padded to 35 — 8 answers over 4 units through image_index —
    equals, bit for bit, score on a per-answer batch of units (one unit per answer) whose pad states are NaN.  The parent's
    score() has no cross_kv_len."""
    g, ref = vc.golden(), vc.reference()
    dec = _decoder()
    lens = torch.from_numpy(g["q_mask"].sum(1))
    st = ref["question_states"].to(DEV).half()                                 # [4, 35, 256]
    Q, Tq, C = st.shape
    pick = torch.tensor([0, 5, 9, 1, 3, 17, 30, 2])
    unit = torch.tensor([0, 0, 1, 2, 2, 3, 3, 1])
    a_ids, a_lens = torch.from_numpy(g["a_ids"])[pick], torch.from_numpy(g["a_mask"]).sum(1)[pick]
    a = dec.score(st.reshape(-1, C).contiguous(), Q, a_ids, a_lens, image_index=unit, prompt_length=1, cross_kv_len=lens)
    per = st[unit].clone()
    pad = torch.arange(Tq, device=DEV)[None, :] >= lens[unit].to(DEV)[:, None]
    per[pad] = float("nan")
    assert bool(torch.isnan(per).any())
    b = dec.score(per.reshape(-1, C).contiguous(), 8, a_ids, a_lens, prompt_length=1, cross_kv_len=lens[unit])
    assert bool(torch.isfinite(b.loss_sum).all()) and torch.equal(a.count, b.count)
    assert torch.equal(a.loss_sum, b.loss_sum), (a.loss_sum - b.loss_sum).abs().max().item()
    for p in range(8):
        for x, y in zip(_tokens(a, p), _tokens(b, p)):
            assert torch.equal(x, y), p
    # the mask is what is compared: without it the answers of the short questions score differently
    c = dec.score(st.reshape(-1, C).contiguous(), Q, a_ids, a_lens, image_index=unit, prompt_length=1)
    assert not torch.equal(a.loss_sum[:3], c.loss_sum[:3])
    # image-major groups give the numbers of image_index
    order = sorted(range(8), key=lambda p: (int(unit[p]), p))
    d = dec.score(st.reshape(-1, C).contiguous(), Q, a_ids[order], a_lens[order], group_start=[0, 2, 4, 6, 8], prompt_length=1,
                  cross_kv_len=lens)
    assert torch.equal(a.loss_sum[order], d.loss_sum)


def test_cross_kv_len_none_is_the_caption_scoring_case_unchanged():
    """cross_kv_len=None issues the launches of the parent; cross_kv_len = the full 17 image tokens masks nothing: the existing
    7-caption case scores bit-identically either way."""
    sd, enc = cs.small_state()
    from vidil_amd.med import BertLMHeadModel

    dec = load_into(BertLMHeadModel(_small_med_cfg()), sd, "text_decoder.").to(DEV)
    ref = cs.reference()
    flat = enc.to(DEV).half().reshape(-1, 256).contiguous()
    kw = dict(image_index=cs.IMAGE_INDEX, prompt_length=cs.PROMPT_LENGTH)
    a = dec.score(flat, 3, ref["ids"], ref["mask"].sum(1), **kw)
    b = dec.score(flat, 3, ref["ids"], ref["mask"].sum(1), cross_kv_len=None, **kw)
    c = dec.score(flat, 3, ref["ids"], ref["mask"].sum(1), cross_kv_len=[17, 17, 17], **kw)
    for r in (b, c):
        assert torch.equal(a.loss_sum, r.loss_sum) and torch.equal(a.lp_label, r.lp_label) and torch.equal(a.argmax, r.argmax)
    g = PLAIN_F16_REL * max(1.0, ref["logits"].abs().max().item())
    assert bool(((a.loss_sum.cpu() - ref["none"]).abs() <= 2.0 * ref["counts"].float() * g).all())


# ============================================================================ the model, small geometry
class _TokensViT(torch.nn.Module):
    """Stands in for the ViT: hands out the golden image tokens of the questions' images."""

    def __init__(self, enc16):
        super().__init__()
        self.enc16 = enc16
        self.patch_embed = types.SimpleNamespace(num_patches=enc16.shape[1] - 1)

    def forward_both(self, x):
        e = self.enc16[:x.shape[0]]
        return e.float(), e.reshape(-1, e.shape[-1])


@pytest.fixture(scope="module")
def small_med_json(tmp_path_factory):
    c = _small_med_cfg()
    path = tmp_path_factory.mktemp("cfg") / "med_small.json"
    path.write_text(json.dumps({k: getattr(c, k) for k in ("hidden_size", "num_attention_heads", "intermediate_size",
                                                           "num_hidden_layers", "vocab_size", "max_position_embeddings",
                                                           "encoder_width")}))
    return str(path)


_MODELS = {}


def _model(small_med_json, dtype="f16"):
    from vidil_amd.blip_vqa import BLIP_VQA
    from vidil_amd.packing import set_compute_dtype

    if dtype not in _MODELS:
        g = vc.golden()
        m = BLIP_VQA(med_config=small_med_json, image_size=32, vit="base", tokenizer=vc.VqaTokenizer())
        m.text_encoder, m.text_decoder = _encoder(), _decoder()
        tdt = torch.float16 if dtype == "f16" else torch.bfloat16
        m.visual_encoder = _TokensViT(torch.from_numpy(g["enc"])[torch.from_numpy(g["q_image"])].to(DEV).to(tdt).contiguous())
        set_compute_dtype(dtype, m)
        _MODELS[dtype] = m
    return _MODELS[dtype]


def _gate(dtype):
    return PLAIN_F16_REL if dtype == "f16" else PLAIN_BF16_REL


def _states(m, g):
    img = torch.zeros(4, 3, 32, 32, device=DEV)
    _, y16 = m.visual_encoder.forward_both(img)
    ids, lens = m.tokenize_questions(vc.questions(g))
    h32, h16 = m.question_states(y16, 4, ids, lens)
    return img, y16, ids, lens, h32, h16


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_rank_and_loss_vs_composed_oracle(small_med_json, dtype):
    """Question states and first-token logits within the plain gates (1.25e-3 x scale f16, 1e-2 x scale bf16); topk_ids and
    max_ids equal the oracle's for every question the oracle decides by more than gate x scale x 2 x target tokens (at most
    one of the four may be excluded; none is for f16 by the fixture's seed); the train=True loss within the gate x target
    count of its answers."""
    g, ref = vc.golden(), vc.reference()
    m = _model(small_med_json, dtype)
    gate = _gate(dtype)
    img, y16, ids, lens, h32, h16 = _states(m, g)
    Q, k = 4, int(g["k"])
    qs = ref["question_states"].reshape(-1, 256)
    s_scale = max(1.0, qs.abs().max().item())
    e_states = (h32.cpu() - qs).abs().max().item()
    a_ids, a_lens = m.tokenize_answers(vc.answers(g))
    logits = m.text_decoder.start_logits(h16, Q, vc.DEC, cross_kv_len=lens)
    l_scale = max(1.0, ref["first_logits"].abs().max().item())
    e_logits = (logits.cpu() - ref["first_logits"]).abs().max().item()
    lp = m.first_token_logprobs(h16, Q, lens, a_ids)
    e_lp = (lp.cpu().double() - ref["lp64"]).abs().max().item()
    max_ids, topk_ids, sums = m.rank_answer(h16, Q, lens, a_ids, a_lens, k)
    out = m(img, vc.questions(g), vc.answers(g), train=False, inference="rank", k_test=k)
    assert out.dtype == torch.int64 and out.is_cuda and torch.equal(out, max_ids)
    tok_obj = types.SimpleNamespace(input_ids=a_ids.to(DEV), attention_mask=torch.from_numpy(g["a_mask"]).to(DEV))
    assert torch.equal(m(img, vc.questions(g), tok_obj, train=False, inference="rank", k_test=k), max_ids)
    ex = vc.excluded(gate)
    print(f"\nBLIP_VQA {dtype}: |d states| {e_states:.3e} (gate {gate * s_scale:.3e}), |d first logits| {e_logits:.3e} (gate "
          f"{gate * l_scale:.3e}), |d first-token lp| {e_lp:.3e}; questions excluded by the oracle's own margins: {int(ex.sum())} of {Q}")
    assert e_states <= gate * s_scale and e_logits <= gate * l_scale and e_lp <= 2.0 * gate * l_scale
    assert int(ex.sum()) <= 1
    unit = 2.0 * gate * ref["scale"]
    if dtype == "f16":
        assert int(ex.sum()) == 0
    for q in range(Q):
        if not bool(ex[q]):
            # the k/(k+1) margin protects the SET of selected answers; their order inside the k is the oracle's at every rank
            # whose first-token log-probability is further than the same margin from both neighbours
            mine, want = topk_ids[q].cpu().tolist(), ref["topk_ids"][q].tolist()
            assert sorted(mine) == sorted(want), q
            srt = ref["lp64"][q].sort(descending=True).values
            for r in range(k):
                if (r == 0 or srt[r - 1] - srt[r] > unit) and srt[r] - srt[r + 1] > unit:
                    assert mine[r] == want[r], (q, r)
            assert int(max_ids[q]) == int(ref["max_ids"][q]) == int(g["max_ids"][q]), q
            by_id = dict(zip(want, ref["log_probs_sum"][q].tolist()))
            for j, a in enumerate(mine):
                assert abs(sums[q, j].item() - by_id[a]) <= 2.0 * float(ref["n_targets"][a]) * gate * ref["scale"], (q, a)
    # train=True (models/blip_vqa.py:46-81)
    ta = g["train_answers"]
    answers = vc.answers(g)
    loss = m(img, vc.questions(g), [answers[i] for i in ta], n=g["n_train"].tolist(), weights=torch.from_numpy(g["train_weights"]))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    bound = float((torch.from_numpy(g["train_weights"]) * 2.0 * ref["n_targets"][torch.from_numpy(ta)].float() * gate * ref["scale"]).sum() / Q)
    print(f"train=True loss {loss.item():.6f} vs oracle {ref['train_loss'].item():.6f} (bound {bound:.3e})")
    assert abs(loss.item() - ref["train_loss"].item()) <= bound


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_generate_vs_oracle_beam_search(small_med_json, dtype):
    """inference='generate' (unmasked cross-attention over all 35 question states, pad states included).

    (1) Teacher-forced along the ORACLE's own beam path: the shared one-token prompt pass and every one of the decode steps that
        follow — driven by the oracle's tokens and beam_idx, through the session the product builds (tiled cross K/V, shared
        prefill: the prompt's K/V in arena slot b * nb) — give logits within the plain gate of the oracle's at that step.  This
        is the independent check of steps 1 and later: a prompt K/V in the wrong arena slot, or a wrong ancestry, shows here.
    (2) The free-running device search equals oracle/beam_ref.py driven by the DEVICE's logits, token for token.
    (3) It equals the golden ids for every question whose candidate gaps in the oracle's search exceed gate x scale x 2 x
        steps.  On this fixture (small random weights: near-flat distributions) the oracle flags all four questions as
        near-ties, so (3) compares nothing here; (1) and (2) carry the check.  The count is printed."""
    from oracle import beam_ref
    from vidil_amd.blip import DecoderSession

    g, ref = vc.golden(), vc.reference()
    m = _model(small_med_json, dtype)
    gate = _gate(dtype)
    img, y16, ids, lens, h32, h16 = _states(m, g)
    Q, nb = 4, vc.NUM_BEAMS
    out_tok, out_len = m.generate_answer_ids(h16, Q)
    toks = out_tok.cpu().numpy()

    def run(sess, ids_, beam_idx):
        """one decoder call of a search on the device: logits f32 [Q * nb, V] on the host"""
        if beam_idx is None:       # the prompt pass, once per question (what _beam_search does); every beam of a question sees it
            lg = sess.prefill(torch.from_numpy(ids_[::nb].copy()).to(torch.int32).reshape(-1).to(DEV), ids_.shape[1], shared=True)
            return lg.cpu().repeat_interleave(nb, 0)
        return sess.step(torch.from_numpy(ids_[:, -1].copy()).to(torch.int32).to(DEV),
                         torch.from_numpy(beam_idx).to(torch.int32).to(DEV), ids_.shape[1] - 1).cpu()

    # (1) every call of the oracle's search, on the oracle's inputs
    calls, ref_logits = ref["gen_calls"], ref["gen_logits"]
    assert len(calls) == vc.MAX_LENGTH - 1 and calls[0][0].shape == (Q * nb, 1)
    scale = max(1.0, max(float(np.abs(l).max()) for l in ref_logits))
    sess = DecoderSession(m.text_decoder, h16, Q, nb, vc.MAX_LENGTH, tiled_cross=True)
    worst = []
    for s, (ids_, beam_idx) in enumerate(calls):
        lg = run(sess, ids_, beam_idx)
        live = torch.from_numpy(ids_[:, -1] != vc.PAD)          # (rows of a finished question carry [PAD]: nothing to compare)
        assert bool(live.any())
        worst.append((lg - torch.from_numpy(ref_logits[s]))[live].abs().max().item())
    print(f"\ngenerate {dtype}: max |d logits| per decoder call along the oracle's beam path "
          f"{' '.join(f'{w:.2e}' for w in worst)} (gate {gate * scale:.3e})")
    assert max(worst) <= gate * scale, worst
    # (2) the production search against the oracle's search on the device's own logits
    sess2 = DecoderSession(m.text_decoder, h16, Q, nb, vc.MAX_LENGTH, tiled_cross=True)
    seqs_dev, _ = beam_ref.beam_search(lambda i, b: run(sess2, i, b).numpy(), np.full((Q, 1), vc.DEC, dtype=np.int64), num_beams=nb,
                                       max_length=vc.MAX_LENGTH, min_length=vc.MIN_LENGTH, eos_token_id=vc.SEP, pad_token_id=vc.PAD)
    for b in range(Q):
        assert np.array_equal(toks[b][:len(seqs_dev[b])], seqs_dev[b]), (b, toks[b], seqs_dev[b])
    # (3) the golden ids, outside the near-ties the oracle flags
    margin = gate * scale * 2.0 * (vc.MAX_LENGTH - 1)
    decided = [b for b in range(Q) if ref["gen_gap"][b] > margin]
    print(f"generate {dtype}: {Q - len(decided)} of {Q} questions have a candidate gap below {margin:.3e} in the oracle's search "
          f"(flagged near-ties); {len(decided)} compared with the golden ids")
    for b in decided:
        assert np.array_equal(toks[b], g["gen_ids"][b]), b
    answers = m(img, vc.questions(g), train=False, inference="generate")
    assert isinstance(answers, list) and len(answers) == Q and all(isinstance(a, str) for a in answers)
    assert answers == [m.tokenizer.decode(r, skip_special_tokens=True) for r in toks.tolist()]


def test_rank_of_a_question_does_not_depend_on_its_batch_bit_for_bit(small_med_json):
    """Every question alone (its ids padded to the batch's 35 tokens) and in the batch of four: identical question states,
    first-token log-probabilities, top-k ids, log_probs_sum and max_ids."""
    g = vc.golden()
    m = _model(small_med_json)
    img, y16, ids, lens, h32, h16 = _states(m, g)
    a_ids, a_lens = m.tokenize_answers(vc.answers(g))
    k, Tq, Te = int(g["k"]), ids.shape[1], 17
    lp4 = m.first_token_logprobs(h16, 4, lens, a_ids)
    max4, top4, sum4 = m.rank_answer(h16, 4, lens, a_ids, a_lens, k)
    for q in range(4):
        _, s1 = m.question_states(y16[q * Te:(q + 1) * Te], 1, ids[q:q + 1], lens[q:q + 1])
        assert torch.equal(s1, h16[q * Tq:(q + 1) * Tq]), q
        assert torch.equal(m.first_token_logprobs(s1, 1, lens[q:q + 1], a_ids)[0], lp4[q]), q
        max1, top1, sum1 = m.rank_answer(s1, 1, lens[q:q + 1], a_ids, a_lens, k)
        assert torch.equal(top1[0], top4[q]) and torch.equal(sum1[0], sum4[q]) and int(max1[0]) == int(max4[q]), q


def test_refusals(small_med_json):
    from vidil_amd import kernels as K
    from vidil_amd.med import CrossRoute, parity_layers
    from vidil_amd.packing import set_compute_dtype, set_parity_mode

    g = vc.golden()
    m = _model(small_med_json)
    img = torch.zeros(4, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="k_test"):
        m(img, vc.questions(g), vc.answers(g), train=False, inference="rank", k_test=41)
    with pytest.raises(ValueError, match="inference"):
        m(img, vc.questions(g), vc.answers(g), train=False, inference="sample")
    with pytest.raises(ValueError, match="parity"):
        set_parity_mode(True, m)
    with pytest.raises(ValueError, match="fp8"):
        set_compute_dtype("fp8", m)
    set_parity_mode(True, m.text_decoder)
    try:
        with pytest.raises(ValueError, match="parity"):
            m(img, vc.questions(g), vc.answers(g), train=False, inference="rank", k_test=8)
        # the stack itself refuses a masked cross-attention in the parity mode
        dec = m.text_decoder
        with pytest.raises(K.VidilHipError, match="cross_kv_len"):
            route = CrossRoute(dec.bert, None, 1, kv_len=torch.ones(1, dtype=torch.int32, device=DEV))
            parity_layers(dec.bert, dec.bert.packed(), None, None, rows=1, T=1, causal=True, kv_len=None, route=route)
    finally:
        set_parity_mode(False, m.text_decoder)
    assert int(m(img, vc.questions(g), vc.answers(g), train=False, inference="rank", k_test=8)[0]) == int(g["max_ids"][0])
