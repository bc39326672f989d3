"""Teacher-forced caption scoring on the GPU: the one-pass reduction kernel through the C ABI against float64, the decoder
path (BertLMHeadModel.score, BLIP_Decoder.caption_nll / forward) against the oracle composed in
caption_scoring_cases.py, batch independence and blocking bit for bit, the beam search's reported score recomputed
teacher-forced, and capfilt.score_captions."""
import json
import types

import numpy as np
import pytest
import torch

import caption_scoring_cases as cs
from common import fullsize_captioner_state, load_into
from test_models_gpu import PLAIN_F16_REL, _small_med_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLAIN_BF16_REL = 1e-2          # the bf16 caption-logit gate of tests/test_bf16_gpu.py (max|d logit| <= 1e-2 x logit scale)

# ============================================================================ the reduction kernel, through the C ABI
KERNEL_SHAPES = [(1, 7), (3, 64), (5, 512), (70, 30524), (2, 38401)]


def _kernel_case(R, V):
    """Rows with standard deviation 1 (even rows) and 20 (odd rows); with five rows or more: an all-equal row, a row that is
    -inf everywhere but three positions, a row whose maximum occurs twice.  Labels hold 0, V-1 and -100 (ignored)."""
    g = torch.Generator().manual_seed(1000 * R + V)
    x = torch.randn(R, V, generator=g) * torch.where(torch.arange(R) % 2 == 0, 1.0, 20.0)[:, None]
    lab = torch.randint(0, V, (R,), generator=g, dtype=torch.int64)
    lab[0] = 0
    if R > 1:
        lab[1] = V - 1
    tie = None
    if R >= 5:
        x[2] = 3.25
        keep = torch.tensor([1, V // 2, V - 2])
        row = torch.full((V,), float("-inf"))
        row[keep] = x[3][keep]
        x[3] = row
        lab[3] = V // 2
        hi = x[4].max().item() + 1.0
        tie = (V // 3, V - 5)
        x[4][tie[0]] = hi
        x[4][tie[1]] = hi
    elif R == 2:
        hi = x[1].max().item() + 1.0
        tie = (5, V - 1)
        x[1][5] = hi
        x[1][V - 1] = hi
    ignored = [R - 1] if R >= 3 else []
    if R > 5:
        ignored.append(5)
    for r in ignored:
        lab[r] = -100
    return x, lab, tie


@pytest.fixture(scope="module")
def kernel_cases():
    """Inputs of every shape, their float64 log-softmax, and the largest error of torch's own f32 log_softmax on the CPU
    against it over ALL of them (finite entries) — the yardstick the kernel gets 4x of."""
    cases, torch_err = {}, 0.0
    for R, V in KERNEL_SHAPES:
        x, lab, tie = _kernel_case(R, V)
        lp64 = torch.log_softmax(x.double(), -1)
        lp32 = torch.log_softmax(x, -1).double()
        fin = torch.isfinite(lp64)
        torch_err = max(torch_err, (lp32 - lp64)[fin].abs().max().item())
        cases[(R, V)] = (x, lab, tie, lp64)
    return cases, torch_err


@pytest.mark.parametrize("R,V", KERNEL_SHAPES)
def test_teacher_forced_kernel_vs_float64_log_softmax(kernel_cases, R, V):
    """vidil_logsoftmax_topk_penalty(num_beams=0) returns VIDIL_OK (VIDIL_EUNSUP / EINVAL before this form existed) and its
    lp[label], mean_j lp[j] and argmax equal float64 log_softmax of the same f32 logits within 4x the error of torch's own f32
    log_softmax on the CPU over these inputs; argmax exactly (lowest index on ties); ignored rows exactly 0 with argmax written.
    Measured on an MI355X: torch f32 vs f64 1.514e-05 over these inputs, the kernel's worst |error| 6.429e-06 (0.42x; per shape
    1.5e-07, 2.9e-06, 3.5e-06, 6.4e-06, 3.5e-06)."""
    from vidil_amd import _lib

    cases, torch_err = kernel_cases
    x, lab, tie, lp64 = cases[(R, V)]
    lib = _lib.load()
    ld = 3                                                     # labels in column 0 of a wider table: ld_seqs > 1
    table = torch.full((R, ld), 7, dtype=torch.int32)
    table[:, 0] = lab.to(torch.int32)
    d_x, d_tab = x.to(DEV), table.to(DEV)
    out_s = torch.full((R, 2), 123.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    rc = lib.vidil_logsoftmax_topk_penalty(d_x.data_ptr(), None, R, 0, 0, V, -1, d_tab.data_ptr(), 0, ld, 1.0, out_s.data_ptr(),
                                           out_i.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.vidil_last_error()
    torch.cuda.synchronize()
    got_s, got_i = out_s.cpu().double(), out_i.cpu().long()
    tol = 4.0 * torch_err
    worst = 0.0
    for r in range(R):
        assert got_i[r].item() == int((x[r] == x[r].max()).nonzero()[0]), (r, "lowest index among equal maxima")
        if lab[r] < 0:
            assert got_s[r, 0].item() == 0.0 and got_s[r, 1].item() == 0.0, r
            continue
        ref_lp, ref_mean = lp64[r, lab[r]].item(), lp64[r].mean().item()
        assert np.isfinite(got_s[r, 0].item()), r
        worst = max(worst, abs(got_s[r, 0].item() - ref_lp))
        if np.isfinite(ref_mean):
            worst = max(worst, abs(got_s[r, 1].item() - ref_mean))
        else:                                                  # -inf logits: probability 0, the mean log-probability is -inf
            assert got_s[r, 1].item() == ref_mean, r
    print(f"\ntoken_logprobs ({R} x {V}): torch f32 log_softmax vs f64 on these inputs {torch_err:.3e}; "
          f"kernel worst |error| {worst:.3e} = {worst / torch_err:.2f}x (allowed 4x)")
    assert worst <= tol, (worst, tol)
    if R >= 5:
        assert abs(got_s[2, 0].item() + np.log(V)) <= tol and abs(got_s[2, 1].item() + np.log(V)) <= tol   # all-equal: -log V
        assert got_i[2].item() == 0
    if tie is not None:
        assert got_i[4 if R >= 5 else 1].item() == tie[0]


def test_token_logprobs_wrapper_matches_the_abi_call():
    from vidil_amd import kernels as K

    x, lab, _ = _kernel_case(5, 512)
    lp, lpm, am = K.token_logprobs(x.to(DEV), lab.to(torch.int32).to(DEV))
    ref = torch.log_softmax(x.double(), -1)
    assert lp.shape == (5,) and lpm.shape == (5,) and am.dtype == torch.int32
    assert abs(lp[0].item() - ref[0, 0].item()) < 1e-4 and lp[4].item() == 0.0
    assert am.cpu().tolist() == [int((x[r] == x[r].max()).nonzero()[0]) for r in range(5)]


# ============================================================================ the decoder path, small geometry
def _decoder(dtype="f16"):
    from vidil_amd.med import BertLMHeadModel
    from vidil_amd.packing import set_compute_dtype

    sd, enc = cs.small_state()
    dec = load_into(BertLMHeadModel(_small_med_cfg()), sd, "text_decoder.").to(DEV)
    if dtype != "f16":
        set_compute_dtype(dtype, dec)
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    return dec, enc.to(DEV).to(tdt).contiguous()              # image tokens [3, 17, 256]


class _TokensViT(torch.nn.Module):
    """Stands in for the ViT: hands out the golden image tokens and counts how often it is entered."""

    def __init__(self, enc16):
        super().__init__()
        self.enc16, self.calls = enc16, 0
        self.patch_embed = types.SimpleNamespace(num_patches=enc16.shape[1] - 1)

    def forward_both(self, x):
        self.calls += 1
        e = self.enc16[:x.shape[0]]
        return e.float(), e.reshape(-1, e.shape[-1])


@pytest.fixture(scope="module")
def small_med_json(tmp_path_factory):
    c = _small_med_cfg()
    path = tmp_path_factory.mktemp("cfg") / "med_small.json"
    path.write_text(json.dumps({k: getattr(c, k) for k in ("hidden_size", "num_attention_heads", "intermediate_size",
                                                           "num_hidden_layers", "vocab_size", "max_position_embeddings")}))
    return str(path)


def _captioner(small_med_json, dtype="f16"):
    from vidil_amd.blip import BLIP_Decoder

    dec, enc16 = _decoder(dtype)
    cap = BLIP_Decoder(med_config=small_med_json, image_size=32, vit="base", tokenizer=cs.SmallTokenizer(), prompt=cs.PROMPT)
    assert cap.prompt_length == cs.PROMPT_LENGTH
    cap.text_decoder = dec
    cap.visual_encoder = _TokensViT(enc16)
    return cap, enc16


def _gate(dtype):
    scale = max(1.0, cs.reference()["logits"].abs().max().item())
    return (PLAIN_F16_REL if dtype == "f16" else PLAIN_BF16_REL) * scale


def _by_caption(res, p):
    i = res.tokens_of(p)
    return res.lp_label[i].clone(), res.lp_mean[i].clone(), res.argmax[i].clone()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_caption_nll_and_forward_vs_composed_oracle(small_med_json, dtype):
    """3 images, 7 captions through image_index (0, 2, 2, 1, 0, 2, 1) with prompt_length + 1, 6, 9, 17, 40, 55 (-> 40) and 12
    tokens: per-caption sums and counts ('none'), the scalar ('mean') and forward().  |d lse| <= max|d logit|, so lp[label]
    and mean lp each move by at most 2 max|d logit|: a caption with n targets is within 2 n g of the oracle and the mean
    within 2 g, g the plain-mode logit gate.  Measured worst ratio to the per-caption bound: f16 0.038, bf16 0.024."""
    cap, enc16 = _captioner(small_med_json, dtype)
    ref, g = cs.reference(), _gate(dtype)
    caps = cs.captions()
    nll, cnt = cap.caption_nll(enc16, caps, cs.IMAGE_INDEX, reduction="none")
    assert nll.dtype == torch.float32 and cnt.dtype == torch.int32 and nll.is_cuda
    assert cnt.cpu().tolist() == ref["counts"].tolist() == [min(n, 40) - cs.PROMPT_LENGTH for n in cs.TOKEN_COUNTS]
    d = (nll.cpu() - ref["none"]).abs()
    bound = 2.0 * ref["counts"].float() * g
    ratio = (d / bound).max().item()
    mean = cap.caption_nll(enc16, caps, cs.IMAGE_INDEX, reduction="mean")
    assert mean.dim() == 0 and mean.dtype == torch.float32 and mean.is_cuda
    r_mean = abs(mean.item() - ref["mean"].item()) / (2.0 * g)
    # forward: caption i describes image i (models/blip.py:104-125)
    pick = [1, 3, 6]
    assert [cs.IMAGE_INDEX[i] for i in pick] != [0, 1, 2]      # (so forward pairs them with OTHER images than the batch above)
    sd, enc = cs.small_state()
    ids3, mask3, lab3 = cs.reference_targets(cs.SmallTokenizer(), [caps[i] for i in pick], cs.PROMPT_LENGTH)
    ref_fwd = cs.oracle_loss(cs.oracle_logits(sd, enc, ids3, mask3, [0, 1, 2]), lab3, "mean")
    loss = cap(torch.zeros(3, 3, 32, 32, device=DEV), [caps[i] for i in pick])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and bool(torch.isfinite(loss))
    r_fwd = abs(loss.item() - ref_fwd.item()) / (2.0 * g)
    print(f"\ncaption_nll {dtype}: worst |d sum| / (2 n g) = {ratio:.3f}, |d mean| / (2 g) = {r_mean:.4f}, forward {r_fwd:.4f} (g = {g:.3e})")
    assert bool((d <= bound).all()), (d, bound)
    assert r_mean <= 1.0 and r_fwd <= 1.0
    # plain negative log-likelihood sums: label_smoothing = 0
    nll0, _ = cap.caption_nll(enc16, caps, cs.IMAGE_INDEX, label_smoothing=0.0, reduction="none")
    ref0 = cs.oracle_loss(ref["logits"], ref["labels"], "none", label_smoothing=0.0)
    assert bool(((nll0.cpu() - ref0).abs() <= bound).all())


def test_forward_returns_a_finite_scalar_and_no_target_scores_zero(small_med_json):
    """BLIP_Decoder.forward raised NotImplementedError before this feature.  A caption that truncates to no target token
    scores 0 with count 0, never NaN."""
    cap, enc16 = _captioner(small_med_json)
    loss = cap.forward(torch.zeros(1, 3, 32, 32, device=DEV), [cs.PROMPT + "w200"])
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and loss.item() > 0
    nll, cnt = cap.caption_nll(enc16, ["w7 w8", cs.PROMPT + "w200 w201"], [1, 1], reduction="none")
    assert cnt.cpu().tolist() == [0, 3] and nll[0].item() == 0.0 and bool(torch.isfinite(nll).all())
    alone, _ = cap.caption_nll(enc16, ["w7 w8"], [2], reduction="none")
    assert alone.item() == 0.0 and cap.caption_nll(enc16, ["w7 w8"], [2], reduction="mean").item() == 0.0


def test_image_major_groups_give_the_numbers_of_image_index():
    dec, enc16 = _decoder()
    ref = cs.reference()
    ids, lens = ref["ids"], ref["mask"].sum(1)
    flat = enc16.reshape(-1, 256)
    a = dec.score(flat, 3, ids, lens, image_index=cs.IMAGE_INDEX, prompt_length=cs.PROMPT_LENGTH)
    order = sorted(range(7), key=lambda p: (cs.IMAGE_INDEX[p], p))              # image-major: 0 4 | 3 6 | 1 2 5
    gs = [0, 2, 4, 7]
    b = dec.score(flat, 3, ids[order], lens[order], group_start=gs, max_group=3, prompt_length=cs.PROMPT_LENGTH)
    assert torch.equal(a.count[order], b.count)
    for j, p in enumerate(order):
        for x, y in zip(_by_caption(a, p), _by_caption(b, j)):
            assert torch.equal(x, y), (p, (x.float() - y.float()).abs().max().item())
    assert torch.equal(a.loss_sum[order], b.loss_sum)


def test_parity_mode_per_token_within_2e3_absolute():
    """packing.set_parity_mode: every target token's lp[label] and mean lp within 2e-3 absolute of the oracle (twice the
    project's 1e-3 absolute logit tolerance, by the argument above)."""
    from vidil_amd import kernels as K
    from vidil_amd.packing import set_parity_mode

    dec, _ = _decoder()
    _, enc = cs.small_state()
    set_parity_mode(True, dec)
    e32 = enc.reshape(-1, 256).to(DEV).contiguous()
    enc3 = K.split3(e32, torch.empty((e32.shape[0], 3 * 256), dtype=torch.float16, device=DEV))
    ref = cs.reference()
    res = dec.score(enc3, 3, ref["ids"], ref["mask"].sum(1), image_index=cs.IMAGE_INDEX, prompt_length=cs.PROMPT_LENGTH)
    c, t = res.caption.cpu(), res.position.cpu()
    lab = ref["ids"][c, t]
    lp_ref = ref["lp"][c, t - 1]                              # logits at t - 1 score the token at t
    d_lab = (res.lp_label.cpu().double() - lp_ref.gather(1, lab[:, None])[:, 0]).abs().max().item()
    d_mean = (res.lp_mean.cpu().double() - lp_ref.mean(1)).abs().max().item()
    print(f"\nparity mode: per-token max |d lp[label]| = {d_lab:.3e}, max |d mean lp| = {d_mean:.3e} (allowed 2e-3)")
    assert res.lp_label.numel() == int(ref["counts"].sum()) and d_lab <= 2e-3 and d_mean <= 2e-3


def test_a_captions_token_scores_do_not_depend_on_its_batch_bit_for_bit(monkeypatch):
    """Caption 3 (17 tokens) alone, in the batch of 7 (40-token block) and in that batch with the logits row block cut to 16
    rows: identical lp[label], mean lp and argmax per token."""
    from vidil_amd import med

    dec, enc16 = _decoder()
    ref = cs.reference()
    ids, lens = ref["ids"], ref["mask"].sum(1)
    flat = enc16.reshape(-1, 256)
    kw = dict(prompt_length=cs.PROMPT_LENGTH)
    batch = _by_caption(dec.score(flat, 3, ids, lens, image_index=cs.IMAGE_INDEX, **kw), 3)
    n3 = int(lens[3])
    alone = _by_caption(dec.score(flat, 3, ids[3:4, :n3], lens[3:4], image_index=[cs.IMAGE_INDEX[3]], **kw), 0)
    monkeypatch.setattr(med, "LOGITS_BLOCK_BYTES", 16 * 4 * cs.V)
    small = _by_caption(dec.score(flat, 3, ids, lens, image_index=cs.IMAGE_INDEX, **kw), 3)
    assert batch[0].numel() == n3 - cs.PROMPT_LENGTH
    for x, y, z in zip(batch, alone, small):
        assert torch.equal(x, y) and torch.equal(x, z), ((x.float() - y.float()).abs().max().item(), (x.float() - z.float()).abs().max().item())


@pytest.mark.parametrize("form", ["image_index", "group_start"])
def test_image_blocks_of_two_give_the_unblocked_bits(monkeypatch, form):
    from vidil_amd.med import BertModel

    dec, enc16 = _decoder()
    ref = cs.reference()
    ids, lens = ref["ids"], ref["mask"].sum(1)
    flat = enc16.reshape(-1, 256)
    if form == "image_index":
        kw = dict(image_index=cs.IMAGE_INDEX, prompt_length=cs.PROMPT_LENGTH)
    else:
        order = sorted(range(7), key=lambda p: (cs.IMAGE_INDEX[p], p))
        ids, lens = ids[order], lens[order]
        kw = dict(group_start=[0, 2, 4, 7], prompt_length=cs.PROMPT_LENGTH)
    whole = dec.score(flat, 3, ids, lens, **kw)
    monkeypatch.setattr(BertModel, "MAX_IMAGES_PER_LAUNCH", 2)
    blocks = dec.score(flat, 3, ids, lens, **kw)
    assert torch.equal(whole.loss_sum, blocks.loss_sum) and torch.equal(whole.count, blocks.count)
    for p in range(7):
        for x, y in zip(_by_caption(whole, p), _by_caption(blocks, p)):
            assert torch.equal(x, y), p


def test_score_captions_runs_the_vit_once_and_equals_per_pair_scores(small_med_json):
    from vidil_amd.capfilt import score_captions

    cap, enc16 = _captioner(small_med_json)
    texts = ["w200 w201 w202", "w300", "w410 w411 w412 w413 w414 w415 w416"]
    images = torch.zeros(2, 3, 32, 32, device=DEV)
    m = score_captions(cap, images, texts)
    assert cap.visual_encoder.calls == 1 and tuple(m.shape) == (3, 2) and m.dtype == torch.float32
    for c, t in enumerate(texts):
        for f in range(2):
            nll, cnt = cap.caption_nll(enc16, [t], [f], add_prompt=True, label_smoothing=0.0, reduction="none")
            assert cnt.item() == len(t.split()) + 1
            assert abs(m[c, f].item() - nll.item() / cnt.item()) <= 1e-6 * abs(m[c, f].item()), (c, f)


# ============================================================================ closing the loop with the beam search
def test_beam_search_scores_are_reproduced_teacher_forced():
    """Full size (12 layers, V = 30,524), 4 synthetic frames, num_beams=3, max_length=20, min_length=5: the winning
    hypothesis' reported score sum_logprob / len (len counts the 4 prompt tokens, not the [SEP]) equals -nll_sum / len of its
    tokens rescored in ONE causal pass (label_smoothing = 0; the final [SEP] is a target when the hypothesis ended on it) within
    2 n g / len, and the scoring pass' argmax at every position is the token the incremental pass' logits pick greedily.
    Measured worst ratio to the bound: 0.011 (all four hypotheses run to max_length on these weights)."""
    from vidil_amd.blip import BLIP_Decoder, DecodeTrace
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    sd, _ = fullsize_captioner_state()
    tok = SyntheticBertTokenizer()
    cap = BLIP_Decoder(image_size=224, vit="base", tokenizer=tok)
    cap.load_state_dict(sd)
    cap = cap.to(DEV).eval()
    B, nb, max_len, P, V = 4, 3, 20, 4, 30524
    x = torch.from_numpy(np.random.default_rng(77).standard_normal((B, 3, 224, 224), dtype=np.float32)).to(DEV)
    _, y16 = cap.visual_encoder.forward_both(x)
    trace = DecodeTrace()
    out_tok, out_len = cap.generate_ids(y16, B, num_beams=nb, max_length=max_len, min_length=5, trace=trace)
    out_tok, out_len, reported = out_tok.cpu().tolist(), out_len.cpu().tolist(), trace.scores.cpu()
    eos = tok.sep_token_id
    # replay the beams from the traced candidates: which row of which step's logits saw which prefix
    prompt = out_tok[0][:P]
    seqs = [[list(prompt) for _ in range(nb)] for _ in range(B)]
    row_of = {(b, tuple(prompt)): (0, b) for b in range(B)}
    for s, ci in enumerate(trace.cand_index):
        ci = ci.cpu().tolist()
        for b in range(B):
            new = []
            for flat in ci[b]:
                beam, t = divmod(flat, V)
                if t != eos and len(new) < nb and beam < len(seqs[b]):
                    new.append(seqs[b][beam] + [t])
            seqs[b] = new
            for j, q in enumerate(new):
                row_of.setdefault((b, tuple(q)), (s + 1, b * nb + j))
    hyps = [out_tok[b][:out_len[b]] + ([eos] if out_len[b] < max_len else []) for b in range(B)]
    lens = torch.tensor([len(h) for h in hyps])
    ids = torch.zeros((B, int(lens.max())), dtype=torch.long)
    for b, h in enumerate(hyps):
        ids[b, :len(h)] = torch.tensor(h)
    res = cap.text_decoder.score(y16, B, ids, lens, label_smoothing=0.0, prompt_length=P)
    scale = max(1.0, max(l.abs().max().item() for l in trace.logits))
    g = PLAIN_F16_REL * scale
    worst = 0.0
    for b in range(B):
        n, ln = int(res.count[b]), out_len[b]
        assert n == len(hyps[b]) - P
        got = -res.loss_sum[b].item() / ln
        bound = 2.0 * n * g / ln
        worst = max(worst, abs(got - reported[b].item()) / bound)
        assert abs(got - reported[b].item()) <= bound, (b, got, reported[b].item(), bound)
        am = res.argmax[res.tokens_of(b)].cpu().tolist()
        for t in range(P, len(hyps[b])):
            s, row = row_of[(b, tuple(hyps[b][:t]))]
            assert s == t - P
            assert am[t - P] == int(trace.logits[s][row].argmax()), (b, t)
    print(f"\nbeam score vs teacher-forced rescoring: worst |d| / (2 n g / len) = {worst:.3f} (g = {g:.3e}, lengths {out_len})")
