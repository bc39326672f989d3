"""Video question answering on the GPU (vidil_amd/blip_vqa.py: BLIP_Video_VQA; vidil_amd/video_qa.py) against the oracle composed
in tests/video_vqa_cases.py, in f16 and bf16: three videos of 776 / 68 / 1,154 keys, seven questions of at most 12 tokens in a
shuffled order (1 / 4 / 2 per video).  The gates are tests/test_vqa_gpu.py's: a softmax average does not get less accurate
with more keys (the argument of tests/test_attention_long_gpu.py)."""
import types

import numpy as np
import pytest
import torch

import video_vqa_cases as C
import vqa_cases as vc
from test_vqa_gpu import _decoder, _encoder, _gate, small_med_json  # noqa: F401  (small_med_json: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE = 32                          # the stub ViT reads a frame's first pixel only
VOQ = torch.tensor(C.VIDEO_OF_QUESTION)
CASE_NAMES = sorted(C.CASES)


class _FramesViT(torch.nn.Module):
    """Stands in for the ViT: a frame's first pixel holds its row in the token table [frames, T, C]; counts its calls."""

    def __init__(self, table16):
        super().__init__()
        self.table16, self.calls = table16, 0
        self.patch_embed = types.SimpleNamespace(num_patches=table16.shape[1] - 1)

    def forward_both(self, x):
        self.calls += 1
        e = self.table16[x[:, 0, 0, 0].round().long()].contiguous()
        return e.float(), e.reshape(-1, e.shape[-1])


def _videos(V, N):
    v = torch.zeros(V, N, 3, SIZE, SIZE)
    v[:, :, 0, 0, 0] = torch.arange(V * N, dtype=torch.float32).view(V, N)
    return v


_MODELS = {}


def _model(med_json, case, dtype, video_tokens=None, key=None):
    """A BLIP_Video_VQA of the small geometry whose ViT hands out ``video_tokens`` f32 [V, N*T, C] (default: the case's)."""
    from vidil_amd.blip_vqa import BLIP_Video_VQA
    from vidil_amd.packing import set_compute_dtype

    key = (case, dtype, key)
    if key not in _MODELS:
        N, T = C.CASES[case]
        tok = C.tokens(case) if video_tokens is None else video_tokens
        m = BLIP_Video_VQA(med_config=med_json, image_size=SIZE, vit="base", tokenizer=vc.VqaTokenizer())
        m.text_encoder, m.text_decoder = _encoder(), _decoder()
        tdt = torch.float16 if dtype == "f16" else torch.bfloat16
        m.visual_encoder = _FramesViT(tok.view(-1, T, C.WIDTH).to(DEV).to(tdt).contiguous())
        set_compute_dtype(dtype, m)
        _MODELS[key] = m
    return _MODELS[key]


_RUNS = {}


def _run(med_json, case, dtype):
    """The grouped path once per (case, dtype), shared by the tests: tokens, question states, the ranking."""
    if (case, dtype) not in _RUNS:
        m = _model(med_json, case, dtype)
        N, T = C.CASES[case]
        video = _videos(C.B, N).to(DEV)
        tok16 = m.video_tokens(video)
        ids, lens = m.tokenize_questions(C.questions(case))
        h32, h16 = m.question_states_grouped(tok16, C.B, ids, lens, VOQ)
        g = vc.golden()
        a_ids, a_lens = m.tokenize_answers(vc.answers(g))
        max_ids, topk_ids, sums = m.rank_answer(h16, C.Q, lens, a_ids, a_lens, int(g["k"]))
        _RUNS[(case, dtype)] = types.SimpleNamespace(m=m, video=video, tok16=tok16, ids=ids, lens=lens, h32=h32, h16=h16, a_ids=a_ids,
                                                     a_lens=a_lens, max_ids=max_ids, topk_ids=topk_ids, sums=sums, k=int(g["k"]),
                                                     answers=vc.answers(g))
    return _RUNS[(case, dtype)]


def _check_ranking(ref, gate, topk_ids, max_ids, sums, ex):
    """test_vqa_gpu.test_rank_and_loss_vs_composed_oracle's comparison of a ranking with the oracle's, question by question."""
    k = ref["k"]
    unit = 2.0 * gate * ref["scale"]
    for q in range(C.Q):
        if bool(ex[q]):
            continue
        mine, want = topk_ids[q].cpu().tolist(), ref["topk_ids"][q].tolist()
        assert sorted(mine) == sorted(want), q
        srt = ref["lp64"][q].sort(descending=True).values
        for r in range(k):
            if (r == 0 or srt[r - 1] - srt[r] > unit) and srt[r] - srt[r + 1] > unit:
                assert mine[r] == want[r], (q, r)
        assert int(max_ids[q]) == int(ref["max_ids"][q]), q
        by_id = dict(zip(want, ref["log_probs_sum"][q].tolist()))
        for j, a in enumerate(mine):
            assert abs(sums[q, j].item() - by_id[a]) <= 2.0 * float(ref["n_targets"][a]) * gate * ref["scale"], (q, a)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_states_rank_and_loss_vs_composed_oracle(small_med_json, case, dtype):  # noqa: F811
    """Question states (returned in the caller's order) and first-token logits within the plain gates (1.25e-3 x scale f16,
    1e-2 x scale bf16), first-token log-probabilities within twice that; topk_ids, max_ids and log_probs_sum against the oracle's
    for every question the oracle decides by more than gate x scale x 2 x target tokens (none excluded for f16, at most one of
    seven for bf16: tests/test_video_vqa_cpu.py); the train=True loss within gate x target count of its answers."""
    ref, r = C.reference(case), _run(small_med_json, case, dtype)
    m, gate = r.m, _gate(dtype)
    assert tuple(r.tok16.shape) == (C.B * C.CASES[case][0] * C.CASES[case][1], C.WIDTH)
    assert torch.equal(r.tok16.float().cpu().view(C.B, -1, C.WIDTH), C.tokens(case))         # a video's N*T rows are contiguous
    qs = ref["question_states"].reshape(-1, C.WIDTH)
    s_scale = max(1.0, qs.abs().max().item())
    e_states = (r.h32.cpu() - qs).abs().max().item()
    assert tuple(r.h16.shape) == (C.Q * 12, C.WIDTH) and (r.h16.float() - r.h32).abs().max().item() <= 2.0 ** -8 * s_scale
    logits = m.text_decoder.start_logits(r.h16, C.Q, vc.DEC, cross_kv_len=r.lens)
    l_scale = max(1.0, ref["first_logits"].abs().max().item())
    e_logits = (logits.cpu() - ref["first_logits"]).abs().max().item()
    lp = m.first_token_logprobs(r.h16, C.Q, r.lens, r.a_ids)
    e_lp = (lp.cpu().double() - ref["lp64"]).abs().max().item()
    ex = C.excluded(case, gate)
    print(f"\nBLIP_Video_VQA {case} {dtype}: |d states| {e_states:.3e} (gate {gate * s_scale:.3e}), |d first logits| {e_logits:.3e} "
          f"(gate {gate * l_scale:.3e}), |d first-token lp| {e_lp:.3e}; excluded by the oracle's own margins: {int(ex.sum())} of {C.Q}")
    assert e_states <= gate * s_scale and e_logits <= gate * l_scale and e_lp <= 2.0 * gate * l_scale
    assert int(ex.sum()) <= 1 and (dtype != "f16" or int(ex.sum()) == 0)
    _check_ranking(ref, gate, r.topk_ids, r.max_ids, r.sums, ex)
    # train=True on the grouped states (models/blip_vqa.py:208-244)
    ta, tw = C.train_inputs(case)
    losses = m.answer_loss(r.h16, C.Q, r.lens, r.a_ids[ta], r.a_lens[ta], C.N_TRAIN)
    loss = float((tw.double() * losses.cpu().double()).sum() / C.Q)
    bound = float((tw * 2.0 * ref["n_targets"][ta].float() * gate * ref["scale"]).sum() / C.Q)
    print(f"train=True loss {loss:.6f} vs oracle {ref['train_loss'].item():.6f} (bound {bound:.3e})")
    assert abs(loss - ref["train_loss"].item()) <= bound


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_generate_vs_oracle_beam_search(small_med_json, case, dtype):  # noqa: F811
    """test_vqa_gpu.test_generate_vs_oracle_beam_search on the grouped question states: (1) every decoder call of the oracle's
    search, on the oracle's tokens and beam_idx, within the plain gate; (2) the device search equals oracle/beam_ref.py driven
    by the device's logits; (3) the oracle's ids where its candidate gaps exceed gate x scale x 2 x steps (count printed)."""
    from oracle import beam_ref
    from vidil_amd.blip import DecoderSession

    ref, r = C.reference(case), _run(small_med_json, case, dtype)
    m, gate = r.m, _gate(dtype)
    Q, nb = C.Q, vc.NUM_BEAMS
    out_tok, _ = m.generate_answer_ids(r.h16, Q)
    toks = out_tok.cpu().numpy()

    def run(sess, ids_, beam_idx):
        if beam_idx is None:
            lg = sess.prefill(torch.from_numpy(ids_[::nb].copy()).to(torch.int32).reshape(-1).to(DEV), ids_.shape[1], shared=True)
            return lg.cpu().repeat_interleave(nb, 0)
        return sess.step(torch.from_numpy(ids_[:, -1].copy()).to(torch.int32).to(DEV),
                         torch.from_numpy(beam_idx).to(torch.int32).to(DEV), ids_.shape[1] - 1).cpu()

    calls, ref_logits = ref["gen_calls"], ref["gen_logits"]
    assert len(calls) == vc.MAX_LENGTH - 1 and calls[0][0].shape == (Q * nb, 1)
    scale = max(1.0, max(float(np.abs(l).max()) for l in ref_logits))
    sess = DecoderSession(m.text_decoder, r.h16, Q, nb, vc.MAX_LENGTH, tiled_cross=True)
    worst = []
    for s, (ids_, beam_idx) in enumerate(calls):
        lg = run(sess, ids_, beam_idx)
        live = torch.from_numpy(ids_[:, -1] != vc.PAD)
        assert bool(live.any())
        worst.append((lg - torch.from_numpy(ref_logits[s]))[live].abs().max().item())
    print(f"\ngenerate {case} {dtype}: max |d logits| per decoder call along the oracle's beam path "
          f"{' '.join(f'{w:.2e}' for w in worst)} (gate {gate * scale:.3e})")
    assert max(worst) <= gate * scale, worst
    sess2 = DecoderSession(m.text_decoder, r.h16, Q, nb, vc.MAX_LENGTH, tiled_cross=True)
    seqs_dev, _ = beam_ref.beam_search(lambda i, b: run(sess2, i, b).numpy(), np.full((Q, 1), vc.DEC, dtype=np.int64), num_beams=nb,
                                       max_length=vc.MAX_LENGTH, min_length=vc.MIN_LENGTH, eos_token_id=vc.SEP, pad_token_id=vc.PAD)
    for b in range(Q):
        assert np.array_equal(toks[b][:len(seqs_dev[b])], seqs_dev[b]), (b, toks[b], seqs_dev[b])
    margin = gate * scale * 2.0 * (vc.MAX_LENGTH - 1)
    decided = [b for b in range(Q) if ref["gen_gap"][b] > margin]
    print(f"generate {case} {dtype}: {len(decided)} of {Q} questions have every candidate gap above {margin:.3e} in the oracle's "
          f"search and are compared with its ids")
    for b in decided:
        assert np.array_equal(toks[b], ref["gen_ids"][b]), b


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_drop_in_forward_equals_the_grouped_path(small_med_json, case, dtype):  # noqa: F811
    """forward(video [7, N, 3, S, S], question [7]) — the reference's call, every question alone with (a copy of) its video: 12
    query rows over 776 / 1,154 keys per unit — in rank, generate and train.  Same answer ids as the grouped path, log_probs_sum
    within the gate of its — and, what the launch forms promise beyond that, the same bits; the loss within the oracle's bound."""
    ref, r = C.reference(case), _run(small_med_json, case, dtype)
    m, gate = r.m, _gate(dtype)
    pairs = r.video[VOQ.to(DEV)].contiguous()
    qs = C.questions(case)
    out = m(pairs, qs, r.answers, train=False, inference="rank", k_test=r.k)
    assert out.dtype == torch.int64 and out.is_cuda and tuple(out.shape) == (C.Q,)
    tok_obj = types.SimpleNamespace(input_ids=r.a_ids.to(DEV), attention_mask=torch.from_numpy(vc.golden()["a_mask"]).to(DEV))
    assert torch.equal(m(pairs, qs, tok_obj, train=False, inference="rank", k_test=r.k), out)
    _, s16 = m.question_states_grouped(m.video_tokens(pairs), C.Q, r.ids, r.lens, torch.arange(C.Q))
    max1, top1, sum1 = m.rank_answer(s16, C.Q, r.lens, r.a_ids, r.a_lens, r.k)
    assert torch.equal(out, max1)
    # every pair alone with a copy of its video has the bits it has where the video is shared
    assert torch.equal(s16, r.h16) and torch.equal(top1, r.topk_ids) and torch.equal(sum1, r.sums)
    ex = C.excluded(case, gate)
    worst = 0.0
    for q in range(C.Q):
        mine = dict(zip(top1[q].cpu().tolist(), sum1[q].cpu().tolist()))
        for a, s in zip(r.topk_ids[q].cpu().tolist(), r.sums[q].cpu().tolist()):
            if a in mine:
                worst = max(worst, abs(mine[a] - s) / (2.0 * float(ref["n_targets"][a]) * gate * ref["scale"]))
        if not bool(ex[q]):
            assert int(out[q]) == int(r.max_ids[q]) and sorted(mine) == sorted(r.topk_ids[q].cpu().tolist()), q
    print(f"\ndrop-in {case} {dtype}: worst |d log_probs_sum| vs the grouped path {worst:.3f} of the gate")
    assert worst <= 1.0
    answers = m(pairs, qs, train=False, inference="generate")
    assert isinstance(answers, list) and len(answers) == C.Q and all(isinstance(a, str) for a in answers)
    assert answers == [m.tokenizer.decode(row, skip_special_tokens=True) for row in m.generate_answer_ids(s16, C.Q)[0].cpu().tolist()]
    ta, tw = C.train_inputs(case)
    loss = m(pairs, qs, [r.answers[i] for i in ta.tolist()], n=C.N_TRAIN, weights=tw)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    bound = float((tw * 2.0 * ref["n_targets"][ta].float() * gate * ref["scale"]).sum() / C.Q)
    assert abs(loss.item() - ref["train_loss"].item()) <= bound, (loss.item(), ref["train_loss"].item(), bound)


def _evaluate(r, case, order=None, **kw):
    from vidil_amd import video_qa as VQ

    order = list(range(C.Q)) if order is None else order
    qs = C.questions(case)
    det = {}
    res = VQ.evaluation(r.m, kw.pop("videos", r.video), [qs[i] for i in order], [100 + i for i in order], VOQ[order],
                        answer_list=r.answers, k_test=r.k, details=det, **kw)
    return res, det


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_results_do_not_depend_on_blocks_group_or_order(small_med_json, case, dtype):  # noqa: F811
    """evaluation with videos_per_block = 1 and with all videos in one block: identical answers, bit-identical log_probs_sum —
    and the bits of the grouped path called directly.  A question alone with its video (its ids padded to the call's 12
    tokens): the bits it has inside its group of four.  Another caller order permutes the result and nothing else."""
    r = _run(small_med_json, case, dtype)
    m = r.m
    res1, det1 = _evaluate(r, case, videos_per_block=1)
    res3, det3 = _evaluate(r, case, videos_per_block=C.B)
    assert res1 == res3 and [x["question_id"] for x in res1] == [100 + i for i in range(C.Q)]
    assert [x["answer"] for x in res1] == [r.answers[int(a)] for a in r.max_ids]
    for name in ("max_ids", "topk_ids", "log_probs_sum"):
        assert torch.equal(det1[name], det3[name]), name
    assert torch.equal(det1["log_probs_sum"], r.sums.cpu()) and torch.equal(det1["topk_ids"], r.topk_ids.cpu())
    # alone with its video
    for q in (0, 4, 3):                                            # two of video 1's group of four; the one question of video 0
        _, s1 = m.question_states_grouped(r.tok16, C.B, r.ids[q:q + 1], r.lens[q:q + 1], VOQ[q:q + 1])
        assert torch.equal(s1, r.h16[q * 12:(q + 1) * 12]), q
        max1, top1, sum1 = m.rank_answer(s1, 1, r.lens[q:q + 1], r.a_ids, r.a_lens, r.k)
        assert torch.equal(top1[0], r.topk_ids[q]) and torch.equal(sum1[0], r.sums[q]) and int(max1[0]) == int(r.max_ids[q]), q
    # another caller order
    perm = [5, 2, 6, 0, 3, 1, 4]
    resp, detp = _evaluate(r, case, order=perm)
    assert resp == [res1[i] for i in perm]
    for name in ("max_ids", "topk_ids", "log_probs_sum"):
        assert torch.equal(detp[name], det1[name][perm]), name
    gen1, gd1 = _evaluate(r, case, inference="generate", videos_per_block=1)
    genp, gdp = _evaluate(r, case, order=perm, inference="generate")
    assert genp == [gen1[i] for i in perm] and torch.equal(gdp["tokens"], gd1["tokens"][perm])
    assert torch.equal(gd1["tokens"], m.generate_answer_ids(r.h16, C.Q)[0].cpu())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_a_video_without_a_question_is_an_empty_group(small_med_json, dtype):  # noqa: F811
    """Four videos of 776 keys, the third without a question (group_start [0, 1, 5, 5, 7]): every question has the bits it has
    among the three videos of case a, in one block and in blocks of one video."""
    r = _run(small_med_json, "a", dtype)
    tok = C.tokens("a")
    four = torch.cat([tok[:2], tok[:1].flip(1), tok[2:]], 0)
    m4 = _model(small_med_json, "a", dtype, video_tokens=four, key="four")
    N = C.CASES["a"][0]
    voq4 = torch.tensor([v if v < 2 else 3 for v in C.VIDEO_OF_QUESTION])
    tok16 = m4.video_tokens(_videos(4, N).to(DEV))
    for vpb in (4, 1):
        h32, h16 = m4.question_states_grouped(tok16, 4, r.ids, r.lens, voq4, videos_per_block=vpb)
        assert torch.equal(h16, r.h16) and torch.equal(h32, r.h32), vpb


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_single_frame_is_the_image_model_on_the_middle_frame(small_med_json, case, dtype):  # noqa: F811
    """video_representation='single_frame' (train_vqa_video.py:83-86): frame int(N/2) alone.  The answers of BLIP_VQA's own
    question_states (one image per question, its launch forms) and rank_answer on that frame's tokens."""
    from vidil_amd.blip_vqa import BLIP_VQA

    r = _run(small_med_json, case, dtype)
    m = r.m
    N, T = C.CASES[case]
    res, det = _evaluate(r, case, video_representation="single_frame")
    mid = r.tok16.view(C.B, N, T, C.WIDTH)[:, int(N / 2)]
    per_q = mid[VOQ.to(DEV)].reshape(-1, C.WIDTH).contiguous()
    _, s16 = BLIP_VQA.question_states(m, per_q, C.Q, r.ids, r.lens)
    max_ids = m.rank_answer(s16, C.Q, r.lens, r.a_ids, r.a_lens, r.k)[0]
    assert [x["answer"] for x in res] == [r.answers[int(a)] for a in max_ids]
    assert torch.equal(det["max_ids"], max_ids.cpu())
    assert not torch.equal(det["log_probs_sum"], r.sums.cpu())                       # (it is not the concat_frame result)


def test_launch_counts_follow_videos_not_questions(small_med_json, monkeypatch):  # noqa: F811
    """Case a: the ViT runs once per batch of videos, the cross K|V projection and the cross-attention launch layers x blocks
    times — not layers x questions."""
    from vidil_amd import kernels as K

    r = _run(small_med_json, "a", "f16")
    m = r.m
    L = m.text_encoder.config.num_hidden_layers
    counts = dict(kv=0, cross=0, self=0)
    gemm, attention = K.gemm, K.attention

    def gemm_shim(a, w, b=None, **kw):
        h = kw.get("heads")
        if h is not None and "k" in h and "vt" in h and h.get("part0") == 1:
            counts["kv"] += 1
            assert a.shape[0] % (C.CASES["a"][0] * C.CASES["a"][1]) == 0          # whole videos
        return gemm(a, w, b, **kw)

    def attention_shim(*a, **kw):
        counts["cross" if kw.get("group_start") is not None else "self"] += 1
        return attention(*a, **kw)

    monkeypatch.setattr(K, "gemm", gemm_shim)
    monkeypatch.setattr(K, "attention", attention_shim)
    for vpb, blocks in ((1, 3), (2, 2), (3, 1)):
        counts.update(kv=0, cross=0, self=0)
        _, h16 = m.question_states_grouped(r.tok16, C.B, r.ids, r.lens, VOQ, videos_per_block=vpb)
        assert counts == dict(kv=L * blocks, cross=L * blocks, self=L * blocks), (vpb, counts)
        assert torch.equal(h16, r.h16)
    monkeypatch.undo()
    m.visual_encoder.calls = 0
    _evaluate(r, "a", videos=[r.video[:2].cpu(), r.video[2:].cpu()])
    assert m.visual_encoder.calls == 2
    m.visual_encoder.calls = 0
    _evaluate(r, "a")                                              # one tensor of three videos: one ViT pass
    assert m.visual_encoder.calls == 1


def test_refusals(small_med_json):  # noqa: F811
    from vidil_amd import video_qa as VQ
    from vidil_amd.packing import set_compute_dtype, set_parity_mode

    r = _run(small_med_json, "b", "f16")
    m = r.m
    qs = C.questions("b")
    pairs = r.video[VOQ.to(DEV)].contiguous()
    with pytest.raises(ValueError, match="k_test"):
        m(pairs, qs, r.answers, train=False, inference="rank", k_test=41)
    with pytest.raises(ValueError, match="k_test=41"):
        VQ.evaluation(m, r.video, qs, list(range(C.Q)), VOQ, answer_list=r.answers, k_test=41)
    with pytest.raises(ValueError, match="inference"):
        m(pairs, qs, r.answers, train=False, inference="sample")
    with pytest.raises(ValueError, match="6 questions for 7 videos"):
        m(pairs, qs[:6], r.answers, train=False, inference="rank", k_test=8)
    with pytest.raises(ValueError, match="7 questions, 7 lengths and 6 entries"):
        m.question_states_grouped(r.tok16, C.B, r.ids, r.lens, VOQ[:6])
    with pytest.raises(ValueError, match="7 questions, 7 question_ids and 6 entries"):
        VQ.evaluation(m, r.video, qs, list(range(C.Q)), VOQ[:6], answer_list=r.answers, k_test=8)
    with pytest.raises(ValueError, match="video_of_question"):
        m.question_states_grouped(r.tok16, C.B, r.ids, r.lens, VOQ + 1)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        m.question_states_grouped(torch.zeros(16385, C.WIDTH, dtype=torch.float16, device=DEV), 1, r.ids[:1], r.lens[:1], [0])
    with pytest.raises(ValueError, match="parity"):
        set_parity_mode(True, m)
    with pytest.raises(ValueError, match="fp8"):
        set_compute_dtype("fp8", m)
    set_parity_mode(True, m.text_encoder)
    try:
        with pytest.raises(ValueError, match="parity"):
            m(pairs, qs, r.answers, train=False, inference="rank", k_test=8)
        with pytest.raises(ValueError, match="parity"):
            m.question_states_grouped(r.tok16, C.B, r.ids, r.lens, VOQ)
        with pytest.raises(ValueError, match="parity"):
            VQ.evaluation(m, r.video, qs, list(range(C.Q)), VOQ, answer_list=r.answers, k_test=8)
    finally:
        set_parity_mode(False, m.text_encoder)
    assert torch.equal(m.question_states_grouped(r.tok16, C.B, r.ids, r.lens, VOQ)[1], r.h16)
