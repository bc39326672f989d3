"""Shared inputs of the video question-answering tests and the reference value composed from the existing oracle
(vqa_cases.stack / decoder_logits / answer_loss, oracle/beam_ref.py) with ``enc = tokens.view(B, N*T, C)[video_of_question]``.

Small geometry of vqa_cases.py (width 256, 4 heads, 2 layers, vocabulary 512; the text encoder of med_itm_small.npz, the decoder
of med_decoder_small.npz, the 40 answers and k_test = 8 of vqa_small.npz).  Three videos of N frames x T tokens:

  a   N = 8, T = 97    776 keys: just past the 768-key boundary, 7 chunks of the long-key attention kernel
  b   N = 4, T = 17     68 keys: the kernels that serve up to 768 keys, through group_start
  c   N = 2, T = 577  1,154 keys: the shape the reference's own comment names (models/blip_vqa.py:201)

Seven questions in a shuffled caller order, 1 / 4 / 2 of them per video, 3 - 12 tokens long ([ENC] and [SEP] included), so
Tq = 12 <= 32: the one-question video presents 12 query rows over its keys.  Video tokens are seeded normal numbers rounded
to bf16 (exact in f16 too), so the device's 16-bit copy of them IS the oracle's input; the seeds are chosen so that the
oracle's own ranking decisions are safe at both gates (tests/test_video_vqa_cpu.py pins that)."""
import numpy as np
import torch

import vqa_cases as vc
from oracle import beam_ref

WIDTH = 256
CASES = {"a": (8, 97), "b": (4, 17), "c": (2, 577)}            # name -> (frames N, tokens per frame T)
SEEDS = {"a": 5, "b": 1, "c": 3}                               # chosen on the CPU: see test_seeds_keep_the_oracles_decisions_safe
B = 3
TAIL = 8                                                       # the loud last tokens of every video (see tokens())
VIDEO_OF_QUESTION = [1, 2, 1, 0, 1, 2, 1]                      # caller order; per-video counts [1, 4, 2]
QUESTION_TOKENS = [7, 12, 3, 12, 9, 5, 10]                     # [ENC] words [SEP]; question 3 is alone with video 0
N_TRAIN = [1, 2, 1, 1, 3, 1, 2]                                # train=True: question q owns the next N_TRAIN[q] answers
Q = len(VIDEO_OF_QUESTION)


def tokens(case):
    """f32 [B, N*T, WIDTH], every value exactly representable in bf16 and f16: a direction per video plus one per frame plus
    unit noise per token — what a softmax average over the keys keeps differs from video to video (pure noise averages to
    nothing over hundreds of keys, and a question answered from the wrong video would pass).  The last TAIL tokens of a video
    are eight times as large, so that keys lost at the end of the sequence (past 768 in case a) move the states by more than
    the gates allow (tests/test_video_vqa_cpu.py measures both on the oracle)."""
    N, T = CASES[case]
    g = torch.Generator().manual_seed(9000 + 100 * SEEDS[case] + N)
    video = 2.0 * torch.randn(B, 1, 1, WIDTH, generator=g)
    frame = torch.randn(B, N, 1, WIDTH, generator=g)
    noise = torch.randn(B, N, T, WIDTH, generator=g)
    out = (video + frame + noise).view(B, N * T, WIDTH)
    out[:, -TAIL:] *= 8.0
    out = out.bfloat16().float()
    return torch.where(out.abs() < 2.0 ** -10, torch.zeros(()), out)       # (smaller bf16 values are not f16 numbers)


def questions(case):
    rng = np.random.default_rng(77 + SEEDS[case])
    return [vc.words(rng.integers(110, 500, size=n - 2)) for n in QUESTION_TOKENS]


def question_ids(case):
    """(ids int64 [Q, 12], mask int64 [Q, 12]) as models/blip_vqa.py:204-206 builds them on the synthetic tokenizer."""
    tok = vc.VqaTokenizer()
    enc = tok(questions(case), padding="longest", truncation=True, max_length=35, return_tensors="pt")
    ids = enc.input_ids.clone().long()
    ids[:, 0] = tok.enc_token_id
    return ids, enc.attention_mask.long()


def train_inputs(case):
    """(answer indices int64 [sum N_TRAIN] into the golden's 40 answers, weights f32 [sum N_TRAIN])."""
    rng = np.random.default_rng(501 + SEEDS[case])
    n = int(np.sum(N_TRAIN))
    return torch.from_numpy(rng.integers(0, 40, size=n)), torch.from_numpy(rng.uniform(0.1, 1.0, size=n).astype(np.float32))


_REF = {}


def reference(case):
    """vqa_cases.reference() for this case's seven (video, question) pairs, in the CALLER's order.  Computed once per case,
    shared, never modified."""
    if case in _REF:
        return _REF[case]
    g = vc.golden()
    sd_e, sd_d = vc.states()
    with torch.no_grad():
        enc = tokens(case)[torch.tensor(VIDEO_OF_QUESTION)]
        q_ids, q_mask = question_ids(case)
        a_ids, a_mask = torch.from_numpy(g["a_ids"]), torch.from_numpy(g["a_mask"])
        k = int(g["k"])
        qs = vc.stack(sd_e, "text_encoder.", q_ids, q_mask, enc, None, False)
        # rank, stage 1
        start = torch.full((Q, 1), int(a_ids[0, 0]))
        first_logits = vc.decoder_logits(sd_d, start, torch.ones_like(start), qs, q_mask)[:, 0]
        lp64 = torch.log_softmax(first_logits.double(), 1).index_select(1, a_ids[:, 1])
        prob = torch.softmax(first_logits, 1).index_select(1, a_ids[:, 1])
        topk_ids = prob.topk(k, dim=1).indices
        # rank, stage 2
        pick = topk_ids.reshape(-1)
        qi = torch.arange(Q).repeat_interleave(k)
        logits2 = vc.decoder_logits(sd_d, a_ids[pick], a_mask[pick], qs[qi], q_mask[qi])
        log_probs_sum = (-vc.answer_loss(logits2, a_ids[pick])).view(Q, k)
        max_ids = topk_ids.gather(1, log_probs_sum.argmax(1)[:, None])[:, 0]
        # generate: unmasked cross-attention (an all-ones question_atts)
        qs3 = qs.repeat_interleave(vc.NUM_BEAMS, 0)
        trace, calls = [], []

        def step(ids, beam_idx):
            calls.append((ids.copy(), None if beam_idx is None else beam_idx.copy()))
            t = torch.from_numpy(ids)
            return vc.decoder_logits(sd_d, t, torch.ones_like(t), qs3, None)[:, -1].numpy()

        seqs, _ = beam_ref.beam_search(step, np.full((Q, 1), vc.DEC, dtype=np.int64), num_beams=vc.NUM_BEAMS,
                                       max_length=vc.MAX_LENGTH, min_length=vc.MIN_LENGTH, eos_token_id=vc.SEP,
                                       pad_token_id=vc.PAD, trace=trace)
        gen = np.full((Q, vc.MAX_LENGTH), vc.PAD, dtype=np.int64)
        for b, s in enumerate(seqs):
            gen[b, :len(s)] = s
        gen_gap = np.min([np.min(t["cand_scores"][:, :-1] - t["cand_scores"][:, 1:], axis=1) for t in trace], axis=0)
        # train=True (the loss divides by the number of videos of the call = Q pairs, models/blip_vqa.py:240-242)
        ta, tw = train_inputs(case)
        ti = torch.arange(Q).repeat_interleave(torch.tensor(N_TRAIN))
        train_losses = vc.answer_loss(vc.decoder_logits(sd_d, a_ids[ta], a_mask[ta], qs[ti], q_mask[ti]), a_ids[ta])
        train_loss = (tw * train_losses).sum() / Q
    _REF[case] = dict(question_states=qs, first_logits=first_logits, lp64=lp64, topk_ids=topk_ids, log_probs_sum=log_probs_sum,
                      max_ids=max_ids, gen_ids=gen, gen_gap=gen_gap, gen_calls=calls, gen_logits=[t["logits"] for t in trace],
                      train_losses=train_losses, train_loss=train_loss, n_targets=a_mask.sum(1) - 1, k=k,
                      scale=max(1.0, first_logits.abs().max().item(), logits2.abs().max().item()))
    return _REF[case]


def excluded(case, gate):
    """vqa_cases.excluded applied to this reference: the questions whose ranking decisions the oracle itself makes by less
    than what operands of relative error ``gate`` may move.  Returns a bool [Q] tensor."""
    ref = reference(case)
    k = ref["k"]
    unit = 2.0 * gate * ref["scale"]
    srt = ref["lp64"].sort(dim=1, descending=True).values
    out = (srt[:, k - 1] - srt[:, k]) < unit
    s = ref["log_probs_sum"].double()
    nt = ref["n_targets"][ref["topk_ids"]].double()
    best = s.argmax(1, keepdim=True)
    gap = s.gather(1, best) - s
    need = unit * torch.maximum(nt, nt.gather(1, best))
    close = gap < need
    close.scatter_(1, best, False)
    return out | close.any(1)


def video_major(video_of_question, n_videos):
    """The schedule restated with numpy (stable sort): (order, inverse, group_start)."""
    v = np.asarray(video_of_question, dtype=np.int64)
    order = np.argsort(v, kind="stable")
    inverse = np.empty_like(order)
    inverse[order] = np.arange(len(v))
    gs = np.zeros(n_videos + 1, dtype=np.int64)
    gs[1:] = np.cumsum(np.bincount(v, minlength=n_videos))
    return order, inverse, gs
