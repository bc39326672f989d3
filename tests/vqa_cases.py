"""Shared inputs of the question-answering tests (tests/golden/vqa_small.npz: small geometry, the text encoder of
med_itm_small.npz and the decoder of med_decoder_small.npz) and the reference value composed from the existing oracle:
oracle/med_ref.py's embeddings, layer (which takes the cross-attention mask), extended_mask and lm_head."""
import numpy as np
import torch

import caption_scoring_cases as cs
from common import load_golden
from oracle import beam_ref, med_ref

LAYERS, HEADS, V = 2, 4, 512
PAD, SEP, DEC, ENC = 0, 102, 510, 509
NUM_BEAMS, MAX_LENGTH, MIN_LENGTH = 3, 10, 1


class VqaTokenizer(cs.SmallTokenizer):
    """The synthetic tokenizer with [DEC] and [ENC] inside the 512-entry vocabulary of the small geometry."""
    enc_token_id = ENC


def words(ids):
    """The string the synthetic tokenizer turns back into [CLS] ids [SEP] (the ids between the first and the closing token)."""
    return " ".join(f"w{int(i)}" for i in ids)


def golden():
    _, g = load_golden("vqa_small.npz")
    return g


def questions(g):
    return [words(row[1:n - 1]) for row, n in zip(g["q_ids"], g["q_mask"].sum(1))]


def answers(g):
    return [words(row[1:n - 1]) for row, n in zip(g["a_ids"], g["a_mask"].sum(1))]


def states():
    sd_e, _ = load_golden("med_itm_small.npz")
    sd_d, _ = load_golden("med_decoder_small.npz")
    return sd_e, sd_d


def stack(sd, p, ids, attention_mask, enc, enc_attention_mask, is_decoder):
    """models/med.py:670-807 with an encoder attention mask: the loop med_ref.bert_model runs, with
    encoder_extended_attention_mask = invert_attention_mask(mask) = (1 - mask) * -10000 (:756-758) instead of none."""
    T = ids.shape[1]
    self_mask = med_ref.extended_mask(attention_mask, T, is_decoder)
    enc_mask = None if enc_attention_mask is None else (1.0 - enc_attention_mask.float())[:, None, None, :] * -10000.0
    h = med_ref.embeddings(sd, p + "embeddings.", ids)
    for i in range(LAYERS):
        h, _ = med_ref.layer(sd, f"{p}encoder.layer.{i}.", h, self_mask, HEADS, enc, enc_mask)
    return h


def decoder_logits(sd_d, ids, attention_mask, enc, enc_attention_mask):
    return med_ref.lm_head(sd_d, "text_decoder.cls.", stack(sd_d, "text_decoder.bert.", ids, attention_mask, enc,
                                                            enc_attention_mask, True))


def answer_loss(logits, ids):
    """models/med.py:909-917 with reduction='none' and labels = ids with pads ignored (models/blip_vqa.py:53,147)."""
    labels = ids.masked_fill(ids == PAD, -100)
    loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1),
                                             label_smoothing=0.1, reduction="none")
    return loss.view(ids.shape[0], -1).sum(1)


_REF = {}


def reference():
    """Computed once, shared, never modified: the arrays of the golden recomputed by the composed oracle, plus the
    first-token log-probabilities (float64) and, of the beam search, every decoder call (ids, beam_idx) with its logits."""
    if _REF:
        return _REF
    g = golden()
    sd_e, sd_d = states()
    with torch.no_grad():
        enc = torch.from_numpy(g["enc"])[torch.from_numpy(g["q_image"])]
        q_ids, q_mask = torch.from_numpy(g["q_ids"]), torch.from_numpy(g["q_mask"])
        a_ids, a_mask = torch.from_numpy(g["a_ids"]), torch.from_numpy(g["a_mask"])
        Q, k = q_ids.shape[0], int(g["k"])
        qs = stack(sd_e, "text_encoder.", q_ids, q_mask, enc, None, False)
        # rank, stage 1
        start = torch.full((Q, 1), int(a_ids[0, 0]))
        first_logits = decoder_logits(sd_d, start, torch.ones_like(start), qs, q_mask)[:, 0]
        lp64 = torch.log_softmax(first_logits.double(), 1).index_select(1, a_ids[:, 1])
        prob = torch.softmax(first_logits, 1).index_select(1, a_ids[:, 1])
        topk_ids = prob.topk(k, dim=1).indices
        # rank, stage 2
        pick = topk_ids.reshape(-1)
        qi = torch.arange(Q).repeat_interleave(k)
        logits2 = decoder_logits(sd_d, a_ids[pick], a_mask[pick], qs[qi], q_mask[qi])
        log_probs_sum = (-answer_loss(logits2, a_ids[pick])).view(Q, k)
        max_ids = topk_ids.gather(1, log_probs_sum.argmax(1)[:, None])[:, 0]
        # generate: unmasked cross-attention (an all-ones question_atts)
        qs3 = qs.repeat_interleave(NUM_BEAMS, 0)
        trace, calls = [], []

        def step(ids, beam_idx):
            calls.append((ids.copy(), None if beam_idx is None else beam_idx.copy()))
            t = torch.from_numpy(ids)
            return decoder_logits(sd_d, t, torch.ones_like(t), qs3, None)[:, -1].numpy()

        seqs, _ = beam_ref.beam_search(step, np.full((Q, 1), DEC, dtype=np.int64), num_beams=NUM_BEAMS, max_length=MAX_LENGTH,
                                       min_length=MIN_LENGTH, eos_token_id=SEP, pad_token_id=PAD, trace=trace)
        gen = np.full((Q, MAX_LENGTH), PAD, dtype=np.int64)
        for b, s in enumerate(seqs):
            gen[b, :len(s)] = s
        gen_gap = np.min([np.min(t["cand_scores"][:, :-1] - t["cand_scores"][:, 1:], axis=1) for t in trace], axis=0)
        # train=True
        ta = torch.from_numpy(g["train_answers"])
        ti = torch.arange(Q).repeat_interleave(torch.from_numpy(g["n_train"]))
        train_losses = answer_loss(decoder_logits(sd_d, a_ids[ta], a_mask[ta], qs[ti], q_mask[ti]), a_ids[ta])
        train_loss = (torch.from_numpy(g["train_weights"]) * train_losses).sum() / Q
    _REF.update(question_states=qs, first_logits=first_logits, lp64=lp64, topk_ids=topk_ids, log_probs_sum=log_probs_sum,
                max_ids=max_ids, gen_ids=gen, gen_gap=gen_gap, gen_calls=calls, gen_logits=[t["logits"] for t in trace],
                train_losses=train_losses, train_loss=train_loss,
                n_targets=a_mask.sum(1) - 1, scale=max(1.0, first_logits.abs().max().item(), logits2.abs().max().item()))
    return _REF


def excluded(gate):
    """Questions whose ranking decisions the oracle itself makes by less than what operands of relative error ``gate`` may move
    (gate x logit scale x 2 x target tokens): the k-th / (k+1)-th first-token log-probabilities (one target token), or the best
    log_probs_sum and any other of the k (the longer answer's target count).  Returns a bool [Q] tensor."""
    ref, g = reference(), golden()
    k = int(g["k"])
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
