"""Shared inputs of the video captioning tests and the reference value composed from what exists: the decoder of
tests/golden/med_decoder_small.npz with the prompt ids 510 7 8 9 (caption_scoring_cases.small_state / oracle_logits /
oracle_loss), oracle/beam_ref.py, and the three-video token tables of video_vqa_cases.tokens(case) as the videos:

  a   N = 8, T = 97    776 keys: just past the 768 keys the short attention kernels end at
  b   N = 4, T = 17     68 keys: the launches of the image captioner
  c   N = 2, T = 577  1,154 keys

Beam search with 3 beams, max_length 30, min_length 5.  tests/test_video_captioning_cpu.py pins what the fixture can detect."""
import numpy as np
import torch

import caption_scoring_cases as cs
import video_vqa_cases as vv
from oracle import beam_ref

CASES, B, WIDTH, TAIL = vv.CASES, vv.B, vv.WIDTH, vv.TAIL
NUM_BEAMS, MAX_LENGTH, MIN_LENGTH = 3, 30, 5
PROMPT_IDS = [510, 7, 8, 9]                       # [DEC] w7 w8 w9: caption_scoring_cases.PROMPT on its SmallTokenizer
SEP, PAD = cs.SmallTokenizer.sep_token_id, cs.SmallTokenizer.pad_token_id
VIDEO_INDEX = cs.IMAGE_INDEX                      # the scored captions: caption p describes video VIDEO_INDEX[p]


def tokens(case):
    """f32 [3, N*T, 256], every value a bf16 and an f16 number (video_vqa_cases.tokens)."""
    return vv.tokens(case)


def last_logits(sd, enc, ids):
    """Oracle logits f32 [rows, V] of the last position: ids int64 [rows, t], row r attends to enc[r] (every key)."""
    ids = torch.as_tensor(ids)
    return cs.oracle_logits(sd, enc, ids, torch.ones_like(ids), torch.arange(ids.shape[0]))[:, -1]


def prompt_logits(enc):
    """The shared prompt pass of a search over videos enc f32 [B, keys, 256]: logits f32 [B, V]."""
    sd, _ = cs.small_state()
    return last_logits(sd, enc, torch.tensor([PROMPT_IDS] * enc.shape[0]))


_REF = {}


def reference(case):
    """The oracle's search over the case's three videos.  Computed once per case, shared, never modified: dict(calls — (ids,
    beam_idx) of every decoder call —, logits — f32 [9, V] per call —, seqs, gen_ids int64 [3, 30], gen_gap — per video the
    smallest gap between neighbouring candidates of any step —, scale = max(1, max|logit|) over all calls)."""
    if case in _REF:
        return _REF[case]
    sd, _ = cs.small_state()
    enc3 = tokens(case).repeat_interleave(NUM_BEAMS, 0)
    trace, calls = [], []

    def step(ids, beam_idx):
        calls.append((ids.copy(), None if beam_idx is None else beam_idx.copy()))
        return last_logits(sd, enc3, torch.from_numpy(ids)).numpy()

    seqs, _ = beam_ref.beam_search(step, np.asarray([PROMPT_IDS] * B, dtype=np.int64), num_beams=NUM_BEAMS, max_length=MAX_LENGTH,
                                   min_length=MIN_LENGTH, eos_token_id=SEP, pad_token_id=PAD, trace=trace)
    gen = np.full((B, MAX_LENGTH), PAD, dtype=np.int64)
    for b, s in enumerate(seqs):
        gen[b, :len(s)] = s
    gap = np.min([np.min(t["cand_scores"][:, :-1] - t["cand_scores"][:, 1:], axis=1) for t in trace], axis=0)
    logits = [t["logits"] for t in trace]
    _REF[case] = dict(calls=calls, logits=logits, seqs=seqs, gen_ids=gen, gen_gap=gap,
                      scale=max(1.0, max(float(np.abs(l).max()) for l in logits)))
    return _REF[case]


_LOSS = {}


def loss_reference(case):
    """caption_scoring_cases.reference() over this case's videos: the seven captions of caption_scoring_cases.captions(),
    caption p about video VIDEO_INDEX[p].  dict(ids, mask, labels, logits, none, mean, counts), computed once per case."""
    if case not in _LOSS:
        sd, _ = cs.small_state()
        ids, mask, labels = cs.reference_targets(cs.SmallTokenizer(), cs.captions(), cs.PROMPT_LENGTH)
        logits = cs.oracle_logits(sd, tokens(case), ids, mask, VIDEO_INDEX)
        _LOSS[case] = dict(ids=ids, mask=mask, labels=labels, logits=logits, none=cs.oracle_loss(logits, labels, "none"),
                           mean=cs.oracle_loss(logits, labels, "mean"), counts=(labels[:, 1:] >= 0).sum(1))
    return _LOSS[case]
