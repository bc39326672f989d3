"""The single-frame representation's ITM filter of pretrain_video.py:30-63: of a video's N frames and its caption's sentences, the
(frame, sentence) pair the matching head scores highest.

The reference calls the filter once per sentence, each call running the ViT over the same N frames again (:54-56).  Here the ViT
runs once and all N x S pairs go through ONE ``BLIP_ITM.itm_pairs`` call: image-major groups (a frame's cross K/V is fetched once
for its S sentences) over the distinct sentences (``pair_text``: the text-only front runs once per sentence).
"""
from __future__ import annotations

import re

import numpy as np
import torch

from . import capfilt
from .packing import require_cuda
from .video import VIT_VIDEOS


def sentence_tokenization(text, nlp=None):
    """pretrain_video.py:30-44: newlines and ``* # / : ; ~`` become '. ', the caption is lower-cased, and the sentences longer
    than 3 characters are kept, stripped; a caption without one yields its stripped original.  nlp: a spaCy pipeline (anything
    whose result has ``.sents`` of objects with ``.text``) or "naive"; None: what ``capfilt.split_sentences`` uses."""
    caption = re.sub(r"([*#/:;~])", ". ", text.replace("\n", ". ").lower())
    sentences = [s.strip() for s in capfilt.sentences_of(capfilt.sentence_splitter() if nlp is None else nlp, caption) if len(s) > 3]
    return sentences or [text.strip()]


def _select(filterer, y16, n_frames, sentences):
    """scores f32 [S, N] (host) of one video's frames (y16: their token rows) against its sentences, and the first maximum."""
    distinct = list(dict.fromkeys(sentences))
    ids, lens = filterer.tokenize(distinct)
    S = len(sentences)
    of_sentence = torch.tensor([distinct.index(s) for s in sentences])
    logits = filterer.itm_pairs(y16, n_frames, ids, lens, group_start=torch.arange(n_frames + 1) * S, max_group=S,
                                pair_text=of_sentence.repeat(n_frames))                       # pair (frame n, sentence s) at n*S + s
    scores = torch.softmax(logits, dim=1)[:, 1].view(n_frames, S).t().contiguous().cpu()
    flat = int(np.argmax(scores.numpy()))                      # the first maximum in the order sentence * N + frame (:57-62)
    return flat % n_frames, sentences[flat // n_frames], scores


@torch.no_grad()
def select_frame(filterer, frames, text, nlp=None):
    """pretrain_video.py:46-63.  filterer: a ``BLIP_ITM``; frames f32 [N,3,S,S] (normalised) on the GPU; text: the video's caption.
    -> (frame_index, sentence, scores f32 [S, N] on the host: softmax(itm logits)[:, 1] of every sentence against every frame)."""
    require_cuda(frames, "select_frame")
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"select_frame: f32 [N,3,S,S] expected, got {tuple(frames.shape)}")
    sentences = sentence_tokenization(text, nlp)
    _, y16 = filterer.visual_encoder.forward_both(frames)
    return _select(filterer, y16, frames.shape[0], sentences)


@torch.no_grad()
def select_frames(filterer, videos, texts, nlp=None, videos_per_pass=VIT_VIDEOS):
    """``select_frame`` for a batch: videos f32 [B,N,3,S,S] on the GPU, texts: B captions -> a list of B results.  The ViT runs
    over ``videos_per_pass`` videos' frames at a time; every video then has its own ``itm_pairs`` call, as in ``select_frame``."""
    require_cuda(videos, "select_frames")
    if videos.dim() != 5 or videos.shape[2] != 3:
        raise ValueError(f"select_frames: f32 [B,N,3,S,S] expected, got {tuple(videos.shape)}")
    texts = list(texts)
    B, N = videos.shape[:2]
    if len(texts) != B:
        raise ValueError(f"select_frames: {B} videos and {len(texts)} captions")
    sentences = [sentence_tokenization(t, nlp) for t in texts]
    out = []
    for b0 in range(0, B, videos_per_pass):
        blk = videos[b0:b0 + videos_per_pass]
        _, y16 = filterer.visual_encoder.forward_both(blk.flatten(0, 1))
        rows = y16.shape[0] // blk.shape[0]
        for j in range(blk.shape[0]):
            out.append(_select(filterer, y16[j * rows:(j + 1) * rows], N, sentences[b0 + j]))
    return out
