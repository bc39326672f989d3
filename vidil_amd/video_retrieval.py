"""Video-text retrieval evaluation on the HIP kernels — the reference's ``eval_retrieval_video.py`` (``evaluation`` :26-129,
``itm_eval`` :133-175) for the ``video_representation: concat_frame`` configs: a video is N frames, its ITC embedding the
normalised mean of the frames' ``vision_proj([CLS])`` and its encoder states ALL N frames' ViT tokens as one sequence of N*T
keys (``video_feat.view(B, -1, C)``, :69) — 8 x 197 = 1,576 at 224^2, 8 x 577 = 4,616 at 384^2: the long-key form of
``vidil_attention``.

Schedule of ``evaluation`` (the reference runs one text-encoder batch of k_test pairs per video and then one per text):

  * features once: the frames' tokens and the video embeddings per batch of ``videos``, the text embeddings per 512 texts;
    the similarity matrix is the exact-f32 ``K.scan_scores``, its candidates ``K.topk_rows`` of the matrix (video -> text)
    and of its transpose (text -> video): sorted (value desc, index asc);
  * ``ITM(v, t)`` is the same number in both directions, so the candidate pairs of BOTH directions are united, sorted
    video-major (``pair_union``) and scored ONCE through ``BLIP_ITM.itm_pairs(group_start=, pair_text=)``;
  * the videos are walked in blocks of ``videos_per_block``: a block's cross-attention K / V (every layer, N*T keys per
    video) are projected once, the text-only front of the encoder runs once per distinct text of the block, and the pair
    stack once per pair.  Every block is launched with the SAME token count (the longest text of all) and the SAME
    ``max_group`` bound (the largest group of all), so a pair's bits do not depend on the block size;
  * both score matrices are scattered from the one score vector ``itm_logit[:, 1] + sim``: a pair that is a candidate in
    both directions holds the same bits in both.

``videos_per_block`` defaults to what fits ``video.KV_BLOCK_BYTES``: a video's K / V are L layers x 2 (K, V) x N*T keys x C
channels x 2 bytes (12 x 2 x 1,576 x 768 x 2 B = 58 MB at 224^2 x 8 frames, 170 MB at 384^2 x 8).  The frames' tokens of
all videos stay on the device (N*T x width x 2 bytes per video: 2.4 GB for 1,000 videos at 224^2 x 8 frames); the frames
themselves are consumed batch by batch.

World size 1; the parity precision mode is not built for this path (``evaluation`` raises)."""
from __future__ import annotations

import json
import re
import time

import numpy as np
import torch

from . import kernels as K
from . import video
from .video import KV_BLOCK_BYTES, phase_timer  # noqa: F401  (their home is video.py; imported from here too)

FILL = -100.0                      # eval_retrieval_video.py:77,100


# ---------------------------------------------------------------------------------------------- annotations
def pre_caption(caption, max_words=50):
    """The reference's caption cleaning (data/utils.py:35-54): lower case, the punctuation . ! " ( ) * # : ; ~ to blanks, runs
    of white space to one blank, stripped, at most ``max_words`` words."""
    caption = re.sub(r"([.!\"()*#:;~])", " ", caption.lower())
    caption = re.sub(r"\s{2,}", " ", caption).rstrip("\n").strip(" ")
    words = caption.split(" ")
    return " ".join(words[:max_words]) if len(words) > max_words else caption


def load_retrieval_annotations(jsonl):
    """One JSON object per line with ``clip_name`` and ``caption`` (data/video_eval_dataset.py:30-32,70-72) ->
    (clip_names, texts = pre_caption(caption, 40), txt2video, video2txt): text i belongs to video i."""
    with open(jsonl, "r") as f:
        ann = [json.loads(line) for line in f if line.strip()]
    names = [a["clip_name"] for a in ann]
    texts = [pre_caption(a["caption"], 40) for a in ann]
    ident = list(range(len(ann)))
    return names, texts, ident, list(ident)


# ---------------------------------------------------------------------------------------------- schedule
def pair_union(idx_v2t, idx_t2v):
    """The united, video-major pair list of both directions' candidates (CPU index tensors; pure).

    idx_v2t int [V, k1]: candidate texts of every video; idx_t2v int [Tn, k2]: candidate videos of every text.
    Returns a dict: ``pair_video`` / ``pair_text`` int64 [P] — every (video, text) that is a candidate in either direction,
    exactly once, ordered by (video, text); ``group_start`` int32 [V+1] — the pairs of video v are group_start[v] ..
    group_start[v+1]-1 (empty for a video nobody lists); ``max_group`` — its largest gap; ``slot_v2t`` int64 [V, k1] /
    ``slot_t2v`` int64 [Tn, k2] — the position in the pair list of every candidate."""
    idx_v2t, idx_t2v = idx_v2t.long().cpu(), idx_t2v.long().cpu()
    V, Tn = idx_v2t.shape[0], idx_t2v.shape[0]
    if idx_v2t.numel() and not (0 <= int(idx_v2t.min()) and int(idx_v2t.max()) < Tn):
        raise ValueError("pair_union: a video lists a text outside 0..Tn-1")
    if idx_t2v.numel() and not (0 <= int(idx_t2v.min()) and int(idx_t2v.max()) < V):
        raise ValueError("pair_union: a text lists a video outside 0..V-1")
    key_v2t = torch.arange(V)[:, None] * Tn + idx_v2t                      # key = video * Tn + text
    key_t2v = idx_t2v * Tn + torch.arange(Tn)[:, None]
    keys, inv = torch.unique(torch.cat([key_v2t.reshape(-1), key_t2v.reshape(-1)]), sorted=True, return_inverse=True)
    pair_video = torch.div(keys, Tn, rounding_mode="floor") if Tn else keys
    pair_text = keys - pair_video * Tn
    group_start, max_group = video.group_table(pair_video, V)
    return dict(pair_video=pair_video, pair_text=pair_text, group_start=group_start, max_group=max_group,
                slot_v2t=inv[:key_v2t.numel()].view(idx_v2t.shape), slot_t2v=inv[key_v2t.numel():].view(idx_t2v.shape))


def scatter_scores(sched, pair_score, idx_v2t, idx_t2v, V, Tn):
    """(score_v2t [V, Tn], score_t2v [Tn, V]) numpy f32: FILL everywhere, a row's candidates hold their pair's score."""
    pair_score = np.asarray(pair_score, dtype=np.float32)
    idx_v2t, idx_t2v = np.asarray(idx_v2t, dtype=np.int64), np.asarray(idx_t2v, dtype=np.int64)
    v2t = np.full((V, Tn), FILL, dtype=np.float32)
    t2v = np.full((Tn, V), FILL, dtype=np.float32)
    np.put_along_axis(v2t, idx_v2t, pair_score[sched["slot_v2t"].numpy()], axis=1)
    np.put_along_axis(t2v, idx_t2v, pair_score[sched["slot_t2v"].numpy()], axis=1)
    return v2t, t2v


def default_videos_per_block(model, tokens_per_video):
    """video.videos_per_block for the model's text encoder."""
    return video.videos_per_block(model.text_encoder.config, tokens_per_video)


# ---------------------------------------------------------------------------------------------- evaluation
@torch.no_grad()
def evaluation(model, videos, texts, k_test, *, videos_per_block=None, device="cuda", timings=None):
    """eval_retrieval_video.py:26-129 for world size 1.  ``model``: a BLIP_Retrieval on ``device``; ``videos``: an iterable of
    uint8 frame batches [b, N, S, S, 3] (numpy or torch; every video the same N); ``texts``: list[str].
    Returns (score_v2t [V, Tn], score_t2v [Tn, V]) numpy f32: -100 except each row's min(k_test, row length) candidates, which
    hold ``itm_logit[:, 1] + sim`` with the texts' first id := [ENC].
    ``timings`` (dict, optional): receives the seconds spent in ``vit`` / ``text`` / ``kv`` / ``pairs`` (each synchronised)."""
    if model.parity:
        raise K.VidilHipError("video_retrieval.evaluation: not built for the parity precision mode (set_parity_mode(False, model))")
    import time

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0

    dev = torch.device(device)
    t0 = time.perf_counter()
    txt_emb, ids, lens = model.text_features(list(texts), dev)            # ids[:, 0] = [ENC] (:55)
    lap("text", t0)
    t0 = time.perf_counter()
    tokens, embeds, n_frames = [], [], None
    for batch in videos:
        batch = torch.as_tensor(batch)
        if batch.dtype != torch.uint8 or batch.dim() != 5:
            raise K.VidilHipError(f"evaluation: uint8 [b,N,S,S,3] frame batches expected, got {batch.dtype} {tuple(batch.shape)}")
        if n_frames is None:
            n_frames = batch.shape[1]
        elif batch.shape[1] != n_frames:
            raise K.VidilHipError(f"evaluation: every video needs the same number of frames ({n_frames}), got {batch.shape[1]}")
        y16, emb = model.video_features_u8(batch.to(dev))
        tokens.append(y16)
        embeds.append(emb)
    if not tokens:
        raise K.VidilHipError("evaluation: no videos")
    tokens = tokens[0] if len(tokens) == 1 else torch.cat(tokens, 0)
    vid_emb = embeds[0] if len(embeds) == 1 else torch.cat(embeds, 0)
    lap("vit", t0)
    V, Tn = vid_emb.shape[0], txt_emb.shape[0]
    Te = tokens.shape[0] // V                                             # N * T keys per video
    sims = K.scan_scores(vid_emb, txt_emb)                                # [V, Tn] exact f32 (:76)
    _, idx_v2t = K.topk_rows(sims, min(k_test, Tn))                       # (:86)
    _, idx_t2v = K.topk_rows(sims.t().contiguous(), min(k_test, V))       # (:99,108)
    sched = pair_union(idx_v2t.cpu(), idx_t2v.cpu())
    pv, pt = sched["pair_video"], sched["pair_text"]
    itm = torch.empty(pv.numel(), dtype=torch.float32, device=dev)
    t_eff = max(1, min(ids.shape[1], int(lens.max().item())))
    if videos_per_block is None:
        videos_per_block = default_videos_per_block(model, Te)
    for b0, b1, p0, p1, groups in video.blocks(sched["group_start"], V, videos_per_block):
        t0 = time.perf_counter()
        enc = tokens[b0 * Te:b1 * Te]
        cross = model.project_image_kv(enc, b1 - b0, sched["max_group"] * t_eff)
        lap("kv", t0)
        t0 = time.perf_counter()
        uniq, local = torch.unique(pt[p0:p1], sorted=True, return_inverse=True)    # the block's distinct texts
        uniq = uniq.to(dev)
        out = model.itm_pairs(enc, b1 - b0, ids.index_select(0, uniq), lens.index_select(0, uniq),
                              group_start=groups, max_group=sched["max_group"], pair_text=local, cross=cross, t_eff=t_eff)
        itm[p0:p1] = out[:, 1]
        lap("pairs", t0)
    score = itm + sims[pv.to(dev), pt.to(dev)]                            # score + topk_sim (:97,118)
    return scatter_scores(sched, score.cpu().numpy(), idx_v2t.cpu().numpy(), idx_t2v.cpu().numpy(), V, Tn)


def itm_eval(scores_v2t, scores_t2v, txt2vid, vid2txt):
    """Recall@1/5/10 of both directions, their means and the median text->video rank (eval_retrieval_video.py:133-175): the
    rank of a row's true match is its position in ``np.argsort(row)[::-1]``."""
    def ranks_of(scores, truth):
        r = np.zeros(scores.shape[0])
        for i, row in enumerate(scores):
            r[i] = np.where(np.argsort(row)[::-1] == truth[i])[0][0]
        return r

    def recalls(r):
        return [100.0 * np.count_nonzero(r < k) / len(r) for k in (1, 5, 10)]

    rv = ranks_of(scores_v2t, vid2txt)           # video -> text
    rt = ranks_of(scores_t2v, txt2vid)           # text -> video
    tr1, tr5, tr10 = recalls(rv)
    vr1, vr5, vr10 = recalls(rt)
    tr_mean, vr_mean = (tr1 + tr5 + tr10) / 3, (vr1 + vr5 + vr10) / 3
    return {"txt_r1": tr1, "txt_r5": tr5, "txt_r10": tr10, "txt_r_mean": tr_mean,
            "vid_r1": vr1, "vid_r5": vr5, "vid_r10": vr10, "vid_r_mean": vr_mean,
            "vid_mdR": np.median(rt + 1), "r_mean": (tr_mean + vr_mean) / 2}
