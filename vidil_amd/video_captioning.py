"""Video captioning evaluation on the HIP kernels — the loop of the reference's ``train_caption_video.py`` (``evaluate``
:76-101) for a ``BLIP_Video_Decoder`` (vidil_amd/blip.py), world size 1.

``video_representation: concat_frame`` hands a batch's videos to ``BLIP_Video_Decoder.generate``: the ViT over the B*N frames,
then a beam search per video over its N*T frame tokens as ONE encoder sequence, ``videos_per_block`` videos side by side
(default: what ``video.KV_BLOCK_BYTES`` holds of cross K / V).  ``single_frame`` captions frame int(N/2) alone through
``BLIP_Decoder``'s path (:88-91).  A video's caption does not depend on the batch or the block it falls in.

Plain f16 / bf16 operands (the model refuses the parity precision mode and fp8)."""
from __future__ import annotations

import torch

from . import kernels as K
from .blip import BLIP_Decoder
from .video import frame_tokens, middle_frame, phase_timer


@torch.no_grad()
def evaluation(model, batches, config, *, videos_per_block=None, timings=None, details=None):
    """train_caption_video.py:76-101.  ``model``: a BLIP_Video_Decoder on the GPU; ``batches``: an iterable of (videos, video_ids)
    — videos f32 [b,N,3,S,S] (normalised) or uint8 [b,N,S,S,3] (the fused preprocessing), numpy or torch, on any device;
    ``config``: ``video_representation`` (concat_frame | single_frame), ``num_beams``, ``max_length``, ``min_length`` — the keys
    the reference's loop reads.  Returns [{"video_id": ..., "caption": str}, ...] in the order the videos arrive.
    ``timings`` (dict, optional): receives the seconds spent in ``vit`` / ``search`` (video.phase_timer: HIP events,
    each phase synchronised; the search includes the cross K | V projection).  ``details`` (dict, optional; what the tests
    compare): receives ``tokens``, the i32 [videos, max_length] token ids of the captions, on the host."""
    rep = config["video_representation"]
    if rep not in ("concat_frame", "single_frame"):
        raise ValueError(f"unknown video_representation {rep!r} (concat_frame | single_frame)")
    kw = dict(num_beams=config["num_beams"], max_length=config["max_length"], min_length=config["min_length"])
    model._require_plain()
    K.require_num_beams(kw["num_beams"], "video_captioning.evaluation")     # (1..K.MAX_BEAMS, before the first batch is touched)
    dev = next(model.text_decoder.parameters()).device
    lap = phase_timer(timings)
    result, tokens = [], []
    for videos, video_ids in batches:
        videos = torch.as_tensor(videos)
        video_ids = list(video_ids)
        if videos.dim() != 5 or videos.shape[0] != len(video_ids):
            raise ValueError(f"evaluation: a batch of [b,N,3,S,S] (f32) or [b,N,S,S,3] (uint8) videos with b video_ids expected, got "
                             f"{tuple(videos.shape)} and {len(video_ids)} ids")
        if rep == "single_frame":
            videos = middle_frame(videos)                                # pick middle frame (:89-91)
        videos = videos.to(dev)
        t0 = lap()
        if rep == "concat_frame":
            tok16 = model.video_tokens_u8(videos) if videos.dtype == torch.uint8 else model.video_tokens(videos)
            t0 = lap("vit", t0)
            det = {}
            captions = model.generate(tok16.view(videos.shape[0], -1, tok16.shape[-1]), sample=False, videos_per_block=videos_per_block,
                                      details=det, **kw)
            out_tok = det["tokens"]
        else:
            tok16 = frame_tokens(model.visual_encoder, videos, who=None)  # (its own check above; BLIP_Decoder refuses the rest)
            t0 = lap("vit", t0)
            out_tok = BLIP_Decoder.generate_ids(model, tok16, videos.shape[0], **kw)[0].cpu()
            captions = model.decode_captions(out_tok)
        lap("search", t0)
        tokens.append(out_tok)
        for caption, vid in zip(captions, video_ids):
            result.append({"video_id": vid, "caption": caption})
    if details is not None:
        details["tokens"] = torch.cat(tokens) if tokens else torch.zeros((0, config["max_length"]), dtype=torch.int32)
    return result
