"""BLIP caption decoder on the HIP kernels — drop-in for the reference's
``models/blip.py`` on the hot path: ``blip_decoder(pretrained, image_size, vit)``,
``BLIP_Decoder.generate(image, sample=False, num_beams=3, max_length=…, min_length=…)
-> list[str]``, ``init_tokenizer``, ``create_vit``, ``load_checkpoint``.

The beam search behind ``generate`` (``generate_ids``) and the decoding session are
decoding.py's: ``BeamSearchMixin``, ``DecoderSession``.
"""
from __future__ import annotations

import os
from urllib.parse import urlparse

import torch
import torch.nn as nn

from . import kernels as K
from . import video as V
from .decoding import BeamSearchMixin, DecoderSession, DecodeTrace  # noqa: F401  (their home is decoding.py; imported from here too)
from .med import BertConfig, BertLMHeadModel, BertModel
from .packing import require_cuda
from .tokenizer import init_tokenizer, refuse_synthetic_with_checkpoint  # noqa: F401  (init_tokenizer re-exported, reference API)
from .video import CLIP_MEAN, CLIP_STD, MAX_VIDEO_TOKENS  # noqa: F401  (their home is video.py; imported from here too)
from .vit import VisionTransformer, interpolate_pos_embed

_DEFAULT_MED_CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs", "med_config.json")

CAPTION_MAX_LENGTH = 40                           # models/blip.py:109 (captions given to forward are cut to 40 tokens)


def resolve_med_config(path):
    """The reference default is the repo-relative 'configs/med_config.json'; fall back to the packaged copy."""
    if path and os.path.isfile(path):
        return path
    return _DEFAULT_MED_CONFIG


def create_vit(vit, image_size, use_grad_checkpointing=False, ckpt_layer=0, drop_path_rate=0, **_):
    """Reference: models/blip.py:298-326 (widths/depths/heads of 'base' and 'large')."""
    if vit == "base":
        width = 768
        enc = VisionTransformer(img_size=image_size, patch_size=16, embed_dim=width, depth=12, num_heads=12)
    elif vit == "large":
        width = 1024
        enc = VisionTransformer(img_size=image_size, patch_size=16, embed_dim=width, depth=24, num_heads=16)
    else:
        raise ValueError("cannot create vit:", vit)
    return enc, width


def is_url(url_or_filename):
    return urlparse(url_or_filename).scheme in ("http", "https")


def load_checkpoint(model, url_or_filename):
    """Reference semantics (models/blip.py:332-354): checkpoint['model'], position-embedding
    interpolation, shape-mismatched keys dropped, strict=False."""
    if is_url(url_or_filename):
        from torch.hub import load_state_dict_from_url

        checkpoint = load_state_dict_from_url(url_or_filename, map_location="cpu", check_hash=False, progress=True)
    elif os.path.isfile(url_or_filename):
        checkpoint = torch.load(url_or_filename, map_location="cpu")
    else:
        raise RuntimeError("checkpoint url or path is invalid")
    state_dict = checkpoint["model"]
    state_dict["visual_encoder.pos_embed"] = interpolate_pos_embed(state_dict["visual_encoder.pos_embed"],
                                                                   model.visual_encoder)
    own = model.state_dict()
    for key in list(own.keys()):
        if key in state_dict and state_dict[key].shape != own[key].shape:
            del state_dict[key]
    msg = model.load_state_dict(state_dict, strict=False)
    print("load checkpoint from %s" % url_or_filename)
    return model, msg


class BLIP_Base(nn.Module):
    """The reference's feature extractor (models/blip.py:22-74): a ViT and the cross-attending text encoder, no heads."""

    def __init__(self, med_config="configs/med_config.json", image_size=224, vit="base", vit_grad_ckpt=False, vit_ckpt_layer=0,
                 tokenizer=None):
        super().__init__()
        self.visual_encoder, vision_width = create_vit(vit, image_size, vit_grad_ckpt, vit_ckpt_layer)
        self.tokenizer = tokenizer if tokenizer is not None else init_tokenizer()
        cfg = BertConfig.from_json_file(resolve_med_config(med_config))
        cfg.encoder_width = vision_width
        self.text_encoder = BertModel(config=cfg, add_pooling_layer=False)

    @torch.no_grad()
    def forward(self, image, caption, mode):
        """models/blip.py:45-73.  image f32 [B,3,S,S] on the device, caption a string or B strings.
        mode='image': the ViT's tokens f32 [B, T, width]; 'text': the text encoder's states without cross-attention, f32
        [B, L, C]; 'multimodal': first id := [ENC], the states of the encoder cross-attending to the image's tokens.
        Captions of different lengths are padded to the longest (L) and masked (``BertModel.forward``'s prefix-mask form) —
        the reference tokenises without padding, which only works for equal lengths."""
        assert mode in ["image", "text", "multimodal"], "mode parameter must be image, text, or multimodal"
        require_cuda(image, "BLIP_Base.forward")
        dev = image.device
        if mode == "image":
            return self.visual_encoder(image)
        text = self.tokenizer([caption] if isinstance(caption, str) else list(caption), padding="longest", return_tensors="pt")
        ids, mask = text.input_ids.clone(), text.attention_mask.to(dev)
        if mode == "text":
            return self.text_encoder(ids.to(dev), attention_mask=mask, return_dict=True, mode="text").last_hidden_state
        B = image.shape[0]
        _, y16 = self.visual_encoder.forward_both(image)
        ids[:, 0] = self.tokenizer.enc_token_id
        # (encoder_attention_mask: the reference's all-ones image_atts is the default)
        return self.text_encoder(ids.to(dev), attention_mask=mask, encoder_hidden_states=y16.view(B, -1, y16.shape[-1]),
                                 return_dict=True).last_hidden_state


def blip_feature_extractor(pretrained="", **kwargs):
    """Reference: models/blip.py:283-288."""
    model = BLIP_Base(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        assert len(msg.missing_keys) == 0
    return model


class BLIP_Decoder(BeamSearchMixin, nn.Module):
    def __init__(self, med_config="configs/med_config.json", image_size=384, vit="base", vit_grad_ckpt=False,
                 vit_ckpt_layer=0, prompt="a picture of ", tokenizer=None):
        super().__init__()
        self.visual_encoder, vision_width = create_vit(vit, image_size, vit_grad_ckpt, vit_ckpt_layer)
        self.tokenizer = tokenizer if tokenizer is not None else init_tokenizer()
        cfg = BertConfig.from_json_file(resolve_med_config(med_config))
        cfg.encoder_width = vision_width
        self.text_decoder = BertLMHeadModel(config=cfg)
        self.prompt = prompt
        self.prompt_length = len(self.tokenizer(self.prompt).input_ids) - 1

    # ------------------------------------------------------------------ prompt ids
    def prompt_ids(self, B, device):
        """models/blip.py:135-138: tokenise the prompt, first id := [DEC], drop the trailing [SEP]."""
        ids = self.tokenizer([self.prompt] * B, return_tensors="pt").input_ids
        ids[:, 0] = self.tokenizer.bos_token_id
        return ids[:, :-1].to(torch.int32).to(device)

    # ------------------------------------------------------------------ nucleus sampling
    def _fresh_seed(self):
        """The seed of a sampling call that is given none: torch's initial seed, moved on by every such call of this model."""
        self._sample_calls = getattr(self, "_sample_calls", 0) + 1
        return (torch.initial_seed() + (self._sample_calls << 32)) & 0xFFFFFFFFFFFFFFFF

    @torch.no_grad()
    def sample_ids(self, enc16, B, *, top_p=0.9, max_length=30, min_length=10, top_k=50, repetition_penalty=1.1,
                   seed=None, row_offset=0, check_done_every=4):
        """Nucleus sampling (models/blip.py:140-151: HF sample() with top_p, BertConfig's default top_k = 50 and the
        hard-coded repetition_penalty = 1.1), one sequence per image.  Returns tokens i32 [B,max_length] (prompt, drawn
        tokens, [SEP] when drawn, then [PAD]).  The random draw follows this library's Philox contract (see
        vidil_sample_top_k_top_p): deterministic in (seed, row_offset + image index, step)."""
        require_cuda(enc16, "BLIP_Decoder.generate")
        tok = self.tokenizer
        eos, pad = tok.sep_token_id, tok.pad_token_id
        dev = enc16.device
        if seed is None:
            seed = self._fresh_seed()
        prompt = self.prompt_ids(B, dev)
        P = prompt.shape[1]
        sess = DecoderSession(self.text_decoder, enc16, B, 1, max_length, tiled_cross=P <= 32)
        seqs = torch.full((B, max_length), pad, dtype=torch.int32, device=dev)
        seqs[:, :P] = prompt
        done = torch.zeros((B,), dtype=torch.int32, device=dev)
        n_done = torch.zeros((1,), dtype=torch.int32, device=dev)
        next_tok = torch.zeros((B,), dtype=torch.int32, device=dev)
        ident = torch.arange(B, dtype=torch.int32, device=dev)
        logits = sess.prefill(prompt.contiguous().view(-1), P, shared=True)     # one row per image == every row
        cur_len, step = P, 0
        while True:
            K.sample_top_k_top_p(logits, seqs, done, n_done, next_tok, cur_len=cur_len, min_length=min_length, eos_id=eos,
                                 pad_id=pad, top_k=top_k, top_p=top_p, rep_penalty=repetition_penalty, seed=seed, step=step,
                                 row_offset=row_offset)
            cur_len += 1
            step += 1
            if cur_len >= max_length:
                break
            if check_done_every and (step % check_done_every == 0) and int(n_done.item()) == B:
                break
            logits = sess.step(next_tok, ident, cur_len - 1)
        return seqs

    def decode_captions(self, out_tok):
        captions = []
        for row in out_tok.cpu().tolist():
            text = self.tokenizer.decode(row, skip_special_tokens=True)
            captions.append(text[len(self.prompt):])
        return captions

    @torch.no_grad()
    def generate(self, image, sample=False, num_beams=3, max_length=30, min_length=10, top_p=0.9,
                 repetition_penalty=1.0):
        """Reference: models/blip.py:127-167.  image f32 [B,3,S,S] on the GPU -> list of B captions."""
        if sample:
            _, y16 = self.visual_encoder.forward_both(image)
            return self.decode_captions(self.sample_ids(y16, image.shape[0], top_p=top_p, max_length=max_length,
                                                        min_length=min_length))
        K.require_num_beams(num_beams, "BLIP_Decoder.generate")              # (before the ViT runs)
        _, y16 = self.visual_encoder.forward_both(image)
        out_tok, _ = self.generate_ids(y16, image.shape[0], num_beams=num_beams, max_length=max_length,
                                       min_length=min_length, repetition_penalty=repetition_penalty)
        return self.decode_captions(out_tok)

    # ------------------------------------------------------------------ scoring given captions
    def tokenize_captions(self, captions):
        """models/blip.py:109-111: padding='longest', truncation at CAPTION_MAX_LENGTH tokens, first id := [DEC].
        Returns (ids i32 [P, T], lens i32 [P]) on the host."""
        enc = self.tokenizer(list(captions), padding="longest", truncation=True, max_length=CAPTION_MAX_LENGTH, return_tensors="pt")
        ids = enc.input_ids.clone()
        ids[:, 0] = self.tokenizer.bos_token_id
        return ids.to(torch.int32), enc.attention_mask.sum(dim=1).to(torch.int32)

    @torch.no_grad()
    def caption_nll(self, image_or_enc16, captions, image_index=None, *, group_start=None, add_prompt=False,
                    label_smoothing=0.1, reduction="none"):
        """How likely the captioner finds GIVEN captions: the teacher-forced loss of models/blip.py:104-125.

        image_or_enc16: images f32 [B,3,S,S] on the GPU (the ViT runs once per image), or their image tokens as the ViT
        left them — [B, Te, width], or [B*Te, width] for this model's ViT (``forward_both``'s second result).  Caption p
        describes image ``image_index[p]`` (default: image p), or, in image-major order, image j owns captions
        group_start[j] .. group_start[j+1]-1.  As in the reference the strings contain the prompt; add_prompt=True
        prepends it.  The first ``prompt_length`` tokens are not scored; the closing [SEP] is.
        reduction='none': (loss f32 [P] summed per caption — models/med.py:916-917 —, target-token counts i32 [P]); a caption
        that truncates to no target token scores 0 with count 0.  reduction='mean': the 0-dim f32 mean over all target tokens
        (what ``forward`` returns).  label_smoothing=0.0 gives plain negative log-likelihood sums."""
        if reduction not in ("none", "mean"):
            raise ValueError(f"caption_nll: reduction={reduction!r} (none | mean)")
        x = image_or_enc16
        require_cuda(x, "BLIP_Decoder.caption_nll")
        if x.dim() == 4:
            B = x.shape[0]
            _, enc16 = self.visual_encoder.forward_both(x)
        elif x.dim() == 3:
            B, enc16 = x.shape[0], x.reshape(-1, x.shape[-1])
        elif x.dim() == 2:
            Te = self.visual_encoder.patch_embed.num_patches + 1
            if x.shape[0] % Te:
                raise ValueError(f"caption_nll: {x.shape[0]} image-token rows are not a multiple of this ViT's {Te} tokens per image")
            B, enc16 = x.shape[0] // Te, x
        else:
            raise ValueError(f"caption_nll: images [B,3,S,S] or image tokens [B,Te,width] / [B*Te,width] expected, got {tuple(x.shape)}")
        captions = [self.prompt + c for c in captions] if add_prompt else list(captions)
        ids, lens = self.tokenize_captions(captions)
        res = self.text_decoder.score(enc16.contiguous(), B, ids, lens, image_index=image_index, group_start=group_start,
                                      label_smoothing=label_smoothing, prompt_length=self.prompt_length)
        if reduction == "none":
            return res.loss_sum, res.count
        return (res.token_loss.double().sum() / max(1, res.token_loss.numel())).float()

    @torch.no_grad()
    def forward(self, image, caption):
        """Reference: models/blip.py:104-125 — the label-smoothed (0.1) language-model loss of the given captions, one per
        image, averaged over their target tokens.  Returns a 0-dim f32 tensor on the device (no backward pass)."""
        return self.caption_nll(image, caption, label_smoothing=0.1, reduction="mean")


def blip_decoder(pretrained="", **kwargs):
    """Reference: models/blip.py:269-274."""
    model = BLIP_Decoder(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        assert len(msg.missing_keys) == 0
    return model


class BLIP_Video_Decoder(BLIP_Decoder):
    """models/blip.py:169-266: the captioner over ``video_representation: concat_frame``.  Same members, parameter names and
    checkpoint as BLIP_Decoder; the ViT runs over the B*N frames and a video's N*T token rows, contiguous as the ViT leaves
    them, are ONE encoder sequence for the decoder's cross-attention (:199-200, 224-225) — no copy.

    A search presents num_beams rows per video on every decode step (4 on the shared prompt pass) over those N*T keys: the
    DecoderSession keeps the video's K / V in fragment tiles and its cross-attention launches take the key-split form of
    ``vidil_attention`` (kv_tiled = 2) past BertModel.LONG_KEYS keys; up to that many keys (short clips, small
    frames) they are the launches of BLIP_Decoder.  The teacher-forced loss (``forward`` / ``caption_nll``) has more than 32
    rows per video in every launch and runs on the long-key form, as the video-level retrieval and QA heads do."""

    #: read by packing.set_parity_mode / set_compute_dtype: why this model refuses the parity precision mode and fp8
    plain_only = ("video captioning is built for plain f16 / bf16 operands (the attention forms past 768 keys have no "
                  "error-compensated form)")

    def __init__(self, med_config="configs/med_config.json", image_size=384, vit="base", vit_grad_ckpt=False,
                 vit_ckpt_layer=0, prompt="a video of ", tokenizer=None):
        super().__init__(med_config=med_config, image_size=image_size, vit=vit, vit_grad_ckpt=vit_grad_ckpt,
                         vit_ckpt_layer=vit_ckpt_layer, prompt=prompt, tokenizer=tokenizer)

    # ------------------------------------------------------------------ refusals, by name, before anything is launched
    def _require_plain(self):
        V.require_plain(self, "BLIP_Video_Decoder", "video captioning", "the attention forms past 768 keys have no error-compensated form")

    def _require_video_tokens(self, n_tokens):
        V.require_video_tokens(n_tokens, "BLIP_Video_Decoder")

    # ------------------------------------------------------------------ frames -> tokens
    def video_tokens(self, video):
        """f32 [B,N,3,S,S] (normalised) -> 16-bit [B*N*T, width] (video.frame_tokens), video.VIT_VIDEOS videos per ViT pass."""
        self._require_plain()
        return V.frame_tokens(self.visual_encoder, video, who="BLIP_Video_Decoder.video_tokens", u8=False, videos_per_pass=V.VIT_VIDEOS)

    def video_tokens_u8(self, frames_u8):
        """uint8 [B,N,S,S,3] frames (already S x S) -> the same, with /255 and the normalisation fused into the patch kernel."""
        self._require_plain()
        return V.frame_tokens(self.visual_encoder, frames_u8, who="BLIP_Video_Decoder.video_tokens_u8", u8=True, videos_per_pass=V.VIT_VIDEOS)

    def _tokens(self, video):
        """(16-bit tokens [B*Te, width], B) of f32 [B,N,3,S,S] / uint8 [B,N,S,S,3] frames, or of token rows [B, Te, width]."""
        if video.dim() == 3:
            require_cuda(video, "BLIP_Video_Decoder")
            return video.reshape(-1, video.shape[-1]), video.shape[0]
        tok = self.video_tokens_u8(video) if video.dtype == torch.uint8 else self.video_tokens(video)
        return tok, video.shape[0]

    # ------------------------------------------------------------------ searches over N*T keys per video
    def videos_per_block(self, tokens_per_video):
        """Videos searched side by side by ``generate``: what video.KV_BLOCK_BYTES holds of this decoder's cross K / V."""
        return V.videos_per_block(self.text_decoder.config, tokens_per_video)

    def _check_tokens(self, enc16, B):
        self._require_plain()
        V.video_rows(enc16, B, "BLIP_Video_Decoder")

    @torch.no_grad()
    def generate_ids(self, enc16, B, **kw):
        """BLIP_Decoder.generate_ids over B videos of enc16.shape[0] / B tokens each (at most MAX_VIDEO_TOKENS)."""
        self._check_tokens(enc16, B)
        return super().generate_ids(enc16, B, **kw)

    @torch.no_grad()
    def sample_ids(self, enc16, B, **kw):
        self._check_tokens(enc16, B)
        return super().sample_ids(enc16, B, **kw)

    @torch.no_grad()
    def generate(self, video, sample=False, num_beams=3, max_length=30, min_length=10, top_p=0.9, repetition_penalty=1.0,
                 videos_per_block=None, details=None, seed=None):
        """Reference: models/blip.py:221-266.  video f32 [B,N,3,S,S] (normalised) or uint8 [B,N,S,S,3] on the GPU -> list of B
        captions.  As there, ``sample=True`` draws with repetition penalty 1.1 whatever ``repetition_penalty`` says (:249).
        The videos are searched ``videos_per_block`` at a time (default: ``self.videos_per_block``); a search is per video
        and every kernel's arithmetic is independent of the batch around a row, so a caption does not depend on the block it
        falls in (``sample=True``: one ``seed`` for the call — default: a fresh one, as sample_ids draws it — and the video's
        index in the call as its Philox row).  ``details`` (dict, optional; what the tests compare): receives ``tokens`` i32
        [B, max_length] on the host."""
        if not sample:
            K.require_num_beams(num_beams, "BLIP_Video_Decoder.generate")   # (before the ViT runs)
        tok16, B = self._tokens(video)
        if sample and seed is None:
            seed = self._fresh_seed()
        Te = tok16.shape[0] // B
        per = self.videos_per_block(Te) if videos_per_block is None else int(videos_per_block)
        if per < 1:
            raise ValueError(f"BLIP_Video_Decoder: videos_per_block={videos_per_block}")
        parts = []
        for b0 in range(0, B, per):
            b1 = min(B, b0 + per)
            blk = tok16[b0 * Te:b1 * Te]
            if sample:
                parts.append(self.sample_ids(blk, b1 - b0, top_p=top_p, max_length=max_length, min_length=min_length, seed=seed,
                                             row_offset=b0))
            else:
                parts.append(self.generate_ids(blk, b1 - b0, num_beams=num_beams, max_length=max_length, min_length=min_length,
                                               repetition_penalty=repetition_penalty)[0].clone())
        out_tok = parts[0] if len(parts) == 1 else torch.cat(parts)
        if details is not None:
            details["tokens"] = out_tok.cpu()
        return self.decode_captions(out_tok)

    # ------------------------------------------------------------------ scoring given captions
    @torch.no_grad()
    def caption_nll(self, video_or_tokens, captions, video_index=None, *, group_start=None, add_prompt=False,
                    label_smoothing=0.1, reduction="none"):
        """BLIP_Decoder.caption_nll for videos: f32 [B,N,3,S,S] / uint8 [B,N,S,S,3] frames (the ViT runs once per frame) or their
        token rows [B, N*T, width].  Caption p describes video ``video_index[p]`` (default: video p), or video j owns captions
        group_start[j] .. group_start[j+1]-1.  Every launch of the teacher-forced pass has more than 32 query rows per video."""
        x = video_or_tokens
        if x.dim() not in (3, 5):
            raise ValueError(f"BLIP_Video_Decoder.caption_nll: videos [B,N,3,S,S] / [B,N,S,S,3] or video tokens [B,N*T,width] "
                             f"expected, got {tuple(x.shape)}")
        tok16, B = self._tokens(x)
        self._check_tokens(tok16, B)
        return super().caption_nll(tok16.view(B, -1, tok16.shape[-1]), captions, video_index, group_start=group_start,
                                   add_prompt=add_prompt, label_smoothing=label_smoothing, reduction=reduction)

    @torch.no_grad()
    def forward(self, video, caption):
        """Reference: models/blip.py:196-219 — the label-smoothed (0.1) language-model loss of the given captions, one per video,
        averaged over their target tokens.  Returns a 0-dim f32 tensor on the device (no backward pass)."""
        return self.caption_nll(video, caption, label_smoothing=0.1, reduction="mean")


def blip_decoder_video(pretrained="", **kwargs):
    """Reference: models/blip.py:276-281."""
    model = BLIP_Video_Decoder(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        assert len(msg.missing_keys) == 0
    return model
