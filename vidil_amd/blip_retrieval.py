"""BLIP retrieval model on the HIP kernels — the ``--encoder_version blip`` backend of the visual tokenizer
(run_visual_tokenization.py:113-133,152-159,277-293; reference model: models/blip_retrieval.py:14-75).

Inference only: the momentum encoders, the feature queues and the contrastive / matching losses of the reference
class are training state; their checkpoint keys are ignored by ``load_checkpoint`` (``strict=False``, as in the
reference's own factory, which only prints the missing keys).  What the tokenizer uses:

  * ``image_features_u8(frames)``  -> ViT tokens (f16, for the ITM cross-attention) and the unit-norm ITC embedding
    ``normalize(vision_proj(cls))``                                   (get_image_embeddings_blip, :152-159)
  * ``text_features(texts)``       -> unit-norm ``normalize(text_proj(text_encoder(ids, mode='text')[:,0]))`` plus the
    ids (first token replaced by [ENC]) and lengths for the re-rank    (get_text_embeddings_blip, :113-133)
  * ``rerank(...)``                -> ``itm_head(text_encoder(ids, image)[:,0])[:,1]`` for (frame, text) pairs (:283-292)

and, for the video-level retrieval evaluation (eval_retrieval_video.py; vidil_amd/video_retrieval.py):

  * ``video_features_u8(frames)``  -> the tokens of every frame, a video's N*T rows contiguous, and
    ``normalize(mean_frames(vision_proj(cls)))``                       (eval_retrieval_video.py:61-69)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K
from .blip import CLIP_MEAN, CLIP_STD, load_checkpoint
from .blip_itm import ITM_MAX_LENGTH, BLIP_ITM
from .packing import require_cuda
from .tokenizer import refuse_synthetic_with_checkpoint
from .video import frame_tokens


class BLIP_Retrieval(BLIP_ITM):
    def __init__(self, med_config="configs/med_config.json", image_size=384, vit="base", vit_grad_ckpt=False,
                 vit_ckpt_layer=0, embed_dim=256, queue_size=57600, momentum=0.995, negative_all_rank=False,
                 tokenizer=None):
        super().__init__(med_config=med_config, image_size=image_size, vit=vit, vit_grad_ckpt=vit_grad_ckpt,
                         vit_ckpt_layer=vit_ckpt_layer, embed_dim=embed_dim, tokenizer=tokenizer)
        self.temp = nn.Parameter(0.07 * torch.ones([]))      # models/blip_retrieval.py:66 (unused at inference)
        self.queue_size, self.momentum, self.negative_all_rank = queue_size, momentum, negative_all_rank
        # pinned to the plain mode so that the process-wide $VIDIL_PARITY default — meant for the captioner, the filter and CLIP —
        # leaves it as it is; the parity form of this backend is an explicit per-model set_parity_mode(True, model)
        from .packing import set_parity_mode
        set_parity_mode(False, self)

    # ------------------------------------------------------------------ features (BLIP_ITM.image_embeds / text_embeds)
    # In the parity precision mode (set_parity_mode(True, model)) the ViT and the text stack run on error-compensated operands and
    # the two ITC projections take their f32 [CLS] states (BLIP_ITM._project_cls_parity); the image tokens handed to ``rerank``
    # are then the ViT's [hi | lo | hi] rows.

    @torch.no_grad()
    def image_features_u8(self, frames_u8):
        """uint8 [N,S,S,3] -> (image tokens f16 [N*T, width] — [N*T, 3*width] in the parity mode —, unit-norm embeddings f32
        [N, embed_dim])."""
        require_cuda(frames_u8, "BLIP_Retrieval.image_features_u8")
        N = frames_u8.shape[0]
        y32, y16 = self.visual_encoder.forward_u8(frames_u8, CLIP_MEAN, CLIP_STD)
        return y16, self.image_embeds(y32, y16, N)

    @torch.no_grad()
    def image_features(self, image):
        """f32 [N,3,S,S] (normalised) -> same as image_features_u8 (run_visual_tokenization.py:152-159)."""
        require_cuda(image, "BLIP_Retrieval.image_features")
        N = image.shape[0]
        y32, y16 = self.visual_encoder.forward_both(image)
        return y16, self.image_embeds(y32, y16, N)

    # ------------------------------------------------------------------ video level (eval_retrieval_video.py:59-71)
    def _video_embeds(self, y16, B, N):
        """normalize(mean over the N frames of vision_proj(frame [CLS])): the UN-normalised projections are averaged, then
        normalised once (eval_retrieval_video.py:65-67) -> f32 [B, embed_dim]."""
        p = self.packed()
        if p["parity"]:
            raise K.VidilHipError("BLIP_Retrieval: the video-level features are not built for the parity precision mode")
        T, C = y16.shape[0] // (B * N), y16.shape[-1]
        proj = torch.empty((B * N, p["vp_w"].shape[0]), dtype=torch.float32, device=y16.device)
        K.gemm(y16.view(-1), p["vp_w"], p["vp_b"], out=proj, M=B * N, lda=T * C)
        return K.l2_normalize_rows(proj.view(B, N, -1).mean(dim=1).contiguous())

    @torch.no_grad()
    def video_features_u8(self, frames_u8):
        """uint8 [B,N,S,S,3] -> (frame tokens 16-bit [B*N*T, width], unit-norm video embeddings f32 [B, embed_dim]).  A video's
        N*T token rows are contiguous: as encoder states it is ONE image of N*T tokens (``video_feat.view(B, -1, C)``,
        eval_retrieval_video.py:69; ``itm_pairs(tokens, B, ...)``)."""
        require_cuda(frames_u8, "BLIP_Retrieval.video_features_u8")
        if frames_u8.dim() != 5 or frames_u8.shape[-1] != 3:
            raise K.VidilHipError(f"video_features_u8: uint8 [B,N,S,S,3] expected, got {tuple(frames_u8.shape)}")
        y16 = frame_tokens(self.visual_encoder, frames_u8, who=None, u8=True)
        return y16, self._video_embeds(y16, *frames_u8.shape[:2])

    @torch.no_grad()
    def video_features(self, video):
        """f32 [B,N,3,S,S] (normalised) -> same as video_features_u8 (eval_retrieval_video.py:61-69)."""
        require_cuda(video, "BLIP_Retrieval.video_features")
        if video.dim() != 5 or video.shape[2] != 3:
            raise K.VidilHipError(f"video_features: f32 [B,N,3,S,S] expected, got {tuple(video.shape)}")
        y16 = frame_tokens(self.visual_encoder, video, who=None, u8=False)
        return y16, self._video_embeds(y16, *video.shape[:2])

    @torch.no_grad()
    def text_features(self, texts, device, batch=512):
        """list[str] -> (unit-norm f32 [N,embed_dim], ids i32 [N,35] with the first id := [ENC], lens i32 [N])."""
        embeds, all_ids, all_lens = [], [], []
        for i in range(0, len(texts), batch):
            ids, lens = self.tokenize(texts[i:i + batch])              # padding='max_length', max_length=35
            t_eff = max(1, min(ITM_MAX_LENGTH, int(lens.max().item())))
            d_ids = ids[:, :t_eff].to(device).contiguous()
            embeds.append(self.text_embeds(d_ids, lens.to(device).contiguous()))
            all_ids.append(ids)
            all_lens.append(lens)
        ids = torch.cat(all_ids, 0)
        ids[:, 0] = self.tokenizer.enc_token_id                         # run_visual_tokenization.py:132
        return torch.cat(embeds, 0), ids.to(device), torch.cat(all_lens, 0).to(device)

    @torch.no_grad()
    def rerank(self, y16, n_images, ids, lens, group_start, max_group):
        """ITM logit of class 1 for image-major (frame, text) pairs (see BLIP_ITM.itm_pairs) -> f32 [P]."""
        return self.itm_pairs(y16, n_images, ids, lens, group_start=group_start, max_group=max_group)[:, 1].contiguous()

    @torch.no_grad()
    def forward(self, image, caption, match_head="itm"):
        """models/blip_itm.py:41-67 call shape; 'itc' returns image_feat @ text_feat.t() [F,F]."""
        if match_head == "itm":
            return super().forward(image, caption, match_head)
        if match_head != "itc":
            raise ValueError(f"unknown match_head {match_head!r}")
        _, img = self.image_features(image)
        txt, _, _ = self.text_features(list(caption), image.device)
        return K.scan_scores(img, txt)


def blip_retrieval(pretrained="", **kwargs):
    """Reference: models/blip_retrieval.py:567-573 (prints, does not assert, the missing keys)."""
    model = BLIP_Retrieval(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
    return model
