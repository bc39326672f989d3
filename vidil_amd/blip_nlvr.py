"""BLIP two-image reasoning (NLVR2) on the HIP kernels — drop-in for the reference's ``models/blip_nlvr.py`` at inference:
``blip_nlvr(pretrained, image_size, vit)``, ``BLIP_NLVR.forward(image, text, targets, train=True)``.

One ViT pass over ``cat([image0, image1])`` (:44-46), the sentences tokenised with padding='longest' and NO truncation, first id
:= [ENC] (:48-49), the twin text encoder over both images' tokens with all-ones image masks (:51-57,
``nlvr_encoder.BertModel.encode_twin``), and ``cls_head = Linear(C, C) -> ReLU -> Linear(C, 2)`` on the [CLS] state (:58-59): two
``kernels.gemm`` launches with the ReLU between them as a torch op on [B, C].  ``train=True`` returns the value of
``F.cross_entropy(prediction, targets)`` (no backward pass), ``train=False`` the prediction f32 [B, 2].

The reference's default image_size=480 is served: 30 x 30 + 1 = 901 image tokens go through the long-key form of
``vidil_attention`` in the ViT's self-attention and in the twin cross-attention.  The only limit on the text is the encoder's
position table: longer input is refused by name before anything is launched.

``load_checkpoint`` has the reference's duplication semantics (:88-98): every ``crossattention.self.*`` key of the checkpoint is
also loaded as ``self0.*`` and ``self1.*`` and every ``crossattention.output.dense.*`` as ``dense0.*`` and ``dense1.*`` — how a BLIP
pre-training checkpoint initialises the twins — with the position embedding interpolated and strict=False.  One deviation: the
reference calls ``os.path.isfile`` without importing ``os`` (:80), so there a local path raises NameError; here it loads.

Plain f16 / bf16 operands only: the parity precision mode and fp8 are refused (``plain_only``).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from . import video as V
from .blip import create_vit, is_url, resolve_med_config
from .med import BertConfig
from .nlvr_encoder import BertModel
from .packing import FP8, PackedCache, compute_dtype, fp8_companion, require_cuda, set_compute_dtype, set_parity_mode, v32, w16
from .tokenizer import init_tokenizer, refuse_synthetic_with_checkpoint
from .vit import interpolate_pos_embed


class BLIP_NLVR(PackedCache, nn.Module):
    #: read by packing.set_parity_mode / set_compute_dtype: why this model refuses the parity precision mode and fp8
    plain_only = "two-image reasoning is built for plain f16 / bf16 operands (the twin encoder's folded output GEMM has no error-compensated form)"

    def __init__(self, med_config="configs/med_config.json", image_size=480, vit="base", vit_grad_ckpt=False, vit_ckpt_layer=0,
                 tokenizer=None):
        super().__init__()
        self.visual_encoder, vision_width = create_vit(vit, image_size, vit_grad_ckpt, vit_ckpt_layer, drop_path_rate=0.1)
        self.tokenizer = tokenizer if tokenizer is not None else init_tokenizer()
        med_config = BertConfig.from_json_file(resolve_med_config(med_config))
        med_config.encoder_width = vision_width
        self.text_encoder = BertModel(config=med_config, add_pooling_layer=False)
        C = self.text_encoder.config.hidden_size
        self.cls_head = nn.Sequential(nn.Linear(C, C), nn.ReLU(), nn.Linear(C, 2))
        # pinned to plain 16-bit operands, whatever the process-wide $VIDIL_PARITY / $VIDIL_DTYPE=fp8 defaults are (as BLIP_VQA)
        set_parity_mode(False, self)
        if compute_dtype(self) == FP8:
            set_compute_dtype(fp8_companion(), self)

    def _require_plain(self):
        V.require_plain(self, "BLIP_NLVR", "two-image reasoning", "the twin encoder's folded output GEMM has no error-compensated form")

    def _pack(self):
        c = self.cdt
        return dict(w1=w16(self.cls_head[0].weight, dtype=c), b1=v32(self.cls_head[0].bias),
                    w2=w16(self.cls_head[2].weight, dtype=c), b2=v32(self.cls_head[2].bias))

    # ------------------------------------------------------------------ tokenisation
    def tokenize(self, text):
        """models/blip_nlvr.py:48-49: padding='longest', no truncation, first id := [ENC].  Returns (ids i32 [B, T], lens i32 [B])
        on the host.  More tokens than the encoder's position table holds are refused here, before any launch."""
        enc = self.tokenizer([text] if isinstance(text, str) else list(text), padding="longest", return_tensors="pt")
        ids = enc.input_ids.clone()
        ids[:, 0] = self.tokenizer.enc_token_id
        limit = self.text_encoder.config.max_position_embeddings
        if ids.shape[1] > limit:
            raise ValueError(f"BLIP_NLVR: a sentence of {ids.shape[1]} tokens exceeds the text encoder's {limit} positions "
                             "(the reference does not truncate; shorten the sentence)")
        return ids.to(torch.int32), enc.attention_mask.sum(dim=1).to(torch.int32)

    # ------------------------------------------------------------------ encoder + head
    @torch.no_grad()
    def predict(self, tokens0, tokens1, B, ids, lens, *, groups=None, max_group=0):
        """tokens_j 16-bit [B*Te, width]: the ViT tokens of image j of B pairs; ids i32 [P, T] / lens i32 [P] (``tokenize``).
        Sentence p reasons over pair p, or — ``groups`` i32 [B+1], pair-major order — pair j serves sentences groups[j] ..
        groups[j+1]-1.  Returns the prediction f32 [P, 2] (models/blip_nlvr.py:51-59)."""
        require_cuda(tokens0, "BLIP_NLVR")
        self._require_plain()
        dev = tokens0.device
        te = self.text_encoder
        cross0, cross1 = te.project_twin_kv(tokens0, tokens1, B, tokens0.shape[0] // B)
        _, h16 = te.encode_twin(ids.to(dev).contiguous(), lens.to(dev).to(torch.int32).contiguous(), cross0, cross1,
                                groups=None if groups is None else groups.to(dev), max_group=max_group)
        return self.classify(h16, ids.shape[0], ids.shape[1])

    def classify(self, h16, P, T):
        """cls_head on token 0 of each of P sequences of T rows of h16 [P*T, C] -> f32 [P, 2]."""
        p = self.packed()
        C = h16.shape[-1]
        hid = torch.empty((P, C), dtype=torch.float32, device=h16.device)
        K.gemm(h16.view(-1), p["w1"], p["b1"], out=hid, M=P, lda=T * C)
        act = torch.relu(hid).to(h16.dtype)
        out = torch.empty((P, 2), dtype=torch.float32, device=h16.device)
        K.gemm(act, p["w2"], p["b2"], out=out)
        return out

    def _finish(self, y16, n_images, text, targets, train):
        if n_images % 2:
            raise ValueError(f"BLIP_NLVR: image holds cat([image0, image1]) — an even number of images, got {n_images}")
        B = n_images // 2
        ids, lens = self.tokenize(text)
        if ids.shape[0] != B or (targets is not None and targets.shape[0] != B):
            raise ValueError(f"BLIP_NLVR: {ids.shape[0]} sentences and {None if targets is None else targets.shape[0]} targets for "
                             f"{B} image pairs")
        half = y16.shape[0] // 2
        prediction = self.predict(y16[:half], y16[half:], B, ids, lens)
        if train:
            return F.cross_entropy(prediction, targets.to(prediction.device).long())
        return prediction

    # ------------------------------------------------------------------ the reference's call
    @torch.no_grad()
    def forward(self, image, text, targets, train=True):
        """Reference: models/blip_nlvr.py:42-65.  image f32 [2B,3,S,S] on the GPU = cat([image0, image1]); text: B sentences;
        targets int [B] (may be None with train=False).  train=True: the 0-dim f32 loss, no backward pass; train=False: the
        prediction f32 [B, 2], on the GPU."""
        if train and targets is None:
            raise ValueError("BLIP_NLVR.forward(train=True) needs targets")
        self._require_plain()
        require_cuda(image, "BLIP_NLVR.forward")
        _, y16 = self.visual_encoder.forward_both(image)
        return self._finish(y16, image.shape[0], text, targets, train)

    @torch.no_grad()
    def forward_u8(self, image0_u8, image1_u8, text):
        """uint8 [B,S,S,3] images (already S x S), /255 and the normalisation fused into the patch kernel -> prediction f32 [B, 2]."""
        self._require_plain()
        require_cuda(image0_u8, "BLIP_NLVR.forward_u8")
        if image0_u8.shape != image1_u8.shape or image0_u8.dim() != 4 or image0_u8.shape[-1] != 3 or image0_u8.dtype != torch.uint8:
            raise ValueError(f"BLIP_NLVR.forward_u8: two uint8 [B,S,S,3] tensors expected, got {tuple(image0_u8.shape)} and "
                             f"{tuple(image1_u8.shape)}")
        frames = torch.cat([image0_u8, image1_u8], 0)
        _, y16 = self.visual_encoder.forward_u8(frames, V.CLIP_MEAN, V.CLIP_STD)
        return self._finish(y16, frames.shape[0], text, None, False)


def blip_nlvr(pretrained="", **kwargs):
    """Reference: models/blip_nlvr.py:67-73 (prints the missing keys)."""
    model = BLIP_NLVR(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
    return model


def load_checkpoint(model, url_or_filename):
    """Reference: models/blip_nlvr.py:76-102 — checkpoint['model'], position-embedding interpolation, the twins' duplication
    (``crossattention.self.`` -> self0 / self1, ``crossattention.output.dense.`` -> dense0 / dense1), strict=False.  A local path
    loads (the reference raises NameError there: it never imports os)."""
    if is_url(url_or_filename):
        from torch.hub import load_state_dict_from_url

        checkpoint = load_state_dict_from_url(url_or_filename, map_location="cpu", check_hash=False, progress=True)
    elif os.path.isfile(url_or_filename):
        checkpoint = torch.load(url_or_filename, map_location="cpu")
    else:
        raise RuntimeError("checkpoint url or path is invalid")
    state_dict = checkpoint["model"]
    state_dict["visual_encoder.pos_embed"] = interpolate_pos_embed(state_dict["visual_encoder.pos_embed"], model.visual_encoder)
    for key in list(state_dict.keys()):
        if "crossattention.self." in key:
            state_dict[key.replace("self", "self0")] = state_dict[key]
            state_dict[key.replace("self", "self1")] = state_dict[key]
        elif "crossattention.output.dense." in key:
            state_dict[key.replace("dense", "dense0")] = state_dict[key]
            state_dict[key.replace("dense", "dense1")] = state_dict[key]
    msg = model.load_state_dict(state_dict, strict=False)
    print("load checkpoint from %s" % url_or_filename)
    return model, msg
