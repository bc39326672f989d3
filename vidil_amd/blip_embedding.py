"""BLIP embedding model on the HIP kernels — drop-in for the reference's ``models/blip_embedding.py``
(``blip_embedding(...)``, ``BLIP_Embedding.forward(image, caption, match_head='itc')``).

The reference class has the members of ``BLIP_ITM`` (a ViT, the text encoder, ``vision_proj``, ``text_proj``, ``itm_head``:
models/blip_embedding.py:27-38) and differs in what ``forward`` returns, so it is that class with another ``forward``: both
heads run on ``BLIP_ITM``'s code paths (``itm_pairs``; ``image_embeds`` / ``text_embeds`` / ``kernels.scan_scores``).
"""
from __future__ import annotations

import torch

from . import kernels as K
from .blip import load_checkpoint
from .blip_itm import BLIP_ITM
from .packing import require_cuda
from .tokenizer import refuse_synthetic_with_checkpoint


class BLIP_Embedding(BLIP_ITM):
    @torch.no_grad()
    def forward(self, image, caption, match_head="itc"):
        """models/blip_embedding.py:41-67.  F images f32 [F,3,S,S] on the device, N captions (a bare string: one caption).
        match_head='itm' (N == F): raw ITM logits f32 [F, 2] — ``BLIP_ITM.forward``, bit for bit.
        match_head='itc': (image_feat f32 [F, embed_dim], text_feat f32 [N, embed_dim], sim f32 [F, N]) — the unit-norm
        projections of the two [CLS] states and image_feat @ text_feat.t()."""
        caption = [caption] if isinstance(caption, str) else list(caption)      # (the reference's tokenizer takes a bare string)
        if match_head == "itm":
            return super().forward(image, caption, "itm")
        if match_head != "itc":
            raise ValueError(f"unknown match_head {match_head!r}")
        require_cuda(image, "BLIP_Embedding.forward")
        y32, y16 = self.visual_encoder.forward_both(image)
        image_feat, text_feat = self.itc_features(y16, image.shape[0], caption, image.device, y32=y32)
        return image_feat, text_feat, K.scan_scores(image_feat, text_feat)


def blip_embedding(pretrained="", **kwargs):
    """Reference: models/blip_embedding.py:70-75."""
    model = BLIP_Embedding(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        assert len(msg.missing_keys) == 0
    return model
