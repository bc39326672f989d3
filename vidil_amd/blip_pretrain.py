"""BLIP pretraining models on the HIP kernels, forward only — drop-in for the reference's ``models/blip_pretrain.py``:
``BLIP_Pretrain`` / ``BLIP_Pretrain_Video`` and their factories, whose ``forward(image | video, caption, alpha)`` returns
``(loss_ita, loss_itm, loss_lm)`` as pretrain_video.py:110 reads them.

One ViT pass serves three losses:

  * ITC — the soft-target contrastive loss over batch + queue of ``BLIP_Retrieval`` (``_itc_direction``: the exact-f32 scan's
    stats form), with the class's momentum towers, EMA and queues; the pointer buffer is ``queue_ptr`` and there are no sample ids.
    ``grads=`` returns its gradients with respect to the online features and ``temp`` (vidil_amd/losses.py), the only backward so far;
  * ITM — one pass over the B positive and 2B hard-negative pairs (``BLIP_Retrieval._itm_loss``).  Unlike the retrieval class the
    weights of a draw come from the student-against-MOMENTUM similarities the contrastive loss already formed (the first B columns
    of sim_t2i / sim_i2t, :155-158): softmax + 1e-4, diagonal zeroed, no id masking;
  * LM — the teacher-forced label-smoothed loss of ``BertLMHeadModel.score`` on the same ViT tokens (first id := [DEC], pads
    ignored, mean over the target tokens, :199-211).

The text encoder and the decoder trunk SHARE every parameter except their self-attention blocks (``tie_encoder_decoder_weights``,
:94,526-595): ``text_encoder.<name>`` is the decoder's ``Parameter`` object for every name that is not under ``attention.``, so
``state_dict()`` lists such a tensor under both names and ``parameters()`` yields it once.  The momentum text encoder is an untied
copy; the EMA reads the shared tensors through ``text_encoder.parameters()``.

The constructor fetches nothing (the reference initialises from DeiT and bert-base-uncased downloads, :40-55,92): weights start
random-init and come from a checkpoint (``blip_pretrain_from_pretrained`` / ``blip_video_pretrain``).  Captions are tokenised to 30
tokens (:105), not the matching head's 35.
"""
from __future__ import annotations

import copy

import torch

from .blip import load_checkpoint
from .blip_retrieval import BLIP_Retrieval, BLIP_Retrieval_Video
from .med import BertLMHeadModel
from .packing import PackedCache, set_parity_mode
from .tokenizer import refuse_synthetic_with_checkpoint
from .video import phase_timer

PRETRAIN_MAX_LENGTH = 30          # models/blip_pretrain.py:105
SELF_ATTENTION = ".attention."    # the one block of a layer that stays the encoder's own (skip_key '/attention', :94)


def tie_encoder_decoder_weights(encoder, decoder):
    """models/blip_pretrain.py:526-595 with base_model_prefix '' and skip_key '/attention', as :94 calls it: every weight and
    bias of ``encoder`` outside a layer's self-attention block becomes the ``Parameter`` object of ``decoder`` under the same
    name.  -> the tied names."""
    mods_e = dict(encoder.named_modules())
    tied = []
    for path, mod_d in decoder.named_modules():
        if SELF_ATTENTION in f".{path}." or path not in mods_e:
            continue
        for name, p in mod_d.named_parameters(recurse=False):
            setattr(mods_e[path], name, p)
            tied.append(f"{path}.{name}")
    return tied


class BLIP_Pretrain(BLIP_Retrieval):
    def __init__(self, med_config="configs/bert_config.json", image_size=224, vit="base", vit_grad_ckpt=False, vit_ckpt_layer=0,
                 embed_dim=256, queue_size=57600, momentum=0.995, tokenizer=None):
        super().__init__(med_config=med_config, image_size=image_size, vit=vit, vit_grad_ckpt=vit_grad_ckpt,
                         vit_ckpt_layer=vit_ckpt_layer, embed_dim=embed_dim, queue_size=queue_size, momentum=momentum,
                         tokenizer=tokenizer)
        cfg = copy.copy(self.text_encoder.config)                    # (a decoder configuration of its own, :90-91)
        self.text_decoder = BertLMHeadModel(config=cfg)              # :90-93
        tie_encoder_decoder_weights(self.text_encoder, self.text_decoder.bert)
        set_parity_mode(False, self)                                 # (the members built here follow the class's pin)
        self.ensure_momentum_state()                                 # the class exists for the loss

    def _adapt_med_config(self, cfg):
        """resize_token_embeddings(len(tokenizer)) (:55,93) before anything is built: the reference's bert_config.json has
        bert-base-uncased's 30,522 entries, its tokenizer two more."""
        cfg.vocab_size = len(self.tokenizer) if hasattr(self.tokenizer, "__len__") else self.tokenizer.vocab_size

    def _register_queue_pointers(self, Q, dev):
        self.register_buffer("queue_ptr", torch.zeros(1, dtype=torch.long, device=dev))       # :80

    def tokenize(self, captions):
        """:105: padding='max_length', truncation, max_length=30; first id stays [CLS]."""
        enc = self.tokenizer(captions, padding="max_length", truncation=True, max_length=PRETRAIN_MAX_LENGTH, return_tensors="pt")
        return enc.input_ids.to(torch.int32), enc.attention_mask.sum(dim=1).to(torch.int32)

    @torch.no_grad()
    def _dequeue_and_enqueue(self, image_feat, text_feat):
        """:231-247 at world size 1."""
        self._enqueue_features(image_feat, text_feat, self.queue_ptr)

    def loss_forward(self, *args, **kwargs):
        raise TypeError(f"{type(self).__name__}: the two-loss forward with idx= is BLIP_Retrieval's; call forward(image, caption, alpha)")

    def _repack_momentum(self):
        """The 16-bit operands of the momentum towers, rebuilt from the parameters the EMA just moved — what their first use
        would do by itself (PackedCache); called apart so that its time can be told from the towers'."""
        for tower in (self.visual_encoder_m, self.text_encoder_m):
            for m in tower.modules():
                if isinstance(m, PackedCache):
                    m.packed()
        return self.packed()

    @torch.no_grad()
    def forward(self, image, caption, alpha, *, negatives=None, seed=None, details=None, timings=None, grads=None,
                head_grads=None):
        """models/blip_pretrain.py:97-212 (BLIP_Pretrain_Video: :328-452) -> (loss_ita, loss_itm, loss_lm), 0-dim
        f32 device tensors.  image f32 [B,3,S,S] (video: [B,N,3,S,S]); caption: B strings; alpha: float.
        negatives = (neg_image_of_text, neg_text_of_image), int [B] each: given draws instead of this library's own Philox draws
        (seed, default 0).  details (dict) receives the four features, ``sim_i2t`` / ``sim_t2i`` (the student rows against the
        batch's momentum features over temp — not transposes of each other), the draws, ``itm_logits`` [3B,2], ``lm_loss_sum`` /
        ``lm_count`` [B] and the per-target ``lm_lp_label`` / ``lm_lp_mean`` / ``lm_caption``, ``loss_i2t`` / ``loss_t2i``, ``temp``.
        timings (dict): seconds per phase from HIP events (video.phase_timer; every phase is synchronised) — ``vit``, ``text``,
        ``ema``, ``repack``, ``momentum``, ``itc``, ``itm``, ``lm``.
        grads (dict) receives ``image_feat``, ``text_feat`` (f32 [B, embed_dim]) and ``temp`` (0-dim f32): the gradients of
        ``loss_ita`` only with respect to the online features and the temperature (partial gradients of the total loss; see
        ``BLIP_Retrieval.loss_forward``).  Losses, ``details`` and every state change are the bits of the call without it.
        head_grads (dict) receives the backward of vision_proj, text_proj (``loss_ita``) and itm_head (``loss_itm``) with the
        keys and rules of ``BLIP_Retrieval.loss_forward``; ``loss_lm`` gets nothing.
        Order of effects as in the reference: temp clamp, online features, EMA, momentum features, ITC loss, enqueue, negatives,
        the ITM pass, the LM pass."""
        who = f"{type(self).__name__}.forward"
        # ---- refusals: before anything is launched or changed
        self._refuse_unserved(image, who)
        B, dev = image.shape[0], image.device
        caption = list(caption)
        if len(caption) != B:
            raise ValueError(f"{who}: {B} {'videos' if image.dim() == 5 else 'images'} and {len(caption)} captions")
        self._refuse_batch(B, who)
        if B == 1:
            raise ValueError(f"{who}: a batch of one has no admissible negative (a sample is no negative of itself)")
        if negatives is not None:
            negatives = self._checked_negatives(negatives, torch.eye(B, dtype=torch.bool), who, "is the row's own index")

        lap = phase_timer(timings)
        t0 = lap()
        self.temp.clamp_(0.001, 0.5)                                                        # :99
        temp = self.temp.detach().float()
        enc16, image_feat = self._visual_side(image, momentum=False)                          # :101-103
        t0 = lap("vit", t0)
        ids, lens = self.tokenize(caption)                                                  # :105
        t_eff = max(1, int(lens.max().item()))
        d_ids, d_lens = ids[:, :t_eff].to(dev).contiguous(), lens.to(dev).contiguous()
        captured = {} if head_grads is not None else None
        text_feat = self.text_embeds(d_ids, d_lens, captured)                               # :107-109
        t0 = lap("text", t0)

        self._momentum_update()                                                             # :113
        t0 = lap("ema", t0)
        p = self._repack_momentum()
        t0 = lap("repack", t0)
        _, image_feat_m = self._visual_side(image, momentum=True)                            # :114-115
        _, h16 = self.text_encoder_m.encode(d_ids, d_lens, None)
        text_feat_m = self._project_cls(h16, B, t_eff, p["tp_w_m"], p["tp_b_m"])            # :118-120
        t0 = lap("momentum", t0)

        # ---- image-text contrastive loss (:123-138) and the enqueue (:140)
        if head_grads is not None and grads is None:
            grads = {}                                                                       # (the head backward starts from them)
        loss_ita, loss_i2t, loss_t2i, sim_i2t, sim_t2i = self._itc_losses(image_feat, text_feat, image_feat_m, text_feat_m, alpha,
                                                                          temp, grads)
        if head_grads is not None:
            self._head_grads_itc(head_grads, grads, self._image_cls_rows(enc16, image), captured["text_cls"])
        self._dequeue_and_enqueue(image_feat_m, text_feat_m)
        t0 = lap("itc", t0)

        # ---- hard negatives (:154-176) and the matching loss (:143-196)
        if negatives is None:
            seed = 0 if seed is None else int(seed)
            neg_image = self._draw_from_weights((torch.softmax(sim_t2i, dim=1) + 1e-4).fill_diagonal_(0), seed, 0)
            neg_text = self._draw_from_weights((torch.softmax(sim_i2t, dim=1) + 1e-4).fill_diagonal_(0), seed, 1)
        else:
            neg_image, neg_text = negatives[0].to(dev), negatives[1].to(dev)
        vl_output, loss_itm = self._itm_loss(enc16, B, ids, lens, neg_image, neg_text, captured)
        if head_grads is not None:
            self._head_grads_itm(head_grads, vl_output, captured["itm_cls"])
        t0 = lap("itm", t0)

        # ---- language modelling on the same tokens (:199-211): every token after [DEC] is a target, the closing [SEP] included
        dec_ids = ids.clone()
        dec_ids[:, 0] = self.tokenizer.bos_token_id
        lm = self.text_decoder.score(enc16, B, dec_ids, lens, label_smoothing=0.1, prompt_length=1)
        loss_lm = (lm.loss_sum.double().sum() / lm.count.sum().clamp_min(1)).float()
        lap("lm", t0)
        if details is not None:
            details.update(image_feat=image_feat, text_feat=text_feat, image_feat_m=image_feat_m, text_feat_m=text_feat_m,
                           sim_i2t=sim_i2t, sim_t2i=sim_t2i, neg_image_of_text=neg_image, neg_text_of_image=neg_text,
                           itm_logits=vl_output, lm_loss_sum=lm.loss_sum, lm_count=lm.count, lm_lp_label=lm.lp_label,
                           lm_lp_mean=lm.lp_mean, lm_caption=lm.caption, loss_i2t=loss_i2t, loss_t2i=loss_t2i, temp=temp.clone())
        return loss_ita.float(), loss_itm.float(), loss_lm


class BLIP_Pretrain_Video(BLIP_Pretrain, BLIP_Retrieval_Video):
    """models/blip_pretrain.py:250-487: the pretraining model over a video of N frames — the feature is
    normalize(mean_frames(vision_proj(cls))) and a video's N*T tokens are ONE encoder sequence for the matching head (image-major
    past BertModel.LONG_KEYS keys) and for the decoder (the long-key attention form)."""

    # (the visual side — frame tokens, the mean-of-frames feature, the token limit — is BLIP_Retrieval_Video's, inherited)

    @torch.no_grad()
    def forward(self, video, caption, alpha, *, negatives=None, seed=None, details=None, timings=None, grads=None,
                head_grads=None):
        return super().forward(video, caption, alpha, negatives=negatives, seed=seed, details=details, timings=timings, grads=grads,
                               head_grads=head_grads)


def _from_pretrained(model, pretrained):
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
    return model


def blip_pretrain(**kwargs):
    """Reference: models/blip_pretrain.py:490-492."""
    return BLIP_Pretrain(**kwargs)


def blip_pretrain_from_pretrained(pretrained=None, **kwargs):
    """Reference: models/blip_pretrain.py:494-500 (prints, does not assert, the missing keys)."""
    return _from_pretrained(BLIP_Pretrain(**kwargs), pretrained)


def blip_video_pretrain(pretrained=None, **kwargs):
    """Reference: models/blip_pretrain.py:502-508."""
    return _from_pretrained(BLIP_Pretrain_Video(**kwargs), pretrained)
