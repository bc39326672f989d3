"""BLIP retrieval model on the HIP kernels — the ``--encoder_version blip`` backend of the visual tokenizer
(run_visual_tokenization.py:113-133,152-159,277-293; reference model: models/blip_retrieval.py:14-75).

As built by default the model is the inference half: the momentum encoders and the feature queues of the reference class
are training state; their checkpoint keys are then ignored by ``load_checkpoint`` (``strict=False``, as in the reference's
own factory, which only prints the missing keys).  What the tokenizer uses:

  * ``image_features_u8(frames)``  -> ViT tokens (f16, for the ITM cross-attention) and the unit-norm ITC embedding
    ``normalize(vision_proj(cls))``                                   (get_image_embeddings_blip, :152-159)
  * ``text_features(texts)``       -> unit-norm ``normalize(text_proj(text_encoder(ids, mode='text')[:,0]))`` plus the
    ids (first token replaced by [ENC]) and lengths for the re-rank    (get_text_embeddings_blip, :113-133)
  * ``rerank(...)``                -> ``itm_head(text_encoder(ids, image)[:,0])[:,1]`` for (frame, text) pairs (:283-292)

and, for the video-level retrieval evaluation (eval_retrieval_video.py; vidil_amd/video_retrieval.py):

  * ``video_features_u8(frames)``  -> the tokens of every frame, a video's N*T rows contiguous, and
    ``normalize(mean_frames(vision_proj(cls)))``                       (eval_retrieval_video.py:61-69)

The loss forward (models/blip_retrieval.py:76-251 and, for ``BLIP_Retrieval_Video``, :350-518; forward only, except that
``grads=`` returns the gradients of ``loss_ita`` with respect to the online features and ``temp``, ``head_grads=`` those of the
three heads' parameters and of the [CLS] states they read: vidil_amd/losses.py):
``forward(image | video, caption, alpha=, idx=) -> (loss_ita, loss_itm)``.  Its state — the momentum towers
``visual_encoder_m / vision_proj_m / text_encoder_m / text_proj_m`` and the queues ``image_queue / text_queue / idx_queue /
ptr_queue`` under the reference's names and shapes — is opt-in: ``momentum_state=True`` in the constructor, or
``ensure_momentum_state()`` (which the loss forward calls).  What the reference EXECUTES, restated:

  * the index-based targets of :100-104 are overwritten by the diagonal at :126-127, so in both classes the hard targets are the
    diagonal and ``idx_queue`` is maintained but never enters the loss;
  * with s = a·K / temp (student row against the other modality's momentum batch features followed by the queue) and
    m = a_m·K / temp (the momentum row), a row's loss is  lse(s) - alpha * sum_j softmax(m)_j s_j - (1 - alpha) * s_diag
    because the targets sum to 1.  ``kernels.scan_softmax_stats`` reads K once and returns per row and per segment (batch,
    queue) the maxima, the two sums of exponentials and the weighted sum; no [B, B + queue] matrix is written;
  * the queue lives row-major behind ``QUEUE_HEAD`` rows kept for the batch features (``image_queue`` is the transposed view of
    rows QUEUE_HEAD.. of that buffer), so a call neither concatenates nor transposes it;
  * hard negatives: torch.multinomial's stream cannot be reproduced, so a draw follows this library's Philox contract
    (csrc/sample.hip): u = philox_uniform(seed, row, stream) with stream 0 for text -> image and 1 for image -> text, the
    weights are the f32 softmax of the in-batch similarities with same-``idx`` entries zeroed, c = cumsum in index order and
    the draw is the first j with c_j > u * c_last.  ``negatives=`` replays given draws.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from . import kernels as K
from . import losses
from .blip import CLIP_MEAN, CLIP_STD, load_checkpoint
from .blip_itm import ITM_MAX_LENGTH, BLIP_ITM
from .packing import require_cuda, v32, w16
from .tokenizer import refuse_synthetic_with_checkpoint
from .video import frame_tokens, group_table, require_plain

QUEUE_HEAD = losses.QUEUE_HEAD     # rows of a key buffer in front of the queue: a call's batch features live in rows [0, B)
MOMENTUM_PAIRS = (("visual_encoder", "visual_encoder_m"), ("vision_proj", "vision_proj_m"),
                  ("text_encoder", "text_encoder_m"), ("text_proj", "text_proj_m"))       # models/blip_retrieval.py:53-57
_MODE_FLAGS = ("_compute_dtype", "_parity", "_parity_attn")


def philox_uniform(seed, rows, stream, device):
    """This library's draw contract (csrc/sample.hip, oracle/sample_ref.py) for ``rows`` (int tensor) on the device:
    u = (Philox4x32-10(key = seed, counter = (row, stream, 0, 0))[0] >> 8) * 2^-24 -> f32 in [0, 1).  32 x 32 -> 64-bit products
    are taken in two 16-bit halves of the counter word, so that nothing exceeds int64."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF

    def mulhilo(m, c):
        a, b = m * (c & 0xFFFF), m * (c >> 16)
        low = a + ((b & 0xFFFF) << 16)
        return ((b >> 16) + (low >> 32)) & MASK, low & MASK

    rows = rows.to(device=device, dtype=torch.int64)
    c = [rows & MASK, torch.full_like(rows, int(stream) & MASK), torch.zeros_like(rows), torch.zeros_like(rows)]
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        hi0, lo0 = mulhilo(M0, c[0])
        hi1, lo1 = mulhilo(M1, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (c[0] >> 8).to(torch.float32) * (1.0 / 16777216.0)


class BLIP_Retrieval(BLIP_ITM):
    def __init__(self, med_config="configs/med_config.json", image_size=384, vit="base", vit_grad_ckpt=False,
                 vit_ckpt_layer=0, embed_dim=256, queue_size=57600, momentum=0.995, negative_all_rank=False,
                 tokenizer=None, momentum_state=False):
        super().__init__(med_config=med_config, image_size=image_size, vit=vit, vit_grad_ckpt=vit_grad_ckpt,
                         vit_ckpt_layer=vit_ckpt_layer, embed_dim=embed_dim, tokenizer=tokenizer)
        self.temp = nn.Parameter(0.07 * torch.ones([]))      # models/blip_retrieval.py:71
        self.queue_size, self.momentum, self.negative_all_rank = queue_size, momentum, negative_all_rank
        self.embed_dim = embed_dim
        # pinned to the plain mode so that the process-wide $VIDIL_PARITY default — meant for the captioner, the filter and CLIP —
        # leaves it as it is; the parity form of this backend is an explicit per-model set_parity_mode(True, model)
        from .packing import set_parity_mode
        set_parity_mode(False, self)
        if momentum_state:
            self.ensure_momentum_state()

    # ------------------------------------------------------------------ training state (models/blip_retrieval.py:47-73)
    @property
    def has_momentum_state(self):
        return "visual_encoder_m" in self._modules

    def ensure_momentum_state(self):
        """Build, once, what the loss forward needs beyond the inference members, under the reference's names and shapes: the
        momentum towers (copies of the online ones: copy_params) and the queues.  A model built without it keeps today's
        members and state_dict keys; the loss forward calls this."""
        if self.has_momentum_state:
            return self
        dev = self.temp.device
        for name, name_m in MOMENTUM_PAIRS:
            src = getattr(self, name)
            caches = [(m, m.__dict__.pop("_packed_cache")) for m in src.modules() if "_packed_cache" in m.__dict__]
            twin = copy.deepcopy(src)                                   # (without the packed operands: they are not state)
            for m, cache in caches:
                m.__dict__["_packed_cache"] = cache
            for a, b in zip(src.modules(), twin.modules()):            # the precision mode the constructor / the user pinned
                for flag in _MODE_FLAGS:
                    if flag in a.__dict__:
                        b.__dict__[flag] = a.__dict__[flag]
            setattr(self, name_m, twin)
        self.copy_params()
        D, Q = self.embed_dim, self.queue_size
        for name in ("image_queue", "text_queue"):                      # unit columns of randn (:61-67), stored as rows
            store = torch.empty((QUEUE_HEAD + Q, D), dtype=torch.float32, device=dev)
            store[:QUEUE_HEAD] = 0
            store[QUEUE_HEAD:] = nn.functional.normalize(torch.randn(D, Q), dim=0).t().to(dev)
            self.__dict__["_store_" + name] = store
            self.register_buffer(name, store[QUEUE_HEAD:].t())
        self._register_queue_pointers(Q, dev)
        return self

    def _register_queue_pointers(self, Q, dev):
        """The queues' bookkeeping buffers under the reference class's names (BLIP_Pretrain has ``queue_ptr`` and no ids)."""
        self.register_buffer("idx_queue", torch.full((1, Q), -100, device=dev))
        self.register_buffer("ptr_queue", torch.zeros(1, dtype=torch.long, device=dev))

    @property
    def model_pairs(self):
        return [[getattr(self, a), getattr(self, b)] for a, b in MOMENTUM_PAIRS]

    @torch.no_grad()
    def copy_params(self):
        for online, mom in self.model_pairs:
            for param, param_m in zip(online.parameters(), mom.parameters()):
                param_m.requires_grad = False
                param_m.copy_(param)            # (through the parameter: its ``_version`` moves and the packed operands follow)

    @torch.no_grad()
    def _momentum_update(self):
        """param_m = param_m * momentum + param * (1 - momentum) (:262-265), in place: a parameter's ``_version`` moves, so the
        packed operands of the momentum towers are rebuilt by themselves (PackedCache)."""
        for online, mom in self.model_pairs:
            ps, pm = [p.detach() for p in online.parameters()], list(mom.parameters())
            torch._foreach_mul_(pm, self.momentum)
            torch._foreach_add_(pm, torch._foreach_mul(ps, 1. - self.momentum))

    def _key_store(self, name):
        """The row-major buffer [QUEUE_HEAD + queue_size, embed_dim] whose rows QUEUE_HEAD.. the buffer ``name`` views
        transposed; rebuilt (one copy) after the module was moved or its buffer replaced."""
        q = getattr(self, name)
        store = self.__dict__.get("_store_" + name)
        if store is None or store.device != q.device or q.data_ptr() != store[QUEUE_HEAD:].data_ptr() or q.stride() != (1, q.shape[0]):
            store = torch.empty((QUEUE_HEAD + q.shape[1], q.shape[0]), dtype=torch.float32, device=q.device)
            store[:QUEUE_HEAD] = 0
            store[QUEUE_HEAD:] = q.t()
            self.__dict__["_store_" + name] = store
            setattr(self, name, store[QUEUE_HEAD:].t())
        return store

    @torch.no_grad()
    def _dequeue_and_enqueue(self, image_feat, text_feat, idxs):
        """:268-286 at world size 1: columns ptr .. ptr + B of the queues := the momentum features (rows of the key stores)."""
        ptr = self._enqueue_features(image_feat, text_feat, self.ptr_queue)
        self.idx_queue[:, ptr:ptr + image_feat.shape[0]] = idxs.view(1, -1).to(self.idx_queue)

    def _enqueue_features(self, image_feat, text_feat, pointer):
        """Rows ptr .. ptr + B of both key stores := the features, ``pointer`` (the class's pointer buffer) moves on; -> the old ptr."""
        B = image_feat.shape[0]
        if self.queue_size % B:
            raise ValueError(f"{type(self).__name__}: queue_size={self.queue_size} is not a multiple of the batch size {B}")
        ptr = int(pointer)
        self._key_store("image_queue")[QUEUE_HEAD + ptr:QUEUE_HEAD + ptr + B] = image_feat
        self._key_store("text_queue")[QUEUE_HEAD + ptr:QUEUE_HEAD + ptr + B] = text_feat
        pointer[0] = (ptr + B) % self.queue_size
        return ptr

    def _pack(self):
        p = super()._pack()
        if self.has_momentum_state:
            p.update(vp_w_m=w16(self.vision_proj_m.weight, dtype=self.cdt), vp_b_m=v32(self.vision_proj_m.bias),
                     tp_w_m=w16(self.text_proj_m.weight, dtype=self.cdt), tp_b_m=v32(self.text_proj_m.bias))
        return p

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
    def _video_embeds(self, y16, B, N, momentum=False):
        """normalize(mean over the N frames of vision_proj(frame [CLS])): the UN-normalised projections are averaged, then
        normalised once (eval_retrieval_video.py:65-67) -> f32 [B, embed_dim].  ``momentum``: through vision_proj_m."""
        p = self.packed()
        if p["parity"]:
            raise K.VidilHipError("BLIP_Retrieval: the video-level features are not built for the parity precision mode")
        w, b = (p["vp_w_m"], p["vp_b_m"]) if momentum else (p["vp_w"], p["vp_b"])
        T, C = y16.shape[0] // (B * N), y16.shape[-1]
        proj = torch.empty((B * N, w.shape[0]), dtype=torch.float32, device=y16.device)
        K.gemm(y16.view(-1), w, b, out=proj, M=B * N, lda=T * C)
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
    def forward(self, image, caption, match_head="itm", *, alpha=None, idx=None, negatives=None, seed=None, details=None,
                grads=None, head_grads=None):
        """Without ``alpha`` / ``idx``: models/blip_itm.py:41-67 call shape; 'itc' returns image_feat @ text_feat.t() [F,F].
        With both (keywords, as train_retrieval.py passes them): the reference's training forward, models/blip_retrieval.py:76-251
        -> (loss_ita, loss_itm), 0-dim f32 device tensors (see ``loss_forward``, also for ``grads=`` and ``head_grads=``)."""
        if alpha is not None or idx is not None:
            if alpha is None or idx is None:
                raise TypeError(f"{type(self).__name__}.forward: the loss forward needs both alpha= and idx=")
            return self.loss_forward(image, caption, alpha, idx, negatives=negatives, seed=seed, details=details, grads=grads,
                                     head_grads=head_grads)
        if negatives is not None or seed is not None or details is not None or grads is not None or head_grads is not None:
            raise TypeError(f"{type(self).__name__}.forward: negatives= / seed= / details= / grads= / head_grads= belong to the loss "
                            "forward (alpha=, idx=)")
        if match_head == "itm":
            return super().forward(image, caption, match_head)
        if match_head != "itc":
            raise ValueError(f"unknown match_head {match_head!r}")
        _, img = self.image_features(image)
        txt, _, _ = self.text_features(list(caption), image.device)
        return K.scan_scores(img, txt)

    # ------------------------------------------------------------------ the loss forward
    def _visual_side(self, image, momentum):
        """(tokens 16-bit [B*Te, width], unit-norm feature f32 [B, embed_dim]) of the online or the momentum tower."""
        vit = self.visual_encoder_m if momentum else self.visual_encoder
        _, y16 = vit.forward_both(image)
        B = image.shape[0]
        p = self.packed()
        w, b = (p["vp_w_m"], p["vp_b_m"]) if momentum else (p["vp_w"], p["vp_b"])
        return y16, self._project_cls(y16, B, y16.shape[0] // B, w, b)

    def _check_visual_input(self, image, who):
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"{who}: f32 [B,3,S,S] expected, got {tuple(image.shape)}")

    def _itc_direction(self, a, a_m, keys_m, store, alpha, temp):
        """One direction of the soft-target contrastive loss (:123-139) -> (f32 [B] row losses, f32 [B,B] the student rows
        against the batch's momentum keys over temp — the block the diagonal is read from).  a, a_m: the student and the
        momentum rows [B, D] (unit norm); keys_m: the other modality's momentum batch features, written to rows [0, B) of its key
        store, whose queue segment starts at QUEUE_HEAD."""
        return losses.ItcDirection.apply(a, a_m, keys_m, store, alpha, temp, self.queue_size)

    def _itc_losses(self, image_feat, text_feat, image_feat_m, text_feat_m, alpha, temp, grads=None):
        """Both directions (:123-141) -> (loss_ita, loss_i2t, loss_t2i, sim_i2t, sim_t2i), the last two the [B,B] blocks of
        ``_itc_direction``.  grads (dict) receives the gradients of loss_ita only, with respect to ``image_feat``, ``text_feat``
        and ``temp`` — computed here, before the enqueue changes the keys the loss was taken over; the values returned are the
        same bits with and without it."""
        image_store, text_store = self._key_store("image_queue"), self._key_store("text_queue")
        if grads is not None:
            return losses.itc_terms_with_grads(grads, image_feat, text_feat, image_feat_m, text_feat_m, image_store, text_store,
                                               temp, alpha, self.queue_size)
        rows_i2t, sim_i2t = self._itc_direction(image_feat, image_feat_m, text_feat_m, text_store, alpha, temp)
        rows_t2i, sim_t2i = self._itc_direction(text_feat, text_feat_m, image_feat_m, image_store, alpha, temp)
        loss_i2t, loss_t2i = rows_i2t.mean(), rows_t2i.mean()
        return (loss_i2t + loss_t2i) / 2, loss_i2t, loss_t2i, sim_i2t, sim_t2i

    def _draw_negatives(self, sim, idx, seed, stream):
        """One negative column per row of sim f32 [B,B] (already / temp): weights = softmax with same-idx entries zeroed
        (:200-209); the draw is the first j with cumsum_j > u * cumsum_last, u = philox_uniform(seed, row, stream)."""
        return self._draw_from_weights(torch.softmax(sim, dim=1).masked_fill(idx.view(-1, 1) == idx.view(1, -1), 0.0), seed, stream)

    def _draw_from_weights(self, w, seed, stream):
        """The inverse-CDF draw of the Philox contract, one column per row of the weights w f32 [B,B]."""
        B = w.shape[0]
        c = torch.cumsum(w, dim=1)
        empty = (c[:, -1] <= 0).nonzero()
        if empty.numel():
            raise ValueError(f"{type(self).__name__}: row {int(empty[0])} has no admissible negative (every weight of its masked "
                             "softmax is zero)")
        u = philox_uniform(seed, torch.arange(B), stream, w.device)
        return (c <= (u * c[:, -1])[:, None]).sum(1).clamp_(max=B - 1)

    @torch.no_grad()
    def loss_forward(self, image, caption, alpha, idx, *, negatives=None, seed=None, details=None, grads=None, head_grads=None):
        """models/blip_retrieval.py:76-251 (BLIP_Retrieval_Video: :350-518) -> (loss_ita, loss_itm).
        image f32 [B,3,S,S] (video: [B,N,3,S,S]); caption: B strings; alpha: float; idx: int [B] (the sample ids whose equals
        are no negatives of each other).  negatives = (neg_image_of_text, neg_text_of_image), int [B] each: given draws instead
        of this library's own (seed, default 0).  details (dict) receives the features, the in-batch similarities, the draws and
        the ITM logits.  grads (dict) receives ``image_feat``, ``text_feat`` (f32 [B, embed_dim]) and ``temp`` (0-dim f32): the
        gradients of ``loss_ita`` only with respect to the online features and the temperature — what the reference's
        ``loss_ita.backward()`` leaves at those nodes, partial gradients of the total loss; nothing is written to a parameter's
        ``.grad``, and losses, ``details`` and every state change are the bits of the call without it.
        head_grads (dict) receives the backward of the three heads, f32 tensors (``_head_grads_itc`` / ``_head_grads_itm``): of
        ``loss_ita`` ``vision_proj.weight`` / ``.bias``, ``text_proj.weight`` / ``.bias``, ``temp`` and, at the 16-bit [CLS] states
        the two projections read, ``image_cls`` [B·N, width] / ``text_cls`` [B, width]; of ``loss_itm`` ``itm_head.weight`` /
        ``.bias`` and ``itm_cls`` [3B, width] in the pair order of ``_itm_loss``.  It may be combined with ``grads=`` and
        ``details=``, changes no result and no state either, and writes no ``.grad``.  The text stack and the ViT have no
        backward yet: the ``*_cls`` entries are where theirs will start.
        Order of effects as in the reference: temp clamp, online features, EMA, momentum features, ITC loss,
        enqueue, negatives, one ITM pass over the B positive and 2B negative pairs, cross-entropy."""
        who = f"{type(self).__name__}.forward"
        # ---- refusals: before anything is launched or changed
        self._refuse_unserved(image, who)
        B, dev = image.shape[0], image.device
        caption = list(caption)
        idx_host = torch.as_tensor(idx).detach().reshape(-1).cpu().long()
        if len(caption) != B or idx_host.numel() != B:
            raise ValueError(f"{who}: {B} images, {len(caption)} captions and {idx_host.numel()} idx entries")
        self._refuse_batch(B, who)
        same = idx_host.view(-1, 1) == idx_host.view(1, -1)
        if negatives is None:
            lonely = same.all(1).nonzero()
            if lonely.numel():
                raise ValueError(f"{who}: row {int(lonely[0])} has no admissible negative (every sample of the batch shares its idx)")
        else:
            negatives = self._checked_negatives(negatives, same, who, "names a sample of the same idx")
        self.ensure_momentum_state()
        idx_dev = idx_host.to(dev)

        self.temp.clamp_(0.001, 0.5)                                                        # :79
        temp = self.temp.detach().float()
        enc16, image_feat = self._visual_side(image, momentum=False)                          # :81-85
        ids, lens = self.tokenize(caption)                                                  # :88
        t_eff = max(1, min(ITM_MAX_LENGTH, int(lens.max().item())))
        d_ids, d_lens = ids[:, :t_eff].to(dev).contiguous(), lens.to(dev).contiguous()
        captured = {} if head_grads is not None else None
        text_feat = self.text_embeds(d_ids, d_lens, captured)                               # :91-93

        self._momentum_update()                                                             # :109
        _, image_feat_m = self._visual_side(image, momentum=True)                            # :110-111
        p = self.packed()
        _, h16 = self.text_encoder_m.encode(d_ids, d_lens, None)
        text_feat_m = self._project_cls(h16, B, t_eff, p["tp_w_m"], p["tp_b_m"])            # :114-116

        # ---- image-text contrastive loss (:123-141)
        if head_grads is not None and grads is None:
            grads = {}                                                                       # (the head backward starts from them)
        loss_ita, loss_i2t, loss_t2i, _, _ = self._itc_losses(image_feat, text_feat, image_feat_m, text_feat_m, alpha, temp, grads)
        if head_grads is not None:
            self._head_grads_itc(head_grads, grads, self._image_cls_rows(enc16, image), captured["text_cls"])
        self._dequeue_and_enqueue(image_feat_m, text_feat_m, idx_dev)                        # :143-145

        # ---- hard negatives (:199-224) and the matching loss (:148-248)
        sim_i2t = K.scan_scores(image_feat, text_feat) / temp
        sim_t2i = sim_i2t.t().contiguous()
        if negatives is None:
            seed = 0 if seed is None else int(seed)
            neg_image = self._draw_negatives(sim_t2i, idx_dev, seed, 0)                       # a negative image for each text
            neg_text = self._draw_negatives(sim_i2t, idx_dev, seed, 1)                        # a negative text for each image
        else:
            neg_image, neg_text = negatives[0].to(dev), negatives[1].to(dev)
        vl_output, loss_itm = self._itm_loss(enc16, B, ids, lens, neg_image, neg_text, captured)
        if head_grads is not None:
            self._head_grads_itm(head_grads, vl_output, captured["itm_cls"])
        if details is not None:
            details.update(image_feat=image_feat, text_feat=text_feat, image_feat_m=image_feat_m, text_feat_m=text_feat_m,
                           sim_i2t=sim_i2t, sim_t2i=sim_t2i, neg_image_of_text=neg_image, neg_text_of_image=neg_text,
                           itm_logits=vl_output, loss_i2t=loss_i2t, loss_t2i=loss_t2i, temp=temp.clone())
        return loss_ita.float(), loss_itm.float()

    # ------------------------------------------------------------------ pieces of the loss forward (shared with BLIP_Pretrain)
    @staticmethod
    def _image_cls_rows(enc16, image):
        """The 16-bit [CLS] rows vision_proj read: token 0 of every image, or of every frame of every video -> [B·N, width]."""
        rows = image.shape[0] * (image.shape[1] if image.dim() == 5 else 1)
        return enc16.view(rows, -1, enc16.shape[-1])[:, 0].contiguous()

    def _head_grads_itc(self, head_grads, grads, image_cls, text_cls):
        """The backward of vision_proj and text_proj under ``loss_ita`` (losses.proj_head_backward), from the gradients at the
        unit-norm features the ITC backward just reported: the heads' parameters and their [CLS] inputs."""
        p = self.packed()
        d_cls, d_w, d_b = losses.proj_head_backward(grads["image_feat"], image_cls, p["vp_w"], p["vp_b"])
        head_grads.update({"vision_proj.weight": d_w, "vision_proj.bias": d_b, "image_cls": d_cls})
        d_cls, d_w, d_b = losses.proj_head_backward(grads["text_feat"], text_cls, p["tp_w"], p["tp_b"])
        head_grads.update({"text_proj.weight": d_w, "text_proj.bias": d_b, "text_cls": d_cls, "temp": grads["temp"]})

    def _head_grads_itm(self, head_grads, vl_output, itm_cls):
        """The backward of itm_head under ``loss_itm`` (losses.itm_head_backward): B positive pairs, then 2B negative ones."""
        B = vl_output.shape[0] // 3
        labels = torch.cat([torch.ones(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long)]).to(vl_output.device)
        d_cls, d_w, d_b = losses.itm_head_backward(vl_output, labels, itm_cls, self.packed()["itm_w"])
        head_grads.update({"itm_head.weight": d_w, "itm_head.bias": d_b, "itm_cls": d_cls})

    def _refuse_unserved(self, image, who):
        require_cuda(image, who)
        self._check_visual_input(image, who)
        require_plain(self, who, "the loss forward", "its momentum towers and contrastive loss run on plain 16-bit operands")
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError(f"{who}: world size {torch.distributed.get_world_size()} — the all-rank negatives and the "
                                      "gathered queue update are not built (negative_all_rank coincides with the local form at "
                                      "world size 1 only)")

    def _refuse_batch(self, B, who):
        if self.queue_size % B:
            raise ValueError(f"{who}: queue_size={self.queue_size} is not a multiple of the batch size {B}")
        if B > QUEUE_HEAD:
            raise ValueError(f"{who}: batch size {B} exceeds the {QUEUE_HEAD} rows kept for the batch features")

    @staticmethod
    def _checked_negatives(negatives, inadmissible, who, why):
        """negatives = (neg_image_of_text, neg_text_of_image) -> two int64 host tensors [B]; ``inadmissible`` bool [B,B]."""
        B = inadmissible.shape[0]
        negatives = tuple(torch.as_tensor(n).detach().reshape(-1).cpu().long() for n in negatives)
        for name, n in zip(("neg_image_of_text", "neg_text_of_image"), negatives):
            if n.numel() != B or (n < 0).any() or (n >= B).any():
                raise ValueError(f"{who}: negatives: {name} must hold {B} indices in [0, {B})")
            bad = inadmissible[torch.arange(B), n].nonzero()
            if bad.numel():
                raise ValueError(f"{who}: negatives: {name}[{int(bad[0])}] {why}")
        return negatives

    def _itm_loss(self, enc16, B, ids, lens, neg_image, neg_text, capture=None):
        """One ITM pass over the B positive and 2B negative pairs (:148-248) -> (logits f32 [3B,2], the two-class cross-entropy).
        ids / lens: the B captions as tokenised (host); the first id becomes [ENC].  capture (dict): receives ``itm_cls``, the
        16-bit [CLS] rows [3B, width] itm_head read, in the pair order of the logits."""
        dev = enc16.device
        enc_ids = ids.clone()
        enc_ids[:, 0] = self.tokenizer.enc_token_id                                          # :148-149
        ar = torch.arange(B, device=dev)
        # pairs (image, text): B positives, then (negative image, text b), then (image b, negative text)   (:229-233)
        pair_image, pair_text = torch.cat([ar, neg_image, ar]), torch.cat([ar, ar, neg_text])
        Te = enc16.shape[0] // B
        if Te > self.text_encoder.LONG_KEYS:          # image-major through group_start, and back to the order above
            order = torch.argsort(pair_image, stable=True)
            group_start, max_group = group_table(pair_image.cpu(), B)
            sorted_logits = self.itm_pairs(enc16, B, enc_ids, lens, group_start=group_start, max_group=max_group,
                                           pair_text=pair_text[order], capture=capture)
            vl_output = torch.empty_like(sorted_logits)
            vl_output[order] = sorted_logits
            if capture is not None:
                sorted_cls = capture["itm_cls"]
                capture["itm_cls"] = torch.empty_like(sorted_cls)
                capture["itm_cls"][order] = sorted_cls
        else:
            vl_output = self.itm_pairs(enc16, B, enc_ids, lens, image_index=pair_image, pair_text=pair_text, capture=capture)
        itm_labels = torch.cat([torch.ones(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long)]).to(dev)
        return vl_output, nn.functional.cross_entropy(vl_output, itm_labels)                # :246-248


class BLIP_Retrieval_Video(BLIP_Retrieval):
    """models/blip_retrieval.py:288-554: the retrieval model whose visual side is a video of N frames — the feature is
    normalize(mean_frames(vision_proj(cls))) and a video's N*T tokens are ONE encoder sequence for the matching head (past
    BertModel.LONG_KEYS keys its pairs go image-major through ``group_start``)."""

    @torch.no_grad()
    def forward(self, video, caption, alpha, idx, *, negatives=None, seed=None, details=None, grads=None, head_grads=None):
        return self.loss_forward(video, caption, alpha, idx, negatives=negatives, seed=seed, details=details, grads=grads,
                                 head_grads=head_grads)

    def _check_visual_input(self, video, who):
        if video.dim() != 5 or video.shape[2] != 3:
            raise ValueError(f"{who}: f32 [B,N,3,S,S] expected, got {tuple(video.shape)}")
        from .video import require_video_tokens
        require_video_tokens(video.shape[1] * (self.visual_encoder.patch_embed.num_patches + 1), type(self).__name__)

    def _visual_side(self, video, momentum):
        y16 = frame_tokens(self.visual_encoder_m if momentum else self.visual_encoder, video, who=None, u8=False)
        return y16, self._video_embeds(y16, *video.shape[:2], momentum=momentum)


def blip_retrieval_video(pretrained="", **kwargs):
    """Reference: models/blip_retrieval.py:559-565."""
    model = BLIP_Retrieval_Video(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
    return model


def blip_retrieval(pretrained="", **kwargs):
    """Reference: models/blip_retrieval.py:567-573 (prints, does not assert, the missing keys)."""
    model = BLIP_Retrieval(**kwargs)
    if pretrained:
        refuse_synthetic_with_checkpoint(model.tokenizer, pretrained)
        model, msg = load_checkpoint(model, pretrained)
        print("missing keys:")
        print(msg.missing_keys)
    return model
