"""BLIP caption decoder on the HIP kernels — drop-in for the reference's
``models/blip.py`` on the hot path: ``blip_decoder(pretrained, image_size, vit)``,
``BLIP_Decoder.generate(image, sample=False, num_beams=3, max_length=…, min_length=…)
-> list[str]``, ``init_tokenizer``, ``create_vit``, ``load_checkpoint``.

The whole beam search (log-softmax, EOS ban, top-2k, BeamSearchScorer bookkeeping,
KV-cache reorder) runs on the device; the host only enqueues kernels and reads the
final token ids back once per batch.
"""
from __future__ import annotations

import os
from urllib.parse import urlparse

import torch
import torch.nn as nn

from . import kernels as K
from . import video as V
from .med import BeamArena, BertConfig, BertLMHeadModel, BertModel, CrossKV
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


class DecodeTrace:
    """Optional capture of per-step tensors for parity tests (off on the hot path)."""

    def __init__(self):
        self.logits = []       # f32 [R,V] per forward
        self.cand_scores = []
        self.cand_index = []
        self.scores = None     # f32 [B]: the winning hypothesis' score (sum of log-probabilities / length) as the search reports it


class DecoderSession:
    """Device-resident decoding state of R = B*nb sequences over B images: per-image cross K/V (projected
    once), the append-only self-attention KV arena + ancestry table, and the two forward entry points the beam
    loop needs."""

    def __init__(self, text_decoder, enc16, B, nb, max_length, tiled_cross=False):
        """tiled_cross: keep the image K/V in fragment tiles (BertModel.project_cross_kv(tiled=True)) — every decode
        step streams them from HBM once, in whole KiB per wave load; the caller guarantees that no launch has more
        than 32 query rows per image (nb beams x 1 token, or the prompt's tokens)."""
        self.dec, self.bert = text_decoder, text_decoder.bert
        cfg = text_decoder.config
        dev = enc16.device
        self.B, self.nb, self.R = B, nb, B * nb
        self.H, self.L = cfg.num_attention_heads, cfg.num_hidden_layers
        Te = enc16.shape[0] // B
        self.tiled_cross = tiled_cross
        self.cross = self.bert.project_cross_kv(enc16, B, Te, tiled=tiled_cross)
        self.Tcap = max_length
        # (parity precision mode with vidil_attention_f32: the self-attention K / V cache is f32 too)
        from .packing import parity_attention_f32
        arena_dtype = torch.float32 if (self.bert.parity and parity_attention_f32(self.bert)) else enc16.dtype
        self.arena = BeamArena(self.L, self.Tcap, self.R, cfg.hidden_size, dev, dtype=arena_dtype)
        self.ws_prefill, self.ws_step = {}, {}
        self.logits = None
        # round 6: the decoder's post-LN stack without LayerNorm launches (BertModel._run_layers_fused: raw sums + row partials
        # between the GEMMs, the LayerNorms folded into the consuming / residual GEMMs) — a property of the SESSION, never of its
        # size: a caption must not depend on how many images share its search ($VIDIL_DECODE_FUSE_LN=0: the unfused launches)
        self.fused_ln = self.bert.decoder_fused_ln(enc16.dtype)

    @classmethod
    def like(cls, parent, B):
        """A session for ``B`` images with the parent's geometry and EMPTY buffers (no projection): ``adopt`` fills it
        with the state of a subset of the parent's images in the middle of a search."""
        self = cls.__new__(cls)
        self.dec, self.bert = parent.dec, parent.bert
        self.B, self.nb, self.R = B, parent.nb, B * parent.nb
        self.H, self.L = parent.H, parent.L
        self.tiled_cross, self.Tcap = parent.tiled_cross, parent.Tcap
        pc = parent.cross
        self.cross = CrossKV(torch.empty((pc.k.shape[0], B) + tuple(pc.k.shape[2:]), dtype=pc.k.dtype, device=pc.k.device),
                             torch.empty((pc.vt.shape[0], B) + tuple(pc.vt.shape[2:]), dtype=pc.vt.dtype, device=pc.vt.device),
                             B, pc.Te, pc.NP, tiled=pc.tiled, Tk_cap=pc.Tk_cap, f32=pc.f32)
        pa = parent.arena
        self.arena = BeamArena(pa.L, pa.Tcap, self.R, pa.k.shape[-1], pa.k.device, dtype=pa.k.dtype)
        self.ws_prefill, self.ws_step = {}, {}
        self.logits = None
        self.fused_ln = parent.fused_ln
        return self

    def adopt(self, parent, images, n_pos):
        """Take over the search state of the parent's images ``images`` (int64 [B] on the device; entries may repeat:
        padding) after ``n_pos`` cached positions: their cross K/V, their rows of the K/V arena and their ancestry
        rows, with the slot numbers (= beam rows, always rows of the same image) renumbered."""
        nb = self.nb
        j = torch.arange(nb, device=images.device)
        rows = (images[:, None] * nb + j).view(-1)                                        # parent row of each new row
        shift = ((torch.arange(self.B, device=images.device) - images) * nb).repeat_interleave(nb).to(torch.int32)
        self.cross.k.copy_(parent.cross.k.index_select(1, images))
        self.cross.vt.copy_(parent.cross.vt.index_select(1, images))
        self.arena.k[:, :n_pos].copy_(parent.arena.k[:, :n_pos].index_select(2, rows))
        self.arena.v[:, :n_pos].copy_(parent.arena.v[:, :n_pos].index_select(2, rows))
        self.arena._cur = parent.arena._cur                                                # the orientation step graphs expect
        self.arena.anc[:, :n_pos] = parent.arena.anc.index_select(0, rows)[:, :n_pos] + shift[:, None]
        return rows, shift

    def rebind(self, enc16):
        """Start a new search on another batch of the same shape IN THE SAME BUFFERS (cross K/V re-projected in place,
        arena orientation reset): device addresses stay what the captured decode-step graphs recorded."""
        Te = enc16.shape[0] // self.B
        self.cross = self.bert.project_cross_kv(enc16, self.B, Te, out=self.cross, tiled=self.tiled_cross)
        self.arena._cur = 0

    def prefill(self, ids_i32, P, shared=False):
        """Prompt pass.  shared=False: ids_i32 int32 [R*P], every row decoded -> logits f32 [R,V] (what HF
        generate() does).  shared=True: ids_i32 int32 [B*P], ONE row per image -> logits f32 [B,V]: the nb beams of
        an image are identical until the first beam update (models/blip.py:130-138 repeats the same prompt and
        image nb times), so their prompt pass is computed once and its K/V are stored once (arena slot b*nb, which
        the ancestry rows of all nb beams point at)."""
        rows = self.B if shared else self.R
        h32, h16 = self.bert.embed(ids_i32, P, 0)
        # the prompt block attends to itself through one scratch K / V^T pair shared by all layers
        sk, sv, NPp = self.bert.scratch_kv(rows, P, h16.dtype, ids_i32.device)
        self.arena.init_prompt(P, self.nb if shared else 1)
        self.bert.run_layers(h32, h16, rows=rows, T=P, self_k=sk, self_vt=sv, t_off=0, Tk_cap=P, NPs=NPp, causal=True,
                             kv_len=None, cross=self.cross, cross_group=1 if shared else self.nb, ws=self.ws_prefill,
                             arena=self.arena, arena_slot_stride=self.nb if shared else 1, fused=self.fused_ln,
                             arena_prompt=(P == 1 and shared))   # (a shared one-token prompt is still a prompt block: slot b*nb)
        return self.dec.lm_logits(h16, rows, P, h32=h32)

    def step(self, next_tok_i32, beam_idx_i32, past_len):
        """Re-point the beams at their new histories (``beam_idx``: models/med.py:951-955 _reorder_cache, here a
        reorder of the ancestry table only), then one cached forward of the single new token at position
        ``past_len``.  Returns logits f32 [R,V]."""
        self.arena.reorder(beam_idx_i32, past_len)
        h32, h16 = self.bert.embed(next_tok_i32, 1, past_len)
        self.bert.run_layers(h32, h16, rows=self.R, T=1, self_k=None, self_vt=None, t_off=past_len, Tk_cap=self.Tcap,
                             NPs=0, causal=False, kv_len=None, cross=self.cross, cross_group=self.nb, ws=self.ws_step,
                             arena=self.arena, fused=self.fused_ln)
        self.logits = self.dec.lm_logits(h16, self.R, 1, out=self.logits, h32=h32)
        return self.logits


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


class BLIP_Decoder(nn.Module):
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

    # ------------------------------------------------------------------ beam decode
    @torch.no_grad()
    def generate_ids(self, enc16, B, *, num_beams=3, max_length=30, min_length=10, trace: DecodeTrace = None,
                     check_done_every=2, streams=1, compact_min=256, repetition_penalty=1.0):
        """enc16: f16 [B*Te, width] image tokens of B images.  Returns (tokens i32 [B,max_length], lens i32 [B]):
        best hypothesis incl. the prompt, then [SEP] if it fits, then [PAD].

        ``streams`` > 1: the images are cut into that many contiguous parts whose searches run side by side on their
        own HIP streams (``_beam_search`` is a generator that yields after queueing each step; the parts are stepped
        round robin).  Measured at 3,072 images: 2 parts +0.2 %, 3 parts -1.4 %, 4 parts -3.8 % of the whole step — the
        ~160 launches of a decode step are short but each already covers the chip (decode time scales ~1/CUs under a
        CU mask), so the default stays 1; kept for small batches per part of a larger job.
        A search is per image, so the tokens do not depend on the split.

        ``repetition_penalty`` != 1.0 (models/blip.py:127,161; the captioning call site leaves it at 1.0): the candidate
        selection of every step penalises the log-probabilities of the tokens a beam already holds, prompt included
        (``vidil_logsoftmax_topk_penalty``; oracle/beam_ref.py ``repetition_penalty``)."""
        require_cuda(enc16, "BLIP_Decoder.generate")
        K.require_num_beams(num_beams, "generate")          # (1..K.MAX_BEAMS; refused here, not in the middle of a search)
        if not repetition_penalty > 0:
            raise ValueError(f"repetition_penalty must be a strictly positive float, got {repetition_penalty}")   # (HF's message)
        kw = dict(num_beams=num_beams, max_length=max_length, min_length=min_length, check_done_every=check_done_every,
                  compact_min=compact_min, repetition_penalty=float(repetition_penalty))
        if streams <= 1 or trace is not None or B < 2 * streams:
            g = self._beam_search(enc16, B, trace=trace, slot=0, **kw)
            while True:
                try:
                    next(g)
                except StopIteration as done:
                    return done.value
        main = torch.cuda.current_stream()
        side = self.__dict__.setdefault("_decode_streams", {})
        Te = enc16.shape[0] // B
        bounds = [(B * i // streams, B * (i + 1) // streams) for i in range(streams)]
        fork = torch.cuda.Event()
        fork.record(main)
        gens = []
        for i, (lo, hi) in enumerate(bounds):
            st = side.get((i, enc16.device))
            if st is None:
                st = side[(i, enc16.device)] = torch.cuda.Stream(device=enc16.device)
            st.wait_event(fork)
            gens.append((st, self._beam_search(enc16[lo * Te:hi * Te], hi - lo, slot=i, **kw)))
        results = [None] * streams
        live = list(range(streams))
        while live:
            for i in list(live):
                st, g = gens[i]
                with torch.cuda.stream(st):
                    try:
                        next(g)
                    except StopIteration as done:
                        results[i] = done.value
                        live.remove(i)
        for i, (st, _) in enumerate(gens):
            join = torch.cuda.Event()
            join.record(st)
            main.wait_event(join)
            for t in results[i]:
                t.record_stream(main)
        return torch.cat([r[0] for r in results]), torch.cat([r[1] for r in results])

    def _beam_search(self, enc16, B, *, num_beams, max_length, min_length, trace=None, check_done_every=2, slot=0,
                     compact_min=256, repetition_penalty=1.0):
        """Generator: queues the prompt pass and one decode step per ``next()`` on the current stream, returns
        (tokens, lens) through StopIteration."""
        dec, bert = self.text_decoder, self.text_decoder.bert
        cfg = dec.config
        tok = self.tokenizer
        eos, pad = tok.sep_token_id, tok.pad_token_id
        dev = enc16.device
        nb = num_beams
        V = cfg.vocab_size
        # Session state (KV arena, cross K/V, beam buffers) is kept per shape (and per stream slot) and reused by the
        # next batch: besides saving the allocations it keeps every device address stable, which is what lets the
        # decode steps — ~160 launches of 8-30 us kernels each, issued faster by the GPU than Python can enqueue them
        # — be captured once into HIP graphs (one per step index: the position is baked into the launches) and replayed.
        prompt = self.prompt_ids(B, dev)
        P = prompt.shape[1]
        rp = float(repetition_penalty)             # (part of the session keys: the step graphs bake it into their launches)
        key = (B, nb, max_length, min_length, str(dev), enc16.shape[0] // B, P, rp, slot)
        cache = self.__dict__.setdefault("_decode_state", {})
        st = cache.get(key)
        packs = (dec.packed(), bert.packed())     # captured graphs hold the addresses of these packed weights
        if st is not None and not (st["packs"][0] is packs[0] and st["packs"][1] is packs[1]):
            st = None                              # parameters changed since the capture (e.g. a checkpoint was loaded)
        if st is None:
            if len(cache) >= 8:
                # make room: the compact sessions first (each holds its own cross K/V, arena and step graphs — roughly
                # +1.6x of a main session's memory over the four bucket sizes — and is cheap to rebuild); if that was not
                # enough, the LEAST RECENTLY USED main sessions go, one at a time, until there is room — the sessions a
                # pipeline alternates between keep their captured step graphs when an eighth shape shows up (ADVICE r2:
                # this used to be cache.clear())
                for k_ in [k_ for k_ in cache if isinstance(k_[-1], tuple)]:
                    del cache[k_]
                while len(cache) >= 8:
                    del cache[min(cache, key=lambda k_: cache[k_].get("last_used", 0))]
            # (the shared prompt pass has P query rows per image, a decode step nb)
            st = cache[key] = dict(sess=DecoderSession(dec, enc16, B, nb, max_length, tiled_cross=P <= 32 and nb <= 32),
                                   bufs=K.BeamBuffers(B, nb, max_length, dev), graphs={}, pool=None, calls=0, packs=packs,
                                   graphs_ok=os.environ.get("VIDIL_DECODE_GRAPHS", "1") != "0",
                                   n_done_host=torch.zeros((1,), dtype=torch.int32, pin_memory=True))
        else:
            st["sess"].rebind(enc16)
        self.__dict__["_decode_clock"] = st["last_used"] = self.__dict__.get("_decode_clock", 0) + 1
        st["calls"] += 1
        st["bufs"].reset(prompt)
        # `cur`: the session the loop is driving — the full batch, or (after compaction, below) a smaller session that
        # adopted the images that are still searching
        cur = dict(st=st, sess=st["sess"], bufs=st["bufs"], B=B,
                   use_graphs=st["graphs_ok"] and trace is None and st["calls"] >= 2)    # the first batch warms every kernel up

        def first_unit(logits):
            bufs = cur["bufs"]
            cs, ci = K.logsoftmax_topk(logits, bufs.beam_scores, B, nb, eos if P < min_length else -1, beams_in_logits=1,
                                       seqs=bufs.seqs if rp != 1.0 else None, cur_len=P, penalty=rp)
            if trace is not None:
                trace.logits.append(logits.clone()); trace.cand_scores.append(cs.clone()); trace.cand_index.append(ci.clone())
            K.beam_update(bufs, cs, ci, V, P, eos, pad)

        def unit(c):
            """Decode step at length c: forward of the token appended last, candidate selection, beam update."""
            sess, bufs = cur["sess"], cur["bufs"]
            logits = sess.step(bufs.next_tok, bufs.beam_idx, c - 1)
            cs, ci = K.logsoftmax_topk(logits, bufs.beam_scores, cur["B"], nb, eos if c < min_length else -1,
                                       seqs=bufs.seqs if rp != 1.0 else None, cur_len=c, penalty=rp)
            if trace is not None:
                trace.logits.append(logits.clone()); trace.cand_scores.append(cs.clone()); trace.cand_index.append(ci.clone())
            K.beam_update(bufs, cs, ci, V, c, eos, pad)

        # ---- finished images leave the batch (VIDIL_DECODE_COMPACT=0 switches it off) --------------------------------
        # Real captions end at different lengths; an image whose nb hypotheses are complete only burns rows.  When the
        # polled counter says the searching images fit the next smaller bucket (3/4, 1/2, 1/4, 1/8 of B, at least
        # `compact_min` images), they move to a session of that size: cross K/V, arena rows, ancestry rows and beam
        # state are gathered (a few ms at 1,500 images), the finished ones are finalised where they are.  A search is
        # per image and every kernel's arithmetic is independent of the batch around a row, so the tokens do not change.
        # The random-weight benchmark never triggers this (nothing finishes before the length limit).
        compact = compact_min > 0 and trace is None and os.environ.get("VIDIL_DECODE_COMPACT", "1") != "0"
        gran = 64 if compact_min >= 64 else 1                                   # bucket sizes in whole 64-image steps
        buckets = sorted({max(compact_min, -(-(B * f) // (8 * gran)) * gran) for f in (6, 4, 2, 1)}, reverse=True) if compact else []
        buckets = [b for b in buckets if b < B]
        final_tok = final_len = None
        orig = None                                # device int64: original image of each image of the current session

        def retire_and_compact(cur_len):
            """Blocking: read the exact done mask, finalise everything into the result buffers, move the searching images
            into the largest bucket they fit.  Returns False when they do not fit a smaller bucket after all."""
            nonlocal final_tok, final_len, orig
            bufs, sess = cur["bufs"], cur["sess"]
            active = (bufs.done == 0).nonzero().view(-1)                      # (host wait: exact state)
            A = int(active.numel())
            fit = [b for b in buckets if A <= b < cur["B"]]
            if not fit or A == 0:
                return False
            Bp = fit[-1]
            images = torch.cat([active, active[-1:].expand(Bp - A)])           # padding: copies of the last one, marked done
            key2 = (Bp, nb, max_length, min_length, str(dev), enc16.shape[0] // B, P, rp, ("compact", slot))
            st2 = cache.get(key2)
            if st2 is not None and not (st2["packs"][0] is packs[0] and st2["packs"][1] is packs[1]):
                st2 = None
            if st2 is None:
                st2 = cache[key2] = dict(sess=DecoderSession.like(st["sess"], Bp), bufs=K.BeamBuffers(Bp, nb, max_length, dev),
                                         graphs={}, pool=None, calls=0, packs=packs, graphs_ok=st["graphs_ok"],
                                         n_done_host=torch.zeros((1,), dtype=torch.int32, pin_memory=True), last_call=-1)
            if st2.get("last_call") != st["calls"]:                             # one use per search of the parent
                st2["calls"] += 1
                st2["last_call"] = st["calls"]
            rows, shift = st2["sess"].adopt(sess, images, cur_len)
            nb2 = st2["bufs"]
            if getattr(nb2, "swapped", False) != getattr(bufs, "swapped", False):
                nb2.swap()                                                      # same buffer roles as the step graphs saw
            nb2.seqs.copy_(bufs.seqs.index_select(0, rows))
            nb2.beam_scores.copy_(bufs.beam_scores.index_select(0, rows))
            nb2.next_tok.copy_(bufs.next_tok.index_select(0, rows))
            nb2.beam_idx.copy_(bufs.beam_idx.index_select(0, rows) + shift)
            for name in ("done", "n_hyp", "hyp_score", "hyp_len", "hyp_tok", "worst"):
                getattr(nb2, name).copy_(getattr(bufs, name).index_select(0, images))
            nb2.done[A:] = 1
            nb2.n_done.fill_(Bp - A)
            # only now: beam_finalize ADDS the running beams of unfinished images to their hypothesis lists in place
            # (BeamSearchScorer.finalize does), which must not reach the copies made above; the state left behind in
            # the old session is dead — its next search starts with reset()
            out_tok, out_len, _ = K.beam_finalize(bufs, cur_len, eos, pad)
            if final_tok is None:
                final_tok, final_len = out_tok, out_len
                orig = torch.arange(B, device=dev)
            else:
                final_tok[orig] = out_tok[:orig.numel()]
                final_len[orig] = out_len[:orig.numel()]
            orig = orig.index_select(0, active)
            cur.update(st=st2, sess=st2["sess"], bufs=nb2, B=Bp,
                       use_graphs=st2["graphs_ok"] and st2["calls"] >= 2)
            return True

        # ---- prompt pass, once per image: the beams of an image are identical until the first update
        first_unit(cur["sess"].prefill(prompt.contiguous().view(-1), P, shared=True))
        yield
        cur_len = P + 1
        probe = None
        while cur_len < max_length:
            # "every image has its nb finished hypotheses" (BeamSearchScorer.is_done) is polled WITHOUT a host wait: the
            # counter travels to pinned memory behind an event and is looked at when it has arrived.  A step queued
            # after the last image finished changes nothing (finished images are skipped by beam_update, like
            # process() skips done batches, and beam_finalize takes their stored hypotheses).
            if check_done_every and trace is None and cur_len % check_done_every == 0:
                if probe is not None and probe.query():
                    n_done = int(cur["st"]["n_done_host"][0])
                    probe = None
                    if n_done == cur["B"]:
                        break
                    if buckets and max_length - cur_len >= 3 and any(cur["B"] - n_done <= b < cur["B"] for b in buckets):
                        retire_and_compact(cur_len)
                if probe is None:
                    cur["st"]["n_done_host"].copy_(cur["bufs"].n_done, non_blocking=True)
                    probe = torch.cuda.Event()
                    probe.record()
            elif check_done_every and trace is not None and int(cur["bufs"].n_done.item()) == B:
                break                        # parity traces stop exactly where the reference's loop stops
            g = cur["st"]["graphs"].get(cur_len) if cur["use_graphs"] else None
            if g is not None:
                g.replay()
                cur["sess"].arena._cur ^= 1      # the host-side halves of arena.reorder() and beam_update()
                cur["bufs"].swap()
            elif cur["use_graphs"]:
                try:
                    g = torch.cuda.CUDAGraph()
                    # thread_local: other threads (the RCCL watchdog of a multi-GPU run) may touch the runtime meanwhile
                    with torch.cuda.graph(g, pool=cur["st"]["pool"], capture_error_mode="thread_local"):
                        unit(cur_len)
                    cur["st"]["pool"] = g.pool()
                    cur["st"]["graphs"][cur_len] = g
                    g.replay()            # capture records, replay executes (host-side state already advanced)
                except Exception as e:    # capture unsupported here: finish this batch with plain launches, loudly
                    import warnings
                    warnings.warn(f"vidil_amd: decode-step graph capture failed ({e!r}); continuing without graphs")
                    torch.cuda.synchronize()
                    for s_ in cache.values():
                        s_["graphs_ok"] = False
                        s_["graphs"].clear()
                    inner = self._beam_search(enc16, B, num_beams=num_beams, max_length=max_length, min_length=min_length,
                                              trace=trace, check_done_every=check_done_every, slot=slot, compact_min=compact_min,
                                              repetition_penalty=rp)
                    return (yield from inner)
            else:
                unit(cur_len)
            cur_len += 1
            yield
        out_tok, out_len, out_score = K.beam_finalize(cur["bufs"], cur_len, eos, pad)
        if trace is not None:
            trace.scores = out_score          # (a traced search never compacts: one score per image)
        if final_tok is None:
            return out_tok, out_len
        final_tok[orig] = out_tok[:orig.numel()]
        final_len[orig] = out_len[:orig.numel()]
        return final_tok, final_len

    # ------------------------------------------------------------------ nucleus sampling
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
            self._sample_calls = getattr(self, "_sample_calls", 0) + 1
            seed = (torch.initial_seed() + (self._sample_calls << 32)) & 0xFFFFFFFFFFFFFFFF
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
            self._sample_calls = getattr(self, "_sample_calls", 0) + 1
            seed = (torch.initial_seed() + (self._sample_calls << 32)) & 0xFFFFFFFFFFFFFFFF
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
