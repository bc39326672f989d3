"""The twin text encoder of BLIP_NLVR on the HIP kernels — mirror of the reference's ``models/nlvr_encoder.py``: a MED text
encoder (``med.BertModel``) whose every cross-attention block is a TWIN (:218-248, :251-324).  Twin j has its own
``crossattention.self{j}.{query,key,value}`` and attends to image j's tokens with the same text hidden states h as queries;
``d_j = output.dense{j}(ctx_j)``; layers 0-5 average, ``u = (d0 + d1) / 2``, layers 6.. merge, ``u = output.merge_layer(cat[d0,
d1])`` (a Linear(2C, C); the activation between them is commented out at :240, so it is linear after linear); then
``h = LayerNorm(u + h)``.  Parameter names are the reference's, so its checkpoints load unchanged.

Schedule differences from the reference (results are the same function):
  * the output side of a twin block is folded at pack time into ONE residual GEMM with K = 2C, ``u = [ctx0 | ctx1] · Wf^T + bf``
    (``fold_twin_output``): averaging layers Wf = ½ [W0 | W1], bf = ½ (b0 + b1) — exact, halving is a power of two —, merge
    layers Wf = [Wm[:, :C] · W0 | Wm[:, C:] · W1], bf = Wm[:, :C] · b0 + Wm[:, C:] · b1 + bm, the products formed in float64
    and rounded once to the operand type.  The two attention launches of a layer write their contexts side by side into one
    [M, 2C] buffer (``kernels.attention(ldo=2C)``);
  * the cross-attention K / V of each side are projected once per image pair per layer (``project_twin_kv``), as plain rows
    (row-major V), and every launch takes the ``group_start`` form with its bound rounded up to more than 32 query rows per
    unit — the form that serves every text length at every token count, past ``LONG_KEYS`` encoder states (901 at the
    reference's 480 x 480) through ``CrossRoute.bound`` / ``CrossRoute.tiled`` and the long-key form of ``vidil_attention``;
  * the stack is ``med.BertModel.run_layers`` on its plain unfused path (LayerNorm launches); only ``cross_block`` differs.

Plain f16 / bf16 operands only: the parity precision mode and fp8 are refused.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import kernels as K
from . import med
from .med import BertConfig, CrossKV, CrossRoute, ModelOutput  # noqa: F401  (BertConfig: the reference imports it from here too)
from .packing import FP8, compute_dtype, parity_mode, require_cuda, v32, w16
from .video import MAX_VIDEO_TOKENS

MERGE_FROM_LAYER = 6             # models/nlvr_encoder.py:259 (hard-coded there)


def fold_twin_output(w0, b0, w1, b1, wm=None, bm=None):
    """(Wf float64 [C, 2C], bf float64 [C]) with [ctx0 | ctx1] · Wf^T + bf = (dense0(ctx0) + dense1(ctx1)) / 2, or — with the
    merge layer's (wm [C, 2C], bm) — = merge_layer(cat[dense0(ctx0), dense1(ctx1)]).  Pure; float64 throughout."""
    w0, b0, w1, b1 = (t.detach().double() for t in (w0, b0, w1, b1))
    C = w0.shape[0]
    if wm is None:
        return torch.cat([w0, w1], 1) * 0.5, (b0 + b1) * 0.5
    wm, bm = wm.detach().double(), bm.detach().double()
    return torch.cat([wm[:, :C] @ w0, wm[:, C:] @ w1], 1), wm[:, :C] @ b0 + wm[:, C:] @ b1 + bm


class _TwinOutput(nn.Module):
    def __init__(self, cfg, merge):
        super().__init__()
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.dense0 = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.dense1 = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        if merge:
            self.merge_layer = nn.Linear(cfg.hidden_size * 2, cfg.hidden_size)


class _TwinAttention(nn.Module):
    def __init__(self, cfg, layer_num):
        super().__init__()
        self.self0 = med._SelfAttn(cfg, True)
        self.self1 = med._SelfAttn(cfg, True)
        self.output = _TwinOutput(cfg, merge=layer_num >= MERGE_FROM_LAYER)


class TwinRoute:
    """The cross-attention side of one twin pass: a ``CrossRoute`` per side — same query batches, same ``group_start`` table,
    each over its own image's K / V — and the [M, 2C] buffer both sides' contexts are written into."""

    def __init__(self, model, cross0, cross1, rows, groups, max_group):
        self.sides = tuple(CrossRoute(model, c, rows, groups=groups, max_group=max_group) for c in (cross0, cross1))
        self.ctx = None

    def contexts(self, M, C, like):
        if self.ctx is None:
            self.ctx = torch.empty((M, 2 * C), dtype=like.dtype, device=like.device)
        return self.ctx


class BertModel(med.BertModel):
    """``med.BertModel`` with twin cross-attention blocks.  The library's own entry is ``encode_twin`` (with ``project_twin_kv``);
    ``forward`` takes the reference's call (models/nlvr_encoder.py:705-722)."""

    #: read by packing.set_parity_mode / set_compute_dtype
    plain_only = "the twin text encoder is built for plain f16 / bf16 operands (its folded output GEMM has no error-compensated form)"

    def __init__(self, config, add_pooling_layer=False):
        super().__init__(config, add_pooling_layer)
        for n, l in enumerate(self.encoder.layer):
            if hasattr(l, "crossattention"):
                l.crossattention = _TwinAttention(config, n)
                l.crossattention.apply(lambda m: med._init_bert(m, config.initializer_range))

    # ------------------------------------------------------------------ precision
    def _require_plain(self, who):
        for m in self.modules():
            if parity_mode(m):
                raise NotImplementedError(f"{who}: the parity precision mode is not served ({self.plain_only})")
            if compute_dtype(m) == FP8:
                raise NotImplementedError(f"{who}: fp8 is not served ({self.plain_only})")

    # ------------------------------------------------------------------ packing
    def _pack(self):
        self._require_plain("nlvr_encoder.BertModel")
        return super()._pack()

    def _pack_cross(self, i, x, d):
        c = self.cdt
        s, o = (x.self0, x.self1), x.output
        merge = (o.merge_layer.weight, o.merge_layer.bias) if hasattr(o, "merge_layer") else ()
        wf, bf = fold_twin_output(o.dense0.weight, o.dense0.bias, o.dense1.weight, o.dense1.bias, *merge)
        d.update(cq_w=[w16(a.query.weight, dtype=c) for a in s], cq_b=[v32(a.query.bias) for a in s],
                 ckv_w=[w16(a.key.weight, a.value.weight, dtype=c) for a in s], ckv_b=[v32(a.key.bias, a.value.bias) for a in s],
                 cf_w=wf.to(c).contiguous(), cf_b=bf.float().contiguous(),
                 co_g=v32(o.LayerNorm.weight), co_bt=v32(o.LayerNorm.bias))

    # ------------------------------------------------------------------ cross K | V (once per image pair)
    def project_cross_kv(self, *a, **kw):
        raise K.VidilHipError("nlvr_encoder.BertModel: the twin encoder projects both sides' K | V with project_twin_kv")

    def project_twin_kv(self, enc16_0, enc16_1, B, Te):
        """enc16_j: 16-bit [B*Te, encoder_width] tokens of image j of B pairs.  One fused K | V GEMM per side per layer with
        that side's [Wk_j; Wv_j].  Returns (CrossKV of side 0, CrossKV of side 1): plain rows, K and V [L][B,H,Te,64] (NP = 0)."""
        p = self.packed()
        H, L = self.config.num_attention_heads, len(p["layers"])
        if Te > MAX_VIDEO_TOKENS:
            raise K.VidilHipError(f"nlvr_encoder.BertModel: {Te} encoder states per image: more than {MAX_VIDEO_TOKENS} keys are not "
                                  "served by the attention kernels")
        out = []
        for j, enc16 in enumerate((enc16_0, enc16_1)):
            require_cuda(enc16, "nlvr_encoder.BertModel.project_twin_kv")
            if tuple(enc16.shape) != (B * Te, self.config.encoder_width) or enc16.dtype != self.cdt:
                raise K.VidilHipError(f"project_twin_kv: side {j} must be {self.cdt} [{B * Te}, {self.config.encoder_width}], got "
                                      f"{enc16.dtype} {tuple(enc16.shape)}")
            k = torch.empty((L, B, H, Te, 64), dtype=enc16.dtype, device=enc16.device)
            v = torch.empty((L, B, H, Te, 64), dtype=enc16.dtype, device=enc16.device)
            for i, d in enumerate(p["layers"]):
                K.gemm(enc16, d["ckv_w"][j], d["ckv_b"][j], heads=dict(k=k[i], vt=v[i], T=Te, H=H, part0=1, t_off=0, Tk_cap=Te, NP=0))
            out.append(CrossKV(k, v, B, Te, 0))
        return tuple(out)

    # ------------------------------------------------------------------ the twin block
    def cross_block(self, i, d, route, q, o, tmp, h32, h16, T):
        """models/nlvr_encoder.py:290-309,235-247: per side the query GEMM and one attention launch (``q`` is reused: the launches
        are ordered on the stream) writing into its half of the [M, 2C] context rows; the folded K = 2C residual GEMM; LayerNorm."""
        H, C, eps = self.config.num_attention_heads, self.config.hidden_size, self.config.layer_norm_eps
        ctx = route.contexts(h16.shape[0], C, h16)
        flat = ctx.view(-1)
        for j, r in enumerate(route.sides):
            c = r.cross
            K.gemm(h16, d["cq_w"][j], d["cq_b"][j], heads=dict(q=q, T=T, H=H, part0=0, Tq_cap=T, q_scale=0.125))
            # (row t of side j: ctx[t, j*C + h*64 ..] — rows 2C apart from an origin j*C elements into the buffer)
            K.attention(q, c.k[i], c.vt[i], flat[j * C:], Bq=r.rows, H=H, Nq=T, Nk=c.Te, Tq_cap=T, Tk_cap=c.Tk_cap, NP=c.NP,
                        group_start=r.groups, max_group=r.bound(T), kv_tiled=r.tiled, ldo=2 * C)
        K.gemm(ctx, d["cf_w"], d["cf_b"], out=tmp, resid=h32)
        K.layernorm(tmp, d["co_g"], d["co_bt"], eps, out16=h16, out32=h32)

    # ------------------------------------------------------------------ the library's entry
    def encode_twin(self, ids_i32, lens_i32, cross0, cross1, *, groups=None, max_group=0):
        """ids i32 [P, T] right-padded sentences and lens i32 [P] (device); cross0 / cross1: ``project_twin_kv``'s pair over B
        image pairs.  Sentence p reasons over pair p (``groups`` None: B == P), or — pair-major order — pair j serves sentences
        groups[j] .. groups[j+1]-1 (i32 [B+1], device; at most ``max_group`` each).  Returns (h32, h16) [P*T, C]: every
        position's last hidden state.  Every cross-attention launch takes the ``group_start`` form with the bound rounded up to
        ceil(33 / T) sentences (row tiles past a pair's last sentence return at once), at every token count."""
        require_cuda(ids_i32, "nlvr_encoder.BertModel.encode_twin")
        self._require_plain("nlvr_encoder.BertModel.encode_twin")
        cfg = self.config
        P, T = ids_i32.shape
        if T > cfg.max_position_embeddings:
            raise ValueError(f"nlvr_encoder.BertModel.encode_twin: {T} tokens exceed max_position_embeddings={cfg.max_position_embeddings}")
        if T > self.LONG_KEYS:
            raise K.VidilHipError(f"nlvr_encoder.BertModel.encode_twin: self-attention over {T} > {self.LONG_KEYS} keys is not served")
        if (cross0.B, cross0.Te) != (cross1.B, cross1.Te):
            raise ValueError(f"encode_twin: the two sides hold {cross0.B} x {cross0.Te} and {cross1.B} x {cross1.Te} encoder states")
        if groups is None:
            if cross0.B != P:
                raise ValueError(f"encode_twin: {P} sentences for {cross0.B} image pairs (pass groups= for the pair-major form)")
            groups, max_group = torch.arange(P + 1, dtype=torch.int32, device=ids_i32.device), 1
        elif groups.dtype != torch.int32 or groups.numel() != cross0.B + 1 or max_group < 1:
            raise ValueError(f"encode_twin: groups must be i32 [{cross0.B + 1}] with max_group >= 1")
        route = TwinRoute(self, cross0, cross1, P, groups.contiguous(), max(max_group, -(-33 // T)))
        h32, h16 = self.embed(ids_i32.reshape(-1), T, 0)
        sk, sv, NPs = self.scratch_kv(P, T, h16.dtype, h32.device)
        return self.run_layers(h32, h16, rows=P, T=T, self_k=sk, self_vt=sv, t_off=0, Tk_cap=T, NPs=NPs, causal=False,
                               kv_len=lens_i32, cross=cross0, route=route, fused=False)

    # ------------------------------------------------------------------ the reference's call
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, head_mask=None, inputs_embeds=None,
                encoder_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None, past_key_values=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, is_decoder=False,
                mode='multimodal'):
        """The reference's call (models/nlvr_encoder.py:705-842; models/blip_nlvr.py:51-57) over ``encode_twin``.

        Served: input_ids int64 / int32 [B, T] on the device; attention_mask [B, T] of 0 / 1 whose ones form a prefix of every
        row (what padding='longest' produces; default: ones); encoder_hidden_states a list of two f32 or 16-bit [B, Te, width]
        tensors; encoder_attention_mask None or a list of two masks that are None or all ones; mode 'multimodal'; return_dict
        (None: True).  Returns an object with ``last_hidden_state`` f32 [B, T, C] (return_dict=False: the tuple
        (last_hidden_state, None)).  Positions whose mask is 0 are outside the contract.
        Refused by a NotImplementedError that names the argument, before the device is required: position_ids, head_mask,
        inputs_embeds, encoder_embeds, past_key_values, use_cache=True, output_attentions=True, output_hidden_states=True,
        is_decoder=True, mode other than 'multimodal', encoder_hidden_states that is not a list of two, an attention mask
        that is not a prefix mask, an image mask with a zero, and the parity precision mode / fp8.
        Cost: both sides' K | V of every layer are projected in every call.  No backward pass."""
        name = "nlvr_encoder.BertModel.forward"
        for arg, value in (("position_ids", position_ids), ("head_mask", head_mask), ("inputs_embeds", inputs_embeds),
                           ("encoder_embeds", encoder_embeds), ("past_key_values", past_key_values), ("use_cache", use_cache),
                           ("output_attentions", output_attentions), ("output_hidden_states", output_hidden_states),
                           ("is_decoder", is_decoder)):
            if value is not None and value is not False:
                raise NotImplementedError(f"{name}: {arg}{'=True' if value is True else ''} is not served (the docstring lists what is)")
        if mode != "multimodal":
            raise NotImplementedError(f"{name}: mode={mode!r} is not served (multimodal)")
        enc = encoder_hidden_states
        if not isinstance(enc, (list, tuple)) or len(enc) != 2:
            raise NotImplementedError(f"{name}: encoder_hidden_states must be a list of the two images' states (a single tensor is "
                                      "med.BertModel's call)")
        masks = encoder_attention_mask
        if masks is not None and (not isinstance(masks, (list, tuple)) or len(masks) != 2):
            raise NotImplementedError(f"{name}: encoder_attention_mask must be None or a list of two masks")
        if input_ids is None:
            raise ValueError(f"{name}: input_ids is required")
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{name}: input_ids must be int64 or int32 [B, T], got {input_ids.dtype} {tuple(input_ids.shape)}")
        B, T = input_ids.shape
        cfg = self.config
        for j, e in enumerate(enc):
            if e.dim() != 3 or e.shape[0] != B or e.shape[2] != cfg.encoder_width or e.shape[1] != enc[0].shape[1]:
                raise ValueError(f"{name}: encoder_hidden_states[{j}] must be [{B}, Te, {cfg.encoder_width}], got {tuple(e.shape)}")
            m = None if masks is None else masks[j]
            if m is not None and (tuple(m.shape) != tuple(e.shape[:2]) or not bool((m != 0).all())):
                raise NotImplementedError(f"{name}: encoder_attention_mask[{j}] with a zero is not served (None or all ones "
                                          f"[{B}, {e.shape[1]}])")
        if attention_mask is None:
            lens = torch.full((B,), T, dtype=torch.int32)
        else:
            if tuple(attention_mask.shape) != (B, T):
                raise ValueError(f"{name}: attention_mask must be [{B}, {T}] of 0 / 1, got {tuple(attention_mask.shape)}")
            keep = attention_mask != 0
            lens = keep.sum(1)
            if not bool((keep == (torch.arange(T, device=keep.device)[None, :] < lens[:, None])).all()) or not bool((lens > 0).all()):
                raise NotImplementedError(f"{name}: an attention_mask whose ones do not form a non-empty prefix of every row is not "
                                          "served (padding='longest' masks are)")
        self._require_plain(name)
        if T > cfg.max_position_embeddings:
            raise ValueError(f"{name}: {T} tokens exceed max_position_embeddings={cfg.max_position_embeddings}")
        require_cuda(input_ids, name)
        dev = input_ids.device
        Te = enc[0].shape[1]
        e16 = [e.to(dev).to(self.cdt).reshape(B * Te, cfg.encoder_width).contiguous() for e in enc]
        cross0, cross1 = self.project_twin_kv(e16[0], e16[1], B, Te)
        h32, _ = self.encode_twin(input_ids.to(torch.int32).contiguous(), lens.to(dev).to(torch.int32).contiguous(), cross0, cross1)
        last = h32.view(B, T, cfg.hidden_size)
        if return_dict is not None and not return_dict:
            return (last, None)
        return ModelOutput(last_hidden_state=last, pooler_output=None, past_key_values=None, hidden_states=None, attentions=None,
                           cross_attentions=None)
