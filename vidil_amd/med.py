"""MED (BERT with cross-attention) on the HIP kernels.

Mirror of the parts of the reference's models/med.py that the hot path executes:
``BertModel`` (ITM text encoder, models/blip_itm.py:31) and ``BertLMHeadModel``
(caption decoder, models/blip.py:98).  Parameter names are the reference's, so
BLIP checkpoints load unchanged (``bert.encoder.layer.N.crossattention.self.key.weight`` …).

Schedule differences from the reference (results are the same function):
  * cross-attention K/V are projected ONCE per image per layer
    (``project_cross_kv``) instead of on every call for every beam
    (models/med.py:160-163);
  * the decoder KV cache is a preallocated [rows, H, max_len, 64] / V^T buffer the
    GEMM epilogue appends into, instead of ``torch.cat`` per step (:164-168);
  * q/k/v of self-attention are one fused GEMM.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn as nn

from . import kernels as K
from .packing import FP8, PackedCache, fold_layernorm, parity_attention_arith, parity_attention_f32, parity_attention_kind, require_cuda, v32, w3, w8, w16
from .video import MAX_VIDEO_TOKENS

LN_EPS_DEFAULT = 1e-12

#: f32 logits BertLMHeadModel.score holds at a time: the target rows go through the LM head and the one-pass reduction
#: (kernels.token_logprobs) in row blocks of this many bytes, in ONE reused buffer (8,704 rows of 30,524 logits)
LOGITS_BLOCK_BYTES = 1 << 30
#: rows of EVERY vocabulary-GEMM launch of lm_logits_rows (a shorter tail is padded with a repeated row): with M fixed the
#: library's GEMM dispatch picks the same kernel for every launch, so a caption's logits cannot depend on what shares its batch
HEAD_GEMM_ROWS = 512
#: shortest token block score() runs the decoder stack on (shorter batches are right-padded): above 32 query rows per unit
#: every attention launch of the stack is served by the staged kernel whatever the longest caption of the batch is
SCORE_MIN_TOKENS = 33
#: captions per stack pass of score() when captions map to images through image_index (one attention unit per caption)
SCORE_MAX_CAPTIONS_PER_PASS = 16384


def teacher_forced_targets(ids, lens, prompt_length):
    """The labels of the teacher-forced caption loss as a pure function (models/blip.py:113-114 and the shift of
    models/med.py:912-913): ids int [P, T] right-padded, lens int [P] real tokens per row -> int64 [P, T] with
    out[p, t] = ids[p, t + 1] where position t + 1 is a real token past the prompt, -100 (ignored) elsewhere —
    the logits at position t are scored against the token at t + 1."""
    ids = torch.as_tensor(ids).long()
    lens = torch.as_tensor(lens).long().to(ids.device)
    T = ids.shape[1]
    t = torch.arange(T, device=ids.device)
    tgt = torch.where(t[None, :] < lens[:, None], ids, torch.full_like(ids, -100))
    tgt[:, :prompt_length] = -100
    out = torch.full_like(tgt, -100)
    out[:, :-1] = tgt[:, 1:]
    return out


class CaptionScores:
    """Result of BertLMHeadModel.score.  Per caption: ``loss_sum`` f32 [P] (the label-smoothed loss summed over the caption's
    target tokens, models/med.py:916-917) and ``count`` i32 [P].  Per target token, N in all, in the order scored:
    ``lp_label`` / ``lp_mean`` f32 [N] (log-probability of the given token, mean log-probability over the vocabulary),
    ``argmax`` i32 [N] (the greedy token at that position), ``token_loss`` f32 [N], ``caption`` / ``position`` int64 [N]
    (caption index and position of the TARGET token in it)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def tokens_of(self, p):
        """Indices (int64, device) of caption p's target tokens, in position order."""
        idx = (self.caption == p).nonzero().view(-1)
        return idx[self.position[idx].argsort()]


class ModelOutput:
    """What the reference-signature ``forward``s return with return_dict=True: the fields as attributes and by name, and —
    as the HF output classes — by position over the fields that are not None."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def to_tuple(self):
        return tuple(v for v in self.__dict__.values() if v is not None)

    def __getitem__(self, key):
        return self.__dict__[key] if isinstance(key, str) else self.to_tuple()[key]


class BertConfig:
    """The fields of configs/med_config.json the hot path reads."""

    def __init__(self, **kw):
        self.hidden_size = 768
        self.num_hidden_layers = 12
        self.num_attention_heads = 12
        self.intermediate_size = 3072
        self.hidden_act = "gelu"
        self.layer_norm_eps = LN_EPS_DEFAULT
        self.max_position_embeddings = 512
        self.vocab_size = 30524
        self.pad_token_id = 0
        self.type_vocab_size = 2
        self.initializer_range = 0.02
        self.encoder_width = 768
        self.add_cross_attention = True
        self.hidden_dropout_prob = 0.1
        self.attention_probs_dropout_prob = 0.1
        for k, v in kw.items():
            setattr(self, k, v)
        if self.hidden_act != "gelu":
            raise ValueError("only hidden_act='gelu' (erf) is implemented")
        if self.hidden_size // self.num_attention_heads != 64:
            raise ValueError("vidil_amd MED kernels are built for head_dim 64")

    @classmethod
    def from_json_file(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


# ---- parameter holders (names = reference state_dict keys) -------------------------
class _SelfAttn(nn.Module):
    def __init__(self, cfg, cross):
        super().__init__()
        kv_in = cfg.encoder_width if cross else cfg.hidden_size
        self.query = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.key = nn.Linear(kv_in, cfg.hidden_size)
        self.value = nn.Linear(kv_in, cfg.hidden_size)


class _DenseLN(nn.Module):
    def __init__(self, d_in, d_out, eps):
        super().__init__()
        self.dense = nn.Linear(d_in, d_out)
        self.LayerNorm = nn.LayerNorm(d_out, eps=eps)


class _Attention(nn.Module):
    def __init__(self, cfg, cross=False):
        super().__init__()
        self.self = _SelfAttn(cfg, cross)
        self.output = _DenseLN(cfg.hidden_size, cfg.hidden_size, cfg.layer_norm_eps)


class _Intermediate(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.intermediate_size)


class BertLayer(nn.Module):
    def __init__(self, cfg, layer_num):
        super().__init__()
        self.attention = _Attention(cfg)
        if cfg.add_cross_attention:
            self.crossattention = _Attention(cfg, cross=True)
        self.intermediate = _Intermediate(cfg)
        self.output = _DenseLN(cfg.intermediate_size, cfg.hidden_size, cfg.layer_norm_eps)


class BertEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([BertLayer(cfg, i) for i in range(cfg.num_hidden_layers)])


class BertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden_size, padding_idx=cfg.pad_token_id)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(cfg.max_position_embeddings).expand((1, -1)))


def _init_bert(module, std):
    """models/med.py:558-568."""
    if isinstance(module, (nn.Linear, nn.Embedding)):
        module.weight.data.normal_(mean=0.0, std=std)
    elif isinstance(module, nn.LayerNorm):
        module.bias.data.zero_()
        module.weight.data.fill_(1.0)
    if isinstance(module, nn.Linear) and module.bias is not None:
        module.bias.data.zero_()


class CrossKV:
    """Per-image cross-attention keys / values^T of every layer: K [L][B,H,Te,64], VT [L][B,H,64,NP]."""

    def __init__(self, k, vt, B, Te, NP, last_vt=None, last_NP=0, tiled=False, Tk_cap=None, f32=False):
        self.k, self.vt, self.B, self.Te, self.NP = k, vt, B, Te, NP
        # f32 (parity precision mode with vidil_attention_f32): k = f32 [L][B, Te, 2C] — the K | V projection GEMM's row-major
        # output, keys in columns 0..C-1 and values in C..2C-1 — and vt a placeholder [L][B, 1] (same batch axis for adopt())
        self.f32 = f32
        # tiled: K and V of every layer in 32-key fragment tiles [L][B,H,Tk_cap/32,2048] (vidil_attention kv_tiled)
        self.tiled, self.Tk_cap = tiled, (Te if Tk_cap is None else Tk_cap)
        # optional second copy of the LAST layer's values in V^T layout (see project_cross_kv(last_layer_vt=True))
        self.last_vt, self.last_NP = last_vt, last_NP


class CrossRoute:
    """The cross-attention side of one stack pass: the ``CrossKV`` (None: a pass without cross-attention) and which encoder unit
    each of the pass's ``rows`` query batches attends to — unit ``index[r]`` (i32 [rows], device); or, image-major order, unit j
    serves batches groups[j] .. groups[j+1]-1 (i32 [B+1], at most ``max_group`` each); or unit r // group.  ``kv_len`` (i32
    [rows], device; None: every one of cross.Te keys): batch r attends to the first kv_len[r] keys of its unit only.
    Building one allocates nothing, launches nothing and waits for nothing (a decode step builds its route under graph capture);
    ``model`` is read for LONG_KEYS and MAX_IMAGES_PER_LAUNCH, as they stand when the pass starts."""

    def __init__(self, model, cross, rows, *, index=None, group=1, groups=None, max_group=0, kv_len=None):
        self.cross, self.rows = cross, rows
        self.index, self.group, self.groups, self.max_group, self.kv_len = index, group, groups, max_group, kv_len
        self.long_keys, self.images_per_launch = model.LONG_KEYS, model.MAX_IMAGES_PER_LAUNCH
        if kv_len is not None and (kv_len.dtype != torch.int32 or kv_len.dim() != 1 or kv_len.numel() != rows or not kv_len.is_contiguous()):
            raise K.VidilHipError(f"run_layers: cross_kv_len must be a contiguous i32 [{rows}] tensor (one length per query batch), got "
                                  f"{kv_len.dtype} {tuple(kv_len.shape)}")

    @property
    def tiled(self):
        """The ``kv_tiled`` selector of a launch: 2 (key-split form allowed) for fragment tiles over more than LONG_KEYS encoder
        states; otherwise what it always was, so launches over up to LONG_KEYS states are unchanged."""
        return 2 if self.cross.tiled and self.cross.Te > self.long_keys else self.cross.tiled

    def bound(self, Nq):
        """The ``max_group`` bound of a launch with Nq query rows per batch.  Up to LONG_KEYS encoder states it is the caller's;
        over more (a video's frames concatenated as one encoder sequence) plain K / V are served by the long-key form, for which
        every launch must present more than 32 query rows per unit, so the bound of the ``groups`` form is rounded up to
        ceil(33 / Nq) — it is an upper bound, row tiles past a unit's last row return at once — and the other forms are refused
        where they cannot reach 33 rows.  Fragment tiles (a decoder session's) are served by the key-split form, at most 32 rows
        per unit: the bound stays the caller's, and more rows are refused."""
        Te = self.cross.Te
        if Te <= self.long_keys:
            return self.max_group
        if self.cross.tiled:
            rows = Nq * (self.max_group if self.groups is not None else 1 if self.index is not None else self.group)
            if rows > 32:
                raise K.VidilHipError(f"cross-attention over {Te} > {self.long_keys} encoder states in fragment tiles serves at most "
                                      f"32 query rows per unit (got {rows}): build the session with tiled_cross=False, whose launches "
                                      "go to the long-key form")
            return self.max_group
        if self.groups is not None:
            return max(self.max_group, -(-33 // Nq))
        rows = Nq * (1 if self.index is not None else self.group)
        if rows <= 32:
            raise K.VidilHipError(f"cross-attention over {Te} > {self.long_keys} encoder states needs more than 32 query rows per "
                                  f"unit (got {rows}): order the pairs image-major and use group_start")
        return self.max_group

    def blocks(self):
        """(b0, b1, r0, r1) of the launches of one layer: units [b0, b1) serve query batches [r0, r1).  One launch over every
        batch, whatever maps batches to units; or — uniform grouping (a beam search) over more than MAX_IMAGES_PER_LAUNCH images
        — blocks of that many images, each a launch over contiguous slices of Q, K, V and the output rows."""
        B, n = self.cross.B, self.images_per_launch
        if self.index is not None or self.groups is not None or B <= n:
            return [(0, B, 0, self.rows)]
        return [(b0, min(B, b0 + n), b0 * self.group, min(B, b0 + n) * self.group) for b0 in range(0, B, n)]

    def len_arg(self, r0, r1):
        """The ``kv_len`` keyword of a launch over query batches r0 .. r1-1: nothing for a route without kv_len (the launch then
        is exactly what it was before the argument existed), else its slice of the table."""
        return {} if self.kv_len is None else dict(kv_len=self.kv_len[r0:r1])

    def attend(self, i, q, o, T):
        """The plain 16-bit cross-attention launches of layer i: q [rows, H, T, 64] -> o [rows*T, C].  Every query batch that
        shares an image (the beams of a caption search, the captions of a frame) is served by one fetch of that image's K/V:
        see vidil_attention's grouping forms."""
        c = self.cross
        mg = self.bound(T)
        for b0, b1, r0, r1 in self.blocks():
            K.attention(q[r0:r1], c.k[i][b0:b1], c.vt[i][b0:b1], o[r0 * T:r1 * T], Bq=r1 - r0, H=q.shape[1], Nq=T, Nk=c.Te, Tq_cap=T,
                        Tk_cap=c.Tk_cap, NP=c.NP, kv_group=self.group, kv_index=self.index, group_start=self.groups, max_group=mg,
                        kv_tiled=self.tiled, **self.len_arg(r0, r1))


class BeamArena:
    """Append-only self-attention K/V of a beam search (all layers): k, v f16 [L][Tcap][rows][H*64], written at
    [position][slot = producing beam row]; ``anc`` i32 [rows][Tcap] maps (beam row, position) -> slot and is the
    only thing reordered per step (vidil_beam_ancestry) — the reference's _reorder_cache without moving the cache."""

    def __init__(self, L, Tcap, rows, C, device, dtype=torch.float16):
        self.L, self.Tcap, self.rows = L, Tcap, rows
        self.k = torch.empty((L, Tcap, rows, C), dtype=dtype, device=device)
        self.v = torch.empty((L, Tcap, rows, C), dtype=dtype, device=device)
        self._anc = [torch.zeros((rows, Tcap), dtype=torch.int32, device=device) for _ in range(2)]
        self._cur = 0

    @property
    def anc(self):
        return self._anc[self._cur]

    def init_prompt(self, P, group):
        """Positions 0..P-1 of beam row r live in slot (r // group) * group (group = nb after a shared prompt
        pass over one row per image, 1 when every row ran its own prompt pass)."""
        r = torch.arange(self.rows, dtype=torch.int32, device=self.k.device)
        self.anc[:, :P] = (torch.div(r, group, rounding_mode="floor") * group).to(torch.int32)[:, None]

    def reorder(self, beam_idx_i32, cur_pos):
        """Beam row r now continues old row beam_idx[r]; its next K/V (position cur_pos) go to slot r."""
        K.beam_ancestry(self._anc[self._cur], self._anc[self._cur ^ 1], beam_idx_i32, cur_pos)
        self._cur ^= 1


def parity_layers(model, p, h32, h3, *, rows, T, causal, kv_len, route=None, self_k=None, self_vt=None, t_off=0, Tk_cap=None, NPs=0,
                  ws=None, arena=None, arena_slot_stride=1, n_layers=None, rel_bias=None, rel_off=None):
    """BertModel.run_layers in the parity precision mode, on the packed layers ``p["layers"]``: ``h3`` [rows*T, 3C] carries the
    hidden states as [hi | lo | hi] operand rows, every GEMM runs against [W_hi | W_hi | W_lo] with K tripled, LayerNorm /
    attention write split rows directly and the GELU output goes through f32 + vidil_split3_f32.  Same launch sequence otherwise.
    Of ``model`` it needs config.num_attention_heads / hidden_size / intermediate_size / layer_norm_eps and the parity-attention
    setting packing keeps for it (parity_attention_f32 / parity_attention_arith): a BertModel, or vidil_amd/sentence.py's
    encoder, which runs this sequence as the layers of MPNet.
    route: the pass's CrossRoute (None: no cross-attention).  self_k / self_vt / Tk_cap / NPs: attention kind "16" only.
    n_layers: only the first n layers (encode_cls_parity runs the last itself); ws["planes_h"] then tells it how many
    planes of ``h3`` the last of them wrote.
    rel_bias / rel_off: a relative-position bias table for the block self-attention of every layer (kernels.attention_f32's
    arguments; the f32-row attention kinds only)."""
    cross = None if route is None else route.cross
    if rel_bias is not None and (not parity_attention_f32(model) or arena is not None or cross is not None):
        raise K.VidilHipError("_run_layers_parity: rel_bias serves the f32-row self-attention of a stack without cross-attention or arena")
    if route is not None and route.kv_len is not None:
        raise K.VidilHipError("_run_layers_parity: cross_kv_len (masked cross-attention) is not built for the parity precision mode")
    cfg = model.config
    H, C = cfg.num_attention_heads, cfg.hidden_size
    eps = cfg.layer_norm_eps
    M = rows * T
    dev, cdt = h32.device, h3.dtype
    if ws is None:
        ws = {}
    q = ws.get("q")
    if q is None or q.shape[0] < rows or q.shape[2] != T:
        q = torch.empty((rows, H, T, 64), dtype=cdt, device=dev)
        ws["q"] = q
    o3 = torch.empty((M, 3 * C), dtype=cdt, device=dev)
    tmp = torch.empty((M, C), dtype=torch.float32, device=dev)
    inter3 = torch.empty((M, 3 * cfg.intermediate_size), dtype=cdt, device=dev)
    # Which producers may leave the third plane of their [hi | lo | hi] rows unwritten: only those whose EVERY
    # consumer takes the K-loop form of the compensated product, asked per CALL (K.split_k_serves).  inter3 feeds fc2 (f32
    # epilogue); with the f32-row attention kinds h3 / o3 feed Q|K|V, the cross query, both output projections and fc1, all
    # with the f32 epilogue; kind "16" feeds h3 to arena / short-sequence scatter epilogues, which run the plain K = 3 Kl
    # product over all three planes.  The consumers state a_planes, so a launch that would read an unwritten plane fails
    # (EINVAL) instead of computing on it.
    f32_attn, arith = parity_attention_f32(model), parity_attention_arith(model)
    qkv32 = torch.empty((M, 3 * C), dtype=torch.float32, device=dev) if f32_attn else None
    q32 = torch.empty((M, C), dtype=torch.float32, device=dev) if f32_attn and cross is not None else None
    d0 = p["layers"][0]
    planes = planes_h = 3
    if K.split_k_serves(inter3, d0["o_w3"], d0["o_b"], out=tmp, resid=h32):
        planes = 2
    if f32_attn and planes == 2 and all((
            K.split_k_serves(h3, d0["qkv_w3"], d0["qkv_b"], out=qkv32),
            K.split_k_serves(o3, d0["ao_w3"], d0["ao_b"], out=tmp, resid=h32),
            K.split_k_serves(h3, d0["i_w3"], d0["i_b"], split3_out=inter3, act=K.ACT_GELU_ERF),
            cross is None or K.split_k_serves(h3, d0["cq_w3"], d0["cq_b"], out=q32))):
        planes_h = 2
    K.poison_third_plane(planes, inter3)
    K.poison_third_plane(planes_h, o3, h3)
    ws["planes_h"] = planes_h
    Nk = t_off + T
    # The three cross launches below are this sequence's own, NOT CrossRoute.attend: they pass the caller's max_group and
    # cross.tiled unmodified (no CrossRoute.bound, no kv_tiled = 2) and only the kv16 branch walks the route's blocks, so past
    # LONG_KEYS keys, or past MAX_IMAGES_PER_LAUNCH images outside kv16, the parity mode lacks what the plain stacks do.
    if f32_attn:
        # Q | K | V (and the cross query) stay f32 and row-major, the KV arena and the cross K | V are f32:
        # vidil_attention_f32 reads all of them in place.  (t_off > 0 happens in the arena form only.)
        # (split-operand kind: the cross K | V of a decoder session are 16-bit fragment tiles instead)
        kv16 = cross is not None and arith == 1 and cross.tiled and not cross.f32
        if (arena is not None and arena.k.dtype != torch.float32) or (cross is not None and not cross.f32 and not kv16):
            raise K.VidilHipError("run_layers (parity mode, f32 attention): the KV arena / cross K|V of this session were built for "
                                  "the 16-bit attention kernels — build the DecoderSession / CrossKV under the same $VIDIL_PARITY_ATTN")
        if t_off != 0 and not (arena is not None and T == 1):
            raise K.VidilHipError("run_layers (parity mode, f32 attention): cached self-attention keys are served by the arena form only")
        if kv16 and T * max(1, route.group) > 32 and route.groups is None and route.index is None:
            # (the kv16 form serves at most 32 query rows per image — a DecoderSession's decode steps and shared
            #  prompt pass; a longer prompt x group must be built with the f32-row cross K|V instead)
            raise K.VidilHipError(f"run_layers (parity mode, split attention): {T} tokens x {route.group} sequences per image exceed the 32 "
                                  "query rows per image the 16-bit cross K/V tiles serve — build the session with tiled_cross=False")
    for i, d in enumerate(p["layers"][:n_layers]):
        if f32_attn:
            K.gemm(h3, d["qkv_w3"], d["qkv_b"], out=qkv32, split_k=True, a_planes=planes_h)
            if arena is not None and T == 1:
                arena.k[i][t_off].copy_(qkv32[:, C:2 * C])          # position t_off, slot = producing beam row
                arena.v[i][t_off].copy_(qkv32[:, 2 * C:])
                K.attention_f32(qkv32[:, :C], arena.k[i], arena.v[i], o3, Bq=rows, H=H, Nq=1, Nk=Nk, anc=arena.anc,
                                arena_rows=arena.rows, planes=planes_h)
            else:
                K.attention_f32(qkv32[:, :C], qkv32[:, C:2 * C], qkv32[:, 2 * C:], o3, Bq=rows, H=H, Nq=T, Nk=T, causal=causal,
                                kv_len=kv_len, arith=arith, planes=planes_h, rel_bias=rel_bias, rel_off=rel_off)
                if arena is not None:   # the prompt's K / V in the arena: position t, slot r * arena_slot_stride
                    blk = qkv32.view(rows, T, 3 * C)
                    arena.k[i][:T, 0:rows * arena_slot_stride:arena_slot_stride] = blk[:, :, C:2 * C].permute(1, 0, 2)
                    arena.v[i][:T, 0:rows * arena_slot_stride:arena_slot_stride] = blk[:, :, 2 * C:].permute(1, 0, 2)
        elif arena is not None and T == 1:
            K.gemm(h3, d["qkv_w3"], d["qkv_b"], split_k=True,
                   arena=dict(q=q, k=arena.k[i], v=arena.v[i], T=1, H=H, part0=0, t_off=t_off, Tcap=arena.Tcap,
                              arena_rows=arena.rows, slot_stride=1, q_scale=0.125))
            K.beam_attention(q, arena.k[i], arena.v[i], arena.anc, o3, rows=rows, H=H, n_keys=Nk, split3=True)
        else:
            K.gemm(h3, d["qkv_w3"], d["qkv_b"], split_k=True,
                   heads=dict(q=q, k=self_k[i], vt=self_vt[i], T=T, H=H, part0=0, t_off=t_off, Tq_cap=T,
                              Tk_cap=Tk_cap, NP=NPs, q_scale=0.125))
            K.attention(q, self_k[i], self_vt[i], o3, Bq=rows, H=H, Nq=T, Nk=Nk, Tq_cap=T, Tk_cap=Tk_cap, NP=NPs,
                        causal=causal, causal_off=t_off, kv_len=kv_len, split3=True)
            if arena is not None:
                K.gemm(h3, d["qkv_w3"][C:], d["qkv_b"][C:], split_k=True,
                       arena=dict(k=arena.k[i], v=arena.v[i], T=T, H=H, part0=1, t_off=0, Tcap=arena.Tcap,
                                  arena_rows=arena.rows, slot_stride=arena_slot_stride))
        K.gemm(o3, d["ao_w3"], d["ao_b"], out=tmp, resid=h32, split_k=True, a_planes=planes_h)
        K.layernorm(tmp, d["ao_g"], d["ao_bt"], eps, out16=h3, out32=h32, split3=True, planes=planes_h)
        if cross is not None and f32_attn:
            K.gemm(h3, d["cq_w3"], d["cq_b"], out=q32, split_k=True, a_planes=planes_h)
            if kv16:
                for b0, b1, r0, r1 in route.blocks():
                    K.attention_f32(q32[r0 * T:r1 * T], cross.k[i][b0:b1], cross.vt[i][b0:b1], o3[r0 * T:r1 * T], Bq=r1 - r0, H=H, Nq=T, Nk=cross.Te,
                                    kv_rows=cross.Tk_cap, kv_group=route.group, kv_index=route.index, group_start=route.groups,
                                    max_group=route.max_group, arith=1, kv16=True, planes=planes_h)
            else:
                kv = cross.k[i]                                     # f32 [B, Te, 2C]: keys | values
                K.attention_f32(q32, kv[..., :C], kv[..., C:], o3, Bq=rows, H=H, Nq=T, Nk=cross.Te, kv_rows=cross.Te,
                                kv_group=route.group, kv_index=route.index, group_start=route.groups, max_group=route.max_group,
                                arith=arith, planes=planes_h)
            K.gemm(o3, d["co_w3"], d["co_b"], out=tmp, resid=h32, split_k=True, a_planes=planes_h)
            K.layernorm(tmp, d["co_g"], d["co_bt"], eps, out16=h3, out32=h32, split3=True, planes=planes_h)
        elif cross is not None:
            K.gemm(h3, d["cq_w3"], d["cq_b"], heads=dict(q=q, T=T, H=H, part0=0, Tq_cap=T, q_scale=0.125), split_k=True)
            # (project_cross_kv(last_layer_vt=True) keeps the LAST layer's values in a V^T buffer of their own)
            last = i == len(p["layers"]) - 1 and cross.last_vt is not None
            K.attention(q, cross.k[i], cross.last_vt if last else cross.vt[i], o3, Bq=rows, H=H, Nq=T, Nk=cross.Te, Tq_cap=T,
                        Tk_cap=cross.Tk_cap, NP=cross.last_NP if last else cross.NP, kv_group=route.group, kv_index=route.index,
                        group_start=route.groups, max_group=route.max_group, kv_tiled=cross.tiled, split3=True)
            K.gemm(o3, d["co_w3"], d["co_b"], out=tmp, resid=h32, split_k=True)
            K.layernorm(tmp, d["co_g"], d["co_bt"], eps, out16=h3, out32=h32, split3=True, planes=planes_h)
        K.gemm(h3, d["i_w3"], d["i_b"], split3_out=inter3, act=K.ACT_GELU_ERF, split_k=True, split3_planes=planes, a_planes=planes_h)
        K.gemm(inter3, d["o_w3"], d["o_b"], out=tmp, resid=h32, split_k=True, a_planes=planes)
        K.layernorm(tmp, d["o_g"], d["o_bt"], eps, out16=h3, out32=h32, split3=True, planes=planes_h)
    return h32, h3


class BertModel(PackedCache, nn.Module):
    """ITM text encoder / decoder trunk.  The hot path calls ``encode`` (ITM) or is driven by ``BertLMHeadModel``;
    ``forward`` takes the reference's call (the HF signature) and runs it on the same passes."""

    #: images per cross-attention / cross K|V projection launch of a decode batch (a search over more images — the images of
    #: several tower chunks — issues these launches per block of this many images: byte-floor kernels whose launch already fills
    #: the chip, kept at the sizes every per-unit offset of theirs has been exercised at)
    MAX_IMAGES_PER_LAUNCH = 4096

    def __init__(self, config, add_pooling_layer=False):
        super().__init__()
        if add_pooling_layer:
            raise ValueError("the pooler is not on the hot path (reference builds add_pooling_layer=False)")
        self.config = config
        self.embeddings = BertEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.apply(lambda m: _init_bert(m, config.initializer_range))

    # ------------------------------------------------------------------ packing
    def _pack(self):
        e = self.embeddings
        c = self.cdt
        p = dict(word=v32(e.word_embeddings.weight).view(self.config.vocab_size, -1),
                 pos=v32(e.position_embeddings.weight).view(self.config.max_position_embeddings, -1),
                 emb_g=v32(e.LayerNorm.weight), emb_b=v32(e.LayerNorm.bias), layers=[])
        for i, l in enumerate(self.encoder.layer):
            a, o = l.attention.self, l.attention.output
            d = dict(qkv_w=w16(a.query.weight, a.key.weight, a.value.weight, dtype=c),
                     qkv_b=v32(a.query.bias, a.key.bias, a.value.bias),
                     ao_w=w16(o.dense.weight, dtype=c), ao_b=v32(o.dense.bias),
                     ao_g=v32(o.LayerNorm.weight), ao_bt=v32(o.LayerNorm.bias),
                     i_w=w16(l.intermediate.dense.weight, dtype=c), i_b=v32(l.intermediate.dense.bias),
                     o_w=w16(l.output.dense.weight, dtype=c), o_b=v32(l.output.dense.bias),
                     o_g=v32(l.output.LayerNorm.weight), o_bt=v32(l.output.LayerNorm.bias))
            if hasattr(l, "crossattention"):
                self._pack_cross(i, l.crossattention, d)
            if self.parity:      # parity precision mode: [W_hi | W_hi | W_lo] for every GEMM of the stack
                d.update(qkv_w3=w3(a.query.weight, a.key.weight, a.value.weight, dtype=c), ao_w3=w3(o.dense.weight, dtype=c),
                         i_w3=w3(l.intermediate.dense.weight, dtype=c), o_w3=w3(l.output.dense.weight, dtype=c))
            p["layers"].append(d)
        p["parity"] = self.parity
        return p

    def _pack_cross(self, i, x, d):
        """The operands of layer i's cross-attention block ``x`` into the layer's dict ``d`` (nlvr_encoder.BertModel overrides it
        with the twin block's)."""
        c = self.cdt
        ca, co = x.self, x.output
        d.update(cq_w=w16(ca.query.weight, dtype=c), cq_b=v32(ca.query.bias),
                 ckv_w=w16(ca.key.weight, ca.value.weight, dtype=c), ckv_b=v32(ca.key.bias, ca.value.bias),
                 co_w=w16(co.dense.weight, dtype=c), co_b=v32(co.dense.bias),
                 co_g=v32(co.LayerNorm.weight), co_bt=v32(co.LayerNorm.bias))
        if self.fp8:     # fp8 tower mode: the image-side K|V projection (its A rows are a tower's output) on e4m3 too
            d["ckv_w8"], d["ckv_s"] = w8(ca.key.weight, ca.value.weight)
        if self.parity:
            d.update(cq_w3=w3(ca.query.weight, dtype=c), ckv_w3=w3(ca.key.weight, ca.value.weight, dtype=c),
                     co_w3=w3(co.dense.weight, dtype=c))

    def pack_flags(self):
        # (the attention kind of the parity mode decides the dtype of a session's KV arena and cross K|V: a change re-packs, and
        #  with the new pack object every DecoderSession / captured step graph keyed on it is rebuilt — ADVICE r4)
        return (self.parity, parity_attention_kind(self) if self.parity else None)

    def _folded(self, p):
        """Weights of the LN-folded text stack (built on first use, kept with the pack): per layer the cross query and
        fc1 against the LayerNorms of the SAME layer's self / cross blocks, and (from layer 1 on) Q|K|V against the
        previous layer's output LayerNorm — W' = T16(gamma (.) W), b' = b + W·beta, colsum (packing.fold_layernorm)."""
        if "folded" in p:
            return p["folded"]
        c = self.cdt
        out = []
        layers = list(self.encoder.layer)
        for i, l in enumerate(layers):
            d = {}
            if hasattr(l, "crossattention"):
                ln1, ln2 = l.attention.output.LayerNorm, l.crossattention.output.LayerNorm
                ca = l.crossattention.self
                d["cq"] = fold_layernorm(ca.query.weight, ca.query.bias, ln1.weight, ln1.bias, c)
                d["fc1"] = fold_layernorm(l.intermediate.dense.weight, l.intermediate.dense.bias, ln2.weight, ln2.bias, c)
            if i > 0:
                a, ln3 = l.attention.self, layers[i - 1].output.LayerNorm
                d["qkv"] = fold_layernorm(torch.cat([a.query.weight, a.key.weight, a.value.weight]),
                                          torch.cat([a.query.bias, a.key.bias, a.value.bias]), ln3.weight, ln3.bias, c)
            out.append(d)
        p["folded"] = out
        return out

    # --------------------------------------------------------- cross K/V (once per image)
    def project_cross_kv(self, enc16, B, Te, out: "CrossKV" = None, v_rowmajor=False, last_layer_vt=False, tiled=False,
                         kv_len=None):
        """enc16: f16 [B*Te, encoder_width] image tokens.  One fused K|V GEMM per layer.  ``out``: buffers of a
        previous call with the same (B, Te) to overwrite (keeps device addresses stable for captured graphs).
        ``v_rowmajor``: keep V as [L][B,H,Te,64] (NP = 0) — for consumers whose every cross-attention launch has more
        than 32 query rows per image (the staged kernel transposes in LDS); the decode steps need V^T.
        ``last_layer_vt`` (with v_rowmajor): the last layer's V goes to a V^T buffer instead (``last_vt``) — its
        consumer is encode_cls, whose last layer has one query row per pair.
        ``tiled``: K and V in 32-key fragment tiles — for consumers whose every launch has at most 32 query rows per
        image and which re-read the K/V from HBM many times (the decode steps of the captioner).
        ``kv_len`` (int [B], device): unit b holds kv_len[b] real encoder states followed by padding (the question states of
        BLIP_VQA); the padding rows are cleared before the projection.  The attention kernels mask the SCORES of the keys past
        ``cross_kv_len`` and still multiply those keys' values by the resulting zero probabilities, so a non-finite pad state
        would reach the output as 0 x NaN; cleared rows project to the bias.  With it no pad state is read into a result."""
        p = self.packed()
        H = self.config.num_attention_heads
        cdt = enc16.dtype
        if kv_len is not None:
            if p["parity"]:
                raise K.VidilHipError("project_cross_kv: kv_len (padded encoder units) is not built for the parity precision mode")
            keep = torch.arange(Te, device=enc16.device)[None, :] < kv_len.to(enc16.device).view(B, 1)
            enc16 = torch.where(keep.view(B * Te, 1), enc16, torch.zeros((), dtype=cdt, device=enc16.device)).contiguous()
        if p["parity"]:
            # parity precision mode: enc16 holds [hi | lo | hi] rows of the image tokens (the ViT's parity output)
            if enc16.shape[1] != 3 * self.config.encoder_width:
                raise K.VidilHipError(f"project_cross_kv (parity mode): image tokens must be [hi | lo | hi] rows of width "
                                      f"{3 * self.config.encoder_width}, got {tuple(enc16.shape)}")

            # (split-operand attention: consumers with at most 32 query rows per image — the caption decoder — keep the 16-bit
            #  fragment tiles of the plain path, written by the K-tripled GEMM's heads epilogue: vidil_attention_f32 kv16)
            if parity_attention_f32(self) and not (tiled and parity_attention_arith(self) == 1):
                L, C = len(p["layers"]), self.config.hidden_size
                dev = enc16.device
                if out is not None and out.f32 and (out.B, out.Te) == (B, Te) and out.k.device == dev:
                    kv32, ph = out.k, out.vt
                else:
                    kv32 = torch.empty((L, B, Te, 2 * C), dtype=torch.float32, device=dev)
                    ph = torch.zeros((L, B, 1), dtype=torch.float32, device=dev)
                for i, d in enumerate(p["layers"]):
                    K.gemm(enc16, d["ckv_w3"], d["ckv_b"], out=kv32[i].view(B * Te, 2 * C), split_k=True)
                return CrossKV(kv32, ph, B, Te, 0, f32=True)

            def kv_gemm(d, r0=0, r1=None, **heads):
                K.gemm(enc16[r0:r1], d["ckv_w3"], d["ckv_b"], heads=heads, split_k=True)
        elif self.fp8 and "ckv_w8" in p["layers"][0] and enc16.shape[1] % 128 == 0:
            # fp8 tower mode (BASELINE config 5): e4m3 image tokens x e4m3 K|V weights, K / V written in the 16-bit type
            # (clamped first: torch's e4m3 cast does not saturate — 470 becomes NaN — while every device-side conversion does)
            enc8 = enc16.clamp(-448.0, 448.0).to(FP8)

            def kv_gemm(d, r0=0, r1=None, **heads):
                K.gemm(enc8[r0:r1], d["ckv_w8"], d["ckv_b"], w_scale=d["ckv_s"], dtype16=cdt, heads=heads)
        else:
            def kv_gemm(d, r0=0, r1=None, **heads):
                K.gemm(enc16[r0:r1], d["ckv_w"], d["ckv_b"], heads=heads)
        if tiled:
            Tc = (Te + 31) // 32 * 32
            L = len(p["layers"])
            dev = enc16.device
            if out is not None and out.tiled and (out.B, out.Te) == (B, Te) and out.k.device == dev:
                k, v = out.k, out.vt
            else:
                k = torch.empty((L, B, H, Tc, 64), dtype=cdt, device=dev)
                v = torch.empty((L, B, H, Tc, 64), dtype=cdt, device=dev)
            # (the images of several tower chunks — a decode batch, round 6 — are projected MAX_IMAGES_PER_LAUNCH at a time: the
            #  launch sizes the tower-sized path has always run, whatever the search holds)
            for i, d in enumerate(p["layers"]):
                for b0 in range(0, B, self.MAX_IMAGES_PER_LAUNCH):
                    b1 = min(B, b0 + self.MAX_IMAGES_PER_LAUNCH)
                    kv_gemm(d, b0 * Te, b1 * Te, k=k[i][b0:b1], vt=v[i][b0:b1], T=Te, H=H, part0=1, t_off=0, Tk_cap=Tc, tiled=True)
            return CrossKV(k, v, B, Te, Tc, tiled=True, Tk_cap=Tc)
        NPt = (Te + 15) // 16 * 16
        NP = 0 if v_rowmajor else NPt
        L = len(p["layers"])
        dev = enc16.device
        if out is not None and not out.tiled and (out.B, out.Te, out.NP) == (B, Te, NP) and out.k.device == dev:
            k, vt = out.k, out.vt
        else:
            k = torch.empty((L, B, H, Te, 64), dtype=cdt, device=dev)
            vt = torch.empty((L, B, H, Te, 64) if v_rowmajor else (L, B, H, 64, NP), dtype=cdt, device=dev)
        last_vt = None
        if v_rowmajor and last_layer_vt:
            last_vt = torch.empty((B, H, 64, NPt), dtype=cdt, device=dev)
        for i, d in enumerate(p["layers"]):
            if last_vt is not None and i == L - 1:
                kv_gemm(d, k=k[i], vt=last_vt, T=Te, H=H, part0=1, t_off=0, Tk_cap=Te, NP=NPt)
            else:
                kv_gemm(d, k=k[i], vt=vt[i], T=Te, H=H, part0=1, t_off=0, Tk_cap=Te, NP=NP)
        return CrossKV(k, vt, B, Te, NP, last_vt, NPt if last_vt is not None else 0)

    # ------------------------------------------------------------------ layers
    def run_layers(self, h32, h16, *, rows, T, self_k, self_vt, t_off, Tk_cap, NPs, causal, kv_len,
                   cross: CrossKV, cross_index=None, cross_group=1, cross_groups=None, cross_max_group=0, ws=None,
                   arena: "BeamArena" = None, arena_slot_stride=1, n_layers=None, self_done_first=False,
                   stop_after_self=False, fused=None, cross_kv_len=None, arena_prompt=False, hidden_out=None, route=None):
        """Run every layer on the f32/f16 hidden pair (both [rows*T, C], updated in place).

        self_k / self_vt: [L][rows,H,Tk_cap,64] / [L][rows,H,64,NPs] — this call's keys are appended at
        ``t_off`` and attention runs over t_off+T keys (causal inside the new block when ``causal``).

        arena (beam-search decoding): with T == 1 the new key/value of row r is appended at
        arena[position t_off][slot r] and attention follows the row's ancestry (self_k / self_vt unused);
        with T > 1 (prompt pass, t_off == 0) attention runs over the block as above and the block's K/V are
        ALSO written to the arena at slots r*arena_slot_stride.

        arena_prompt: a ONE-token block at position 0 is a prompt block, not a decode step (a search that starts from the
        start token alone, models/blip_vqa.py:97): it takes the T > 1 route, so its K/V land at slots r*arena_slot_stride.

        cross_kv_len (i32 [rows], device; default None: every one of cross.Te keys): query batch r attends to the first
        cross_kv_len[r] keys of its encoder unit only (a decoder over padded question states: models/blip_vqa.py:69-76,125-129).

        route: the CrossRoute of ``cross``, from a caller that built it already — instead of the cross_* keywords, of which this
        call otherwise builds it, once.

        hidden_out (a list; BertModel.forward(output_hidden_states=True)): receives a f32 [rows*T, C] copy of the normalised
        hidden states after every layer run.  Not built for the parity precision mode.
        """
        p = self.packed()
        cfg = self.config
        H, C = cfg.num_attention_heads, cfg.hidden_size
        eps = cfg.layer_norm_eps
        M = rows * T
        dev = h32.device
        cdt = h16.dtype
        if p["parity"] and hidden_out is not None:
            raise K.VidilHipError("run_layers: hidden_out (per-layer hidden states) is not built for the parity precision mode")
        if p["parity"]:
            if self_done_first or stop_after_self or n_layers is not None:
                raise K.VidilHipError("run_layers: the parity precision mode runs whole stacks (the caption decoder, "
                                      "BertModel.encode); encode_cls' split schedules are not built for it — BLIP_ITM.itm_pairs "
                                      "takes encode_cls_parity (or the encode() route) in that mode")
            if cross_kv_len is not None:
                raise K.VidilHipError("run_layers: cross_kv_len (masked cross-attention) is not built for the parity precision mode")
            if arena_prompt:
                raise K.VidilHipError("run_layers: a one-token prompt block (arena_prompt) is not built for the parity precision mode")
        if arena is not None and T > 1 and t_off != 0:
            raise K.VidilHipError("run_layers: a multi-token block can only be appended to a beam arena at position 0")
        if route is None:
            route = CrossRoute(self, cross, rows, index=cross_index, group=cross_group, groups=cross_groups, max_group=cross_max_group,
                               kv_len=cross_kv_len)
        if p["parity"]:
            return parity_layers(self, p, h32, h16, rows=rows, T=T, causal=causal, kv_len=kv_len, route=route, self_k=self_k,
                                 self_vt=self_vt, t_off=t_off, Tk_cap=Tk_cap, NPs=NPs, ws=ws, arena=arena,
                                 arena_slot_stride=arena_slot_stride)
        if fused is None:
            # encoder batches with cross-attention (the ITM pairs) run without LayerNorm launches, WHATEVER their size: a
            # pair's logits must not depend on how many other pairs share its batch (ranks / tail batches of different
            # sizes write the same JSON), so the choice cannot depend on M.
            # Decoder sessions (arena) state their choice themselves (DecoderSession.fused_ln), for the same reason.
            fused = self._text_fold_ok(cdt) and cross is not None and arena is None and not stop_after_self
        elif fused and not (self._text_fold_ok(cdt) and cross is not None and not stop_after_self):
            raise K.VidilHipError("run_layers(fused=True): the LN-folded text stack needs cross-attention layers, 16-bit operands and "
                                  "hidden_size % 64 == 0, <= 1024")
        if fused:
            return self._run_layers_fused(h32, h16, rows=rows, T=T, self_k=self_k, self_vt=self_vt, t_off=t_off, Tk_cap=Tk_cap,
                                          NPs=NPs, causal=causal, kv_len=kv_len, route=route, n_layers=n_layers,
                                          self_done_first=self_done_first, arena=arena, arena_slot_stride=arena_slot_stride,
                                          arena_prompt=arena_prompt, hidden_out=hidden_out)
        if ws is None:
            ws = {}
        q = ws.get("q")
        if q is None or q.shape[0] < rows or q.shape[2] != T:
            q = torch.empty((rows, H, T, 64), dtype=cdt, device=dev)
            ws["q"] = q
        o = torch.empty((M, C), dtype=cdt, device=dev)
        tmp = torch.empty((M, C), dtype=torch.float32, device=dev)
        inter = torch.empty((M, cfg.intermediate_size), dtype=cdt, device=dev)
        Nk = t_off + T
        # n_layers: only the first n (encode_cls runs the last itself).  self_done_first / stop_after_self split layer
        # 0 after its self-attention block (dense + residual + LayerNorm included): that block does not see the image,
        # so encode_cls runs it once per TEXT and the rest of the stack once per (image, text) pair.
        for i, d in enumerate(p["layers"][:n_layers]):
            if self_done_first and i == 0:
                pass
            elif arena is not None and T == 1 and not arena_prompt:
                K.gemm(h16, d["qkv_w"], d["qkv_b"],
                       arena=dict(q=q, k=arena.k[i], v=arena.v[i], T=1, H=H, part0=0, t_off=t_off, Tcap=arena.Tcap,
                                  arena_rows=arena.rows, slot_stride=1, q_scale=0.125))
                K.beam_attention(q, arena.k[i], arena.v[i], arena.anc, o, rows=rows, H=H, n_keys=Nk)
            else:
                K.gemm(h16, d["qkv_w"], d["qkv_b"],
                       heads=dict(q=q, k=self_k[i], vt=self_vt[i], T=T, H=H, part0=0, t_off=t_off, Tq_cap=T,
                                  Tk_cap=Tk_cap, NP=NPs, q_scale=0.125))
                K.attention(q, self_k[i], self_vt[i], o, Bq=rows, H=H, Nq=T, Nk=Nk, Tq_cap=T, Tk_cap=Tk_cap, NP=NPs,
                            causal=causal, causal_off=t_off, kv_len=kv_len)
                if arena is not None:   # the prompt's K/V, once more, in the arena layout (a prompt is a few tokens)
                    K.gemm(h16, d["qkv_w"][C:], d["qkv_b"][C:],
                           arena=dict(k=arena.k[i], v=arena.v[i], T=T, H=H, part0=1, t_off=0, Tcap=arena.Tcap,
                                      arena_rows=arena.rows, slot_stride=arena_slot_stride))
            if not (self_done_first and i == 0):
                K.gemm(o, d["ao_w"], d["ao_b"], out=tmp, resid=h32)
                K.layernorm(tmp, d["ao_g"], d["ao_bt"], eps, out16=h16, out32=h32)
            if stop_after_self:
                break
            if cross is not None:
                self.cross_block(i, d, route, q, o, tmp, h32, h16, T)
            K.gemm(h16, d["i_w"], d["i_b"], out=inter, act=K.ACT_GELU_ERF)
            K.gemm(inter, d["o_w"], d["o_b"], out=tmp, resid=h32)
            K.layernorm(tmp, d["o_g"], d["o_bt"], eps, out16=h16, out32=h32)
            if hidden_out is not None:
                hidden_out.append(h32.clone())
        return h32, h16

    def cross_block(self, i, d, route, q, o, tmp, h32, h16, T):
        """The cross-attention block of layer i on the plain unfused path of ``run_layers`` (models/med.py:228-239 with encoder
        states): query, the route's attention launches, dense + residual, LayerNorm — on run_layers' scratch (q, o, tmp).
        nlvr_encoder.BertModel overrides it with the twin block."""
        H, eps = self.config.num_attention_heads, self.config.layer_norm_eps
        K.gemm(h16, d["cq_w"], d["cq_b"], heads=dict(q=q, T=T, H=H, part0=0, Tq_cap=T, q_scale=0.125))
        route.attend(i, q, o, T)
        K.gemm(o, d["co_w"], d["co_b"], out=tmp, resid=h32)
        K.layernorm(tmp, d["co_g"], d["co_bt"], eps, out16=h16, out32=h32)

    #: vidil_attention's short kernels end here; past it the long-key form serves MORE than 32 query rows per unit on plain K / V,
    #: the key-split form at most 32 on fragment tiles (a decoder session's: kv_tiled = 2)
    LONG_KEYS = 768

    def _text_fold_ok(self, cdt):
        C = self.config.hidden_size
        return (os.environ.get("VIDIL_FUSE_LN", "1") != "0" and C % 64 == 0 and C <= 1024
                and cdt in (torch.float16, torch.bfloat16))

    def decoder_fused_ln(self, cdt):
        """Whether the decoder passes over this trunk (a DecoderSession's, ``causal_pass``) run the LN-folded stack: a property of
        the model and $VIDIL_DECODE_FUSE_LN (=0: the unfused launches), never of a batch."""
        return (os.environ.get("VIDIL_DECODE_FUSE_LN", "1") != "0" and not self.parity and self._text_fold_ok(cdt)
                and self.config.add_cross_attention)

    def scratch_kv(self, rows, T, cdt, dev):
        """The self-attention K [rows,H,T,64] / V^T [rows,H,64,NPs] of ONE layer, presented as [L][...] to ``run_layers``: a block
        that attends to itself keeps no cache, so every layer reuses the pair.  Returns (k, vt, NPs)."""
        H, L = self.config.num_attention_heads, self.config.num_hidden_layers
        NPs = (T + 15) // 16 * 16
        k = torch.empty((1, rows, H, T, 64), dtype=cdt, device=dev).expand(L, -1, -1, -1, -1)
        vt = torch.empty((1, rows, H, 64, NPs), dtype=cdt, device=dev).expand(L, -1, -1, -1, -1)
        return k, vt, NPs

    def _run_layers_fused(self, h32, h16, *, rows, T, self_k, self_vt, t_off, Tk_cap, NPs, causal, kv_len, route=None, n_layers=None,
                          self_done_first=False, stop_after_self=False, state_in=None, arena: "BeamArena" = None, arena_slot_stride=1,
                          arena_prompt=False, hidden_out=None):
        """run_layers for encoder batches with cross-attention, WITHOUT LayerNorm launches between the GEMMs
        (models/med.py:236-239,306-317 are post-LN: h = LN(x + dense(.)) is the next dense's input AND the next residual).
        The stream is kept as the RAW sums u (f32 in h32's storage, a 16-bit copy in h16's) plus per-row (sum, sum of
        squares) partials written by the producing GEMM's epilogue; a consumer GEMM normalises its A rows algebraically
        (ln_fold: gamma-scaled weights, mean / rstd applied to the accumulators) and a residual GEMM normalises the
        residual rows on the way in (rln_gamma / rln_beta).  One LayerNorm launch at the end restores the (h32, h16)
        contract for the caller.  Same arithmetic as run_layers up to the rounding point of the GEMM operands (raw u
        instead of LN(u) is rounded to 16 bits).
        stop_after_self: run layer 0's self-attention block only and return the RAW state (h32, h16, partials, (gamma,
        beta)) — what encode_cls computes once per distinct text; state_in = (partials, (gamma, beta)): start from such
        a state (h32 / h16 hold raw sums), so the per-text front and the per-pair rest are the same arithmetic as one
        pass over the expanded batch.
        arena (round 6, the caption decoder: models/med.py:228-239,291-317,333-383 through the same folds): as run_layers — with
        T == 1 the new key / value of row r go to arena[position t_off][slot r] straight from the (LN-folded) Q|K|V GEMM's epilogue
        and attention follows the ancestry table; the prompt block (T > 1, t_off == 0) attends to itself and its K / V are also
        written to the arena at slots r * arena_slot_stride by a second, equally folded, K|V GEMM."""
        p = self.packed()
        fw = self._folded(p)
        cfg = self.config
        H, C = cfg.num_attention_heads, cfg.hidden_size
        eps = cfg.layer_norm_eps
        M = rows * T
        dev, cdt = h32.device, h16.dtype
        q = torch.empty((rows, H, T, 64), dtype=cdt, device=dev)
        o = torch.empty((M, C), dtype=cdt, device=dev)
        inter = torch.empty((M, cfg.intermediate_size), dtype=cdt, device=dev)
        stats = [torch.empty((M, C // 64, 2), dtype=torch.float32, device=dev) for _ in range(2)]
        cur = 0                      # stats[cur] describes the raw stream when `pend` is set
        pend = None                  # (gamma, beta) of the LayerNorm still owed to the stream; None: h32 / h16 are normalised
        if state_in is not None:
            stats[0], pend = state_in
        Nk = t_off + T

        def residual_gemm(a, w, b, ln_g, ln_b):
            """stream <- LN_pending(stream) + a·w^T + b, left RAW with fresh partials; (ln_g, ln_b) become pending."""
            nonlocal cur, pend
            kw = dict(out=h32, resid=h32, out16=h16, ln_stats_out=stats[cur ^ 1])
            if pend is not None:
                kw["rln"] = (pend[0], pend[1], eps, stats[cur])
            K.gemm(a, w, b, **kw)
            cur ^= 1
            pend = (ln_g, ln_b)

        def consumer(name, i, w, b, **kw):
            """a GEMM whose A operand is the stream: plain when it is normalised, LN-folded when a LayerNorm is pending."""
            if pend is None:
                return K.gemm(h16, w, b, **kw)
            wf, bf, cs = fw[i][name]
            return K.gemm(h16, wf, bf, ln=(cs, eps, stats[cur]), **kw)

        def arena_kv(i, d):
            """the prompt block's K | V once more, in the arena layout (a prompt is a few tokens): the K|V rows of the same
            (folded) weights — same values as the per-head K / V the block attends to"""
            kw = dict(arena=dict(k=arena.k[i], v=arena.v[i], T=T, H=H, part0=1, t_off=0, Tcap=arena.Tcap, arena_rows=arena.rows,
                                 slot_stride=arena_slot_stride))
            if pend is None:
                return K.gemm(h16, d["qkv_w"][C:], d["qkv_b"][C:], **kw)
            wf, bf, cs = fw[i]["qkv"]
            return K.gemm(h16, wf[C:], bf[C:], ln=(cs[C:], eps, stats[cur]), **kw)

        for i, d in enumerate(p["layers"][:n_layers]):
            if self_done_first and i == 0:
                pass
            elif arena is not None and T == 1 and not arena_prompt:
                consumer("qkv", i, d["qkv_w"], d["qkv_b"],
                         arena=dict(q=q, k=arena.k[i], v=arena.v[i], T=1, H=H, part0=0, t_off=t_off, Tcap=arena.Tcap,
                                    arena_rows=arena.rows, slot_stride=1, q_scale=0.125))
                K.beam_attention(q, arena.k[i], arena.v[i], arena.anc, o, rows=rows, H=H, n_keys=Nk)
                residual_gemm(o, d["ao_w"], d["ao_b"], d["ao_g"], d["ao_bt"])
            else:
                if arena is not None:
                    arena_kv(i, d)                     # (before the residual GEMM below replaces the stream it reads)
                consumer("qkv", i, d["qkv_w"], d["qkv_b"],
                         heads=dict(q=q, k=self_k[i], vt=self_vt[i], T=T, H=H, part0=0, t_off=t_off, Tq_cap=T, Tk_cap=Tk_cap,
                                    NP=NPs, q_scale=0.125))
                K.attention(q, self_k[i], self_vt[i], o, Bq=rows, H=H, Nq=T, Nk=Nk, Tq_cap=T, Tk_cap=Tk_cap, NP=NPs,
                            causal=causal, causal_off=t_off, kv_len=kv_len)
                residual_gemm(o, d["ao_w"], d["ao_b"], d["ao_g"], d["ao_bt"])
            if stop_after_self:
                return h32, h16, stats[cur], pend
            consumer("cq", i, d["cq_w"], d["cq_b"], heads=dict(q=q, T=T, H=H, part0=0, Tq_cap=T, q_scale=0.125))
            route.attend(i, q, o, T)
            residual_gemm(o, d["co_w"], d["co_b"], d["co_g"], d["co_bt"])
            consumer("fc1", i, d["i_w"], d["i_b"], out=inter, act=K.ACT_GELU_ERF)
            residual_gemm(inter, d["o_w"], d["o_b"], d["o_g"], d["o_bt"])
            if hidden_out is not None:   # (the stream is raw here: the layer's output LayerNorm into a buffer of its own)
                snap = torch.empty_like(h32)
                K.layernorm(h32, pend[0], pend[1], eps, out32=snap)
                hidden_out.append(snap)
        if pend is not None:         # hand the caller normalised (h32, h16) again
            K.layernorm(h32, pend[0], pend[1], eps, out16=h16, out32=h32)
        return h32, h16

    def embed(self, ids_i32, T, pos_off):
        """ids int32 [rows*T] -> (h32, h16) after the embedding LayerNorm (models/med.py:71-94)."""
        p = self.packed()
        C = self.config.hidden_size
        M = ids_i32.numel()
        dev = ids_i32.device
        cdt = p["layers"][0]["qkv_w"].dtype
        raw = torch.empty((M, C), dtype=torch.float32, device=dev)
        K.embed_tokens(ids_i32, p["word"], p["pos"], raw, T=T, pos_off=pos_off)
        h32 = torch.empty((M, C), dtype=torch.float32, device=dev)
        par = p["parity"]                 # parity precision mode: the 16-bit companion is [hi | lo | hi] rows
        h16 = torch.empty((M, 3 * C if par else C), dtype=cdt, device=dev)
        K.layernorm(raw, p["emb_g"], p["emb_b"], self.config.layer_norm_eps, out16=h16, out32=h32, split3=par)
        return h32, h16

    def encode(self, ids_i32, kv_len_i32, cross: CrossKV, cross_index=None, cross_groups=None, cross_max_group=0, cross_kv_len=None):
        """ITM encoder pass (models/blip_itm.py:51-56): ids int32 [P,T] right-padded, kv_len [P] = number of
        real tokens.  Pair p attends to image ``cross_index[p]``, or — image-major pair order — image j serves
        pairs cross_groups[j] .. cross_groups[j+1]-1.  cross_kv_len (i32 [P], device): pair p attends to the first
        cross_kv_len[p] encoder states of its unit only (run_layers).  Returns (h32, h16) [P*T, C]."""
        require_cuda(ids_i32, "BertModel.encode")
        P, T = ids_i32.shape
        h32, h16 = self.embed(ids_i32.reshape(-1), T, 0)
        return self.bidirectional_pass(h32, h16, P, T, kv_len_i32, cross, cross_index=cross_index, cross_groups=cross_groups,
                                       cross_max_group=cross_max_group, cross_kv_len=cross_kv_len)

    def bidirectional_pass(self, h32, h16, P, T, kv_len_i32, cross, *, hidden_out=None, **cross_kw):
        """The stack pass of ``encode`` on embedded rows (h32, h16) [P*T, C], updated in place: every token attends to the first
        kv_len[p] tokens of its sequence and to ``cross`` (cross_kw: cross_index / cross_groups / cross_max_group / cross_kv_len)."""
        sk, sv, NPs = self.scratch_kv(P, T, h16.dtype, h32.device)
        self.run_layers(h32, h16, rows=P, T=T, self_k=sk, self_vt=sv, t_off=0, Tk_cap=T, NPs=NPs, causal=False,
                        kv_len=kv_len_i32, cross=cross, hidden_out=hidden_out, **cross_kw)
        return h32, h16

    def causal_pass(self, h32, h16, rows, T, cross, *, kv_len=None, hidden_out=None, **cross_kw):
        """The stack pass of ``BertLMHeadModel.score`` / ``start_logits`` on embedded rows (h32, h16) [rows*T, C], updated in
        place: every block of T tokens attends causally to itself through one scratch K / V^T pair shared by all layers (as
        DecoderSession.prefill does for a prompt) and to ``cross`` (cross_kw: cross_index / cross_groups / cross_max_group /
        cross_kv_len).  The stack is the one a DecoderSession runs (LN-folded or parity) — never a function of the batch.
        kv_len (i32 [rows], device): a row also ignores the keys past kv_len[r] (models/med.py:651, causal x padding mask);
        a query inside its sequence sees the same keys with and without it."""
        sk, sv, NPs = self.scratch_kv(rows, T, h16.dtype, h32.device)
        self.run_layers(h32, h16, rows=rows, T=T, self_k=sk, self_vt=sv, t_off=0, Tk_cap=T, NPs=NPs, causal=True, kv_len=kv_len,
                        cross=cross, fused=self.decoder_fused_ln(h16.dtype) and cross is not None, hidden_out=hidden_out, **cross_kw)
        return h32, h16

    def encode_cls(self, ids_i32, kv_len_i32, cross: CrossKV, cross_index=None, cross_groups=None, cross_max_group=0,
                   pair_text=None):
        """encode() for consumers of the [CLS] position only (the ITM head, models/blip_itm.py:57): same arguments,
        returns (h32, h16) [P, C] — token 0 of every pair after the last layer.

        Layers 0..L-2 run on every token.  In the last layer only the keys and values of the self-attention depend on
        the other tokens, so it computes K|V for all P*T rows and everything else — the query, both attention
        outputs, the three dense+LayerNorm blocks and the feed-forward — for the P [CLS] rows alone (1/T of the
        layer's GEMM rows).  The arithmetic per [CLS] row is unchanged.  Needs ``cross.last_vt`` when the cross
        values are row-major (one query row per pair goes through the direct attention kernel).

        ``pair_text`` (int64 [P], device): ids / kv_len then describe U distinct TEXTS and pair p uses text
        pair_text[p] (CapFilt scores every caption of a video against each of its F frames).  Everything before
        the first cross-attention — the embedding and layer 0's self-attention block — is computed once per text
        and its rows are copied out to the pairs; same bits as running it per pair."""
        require_cuda(ids_i32, "BertModel.encode_cls")
        p = self.packed()
        cfg = self.config
        T = ids_i32.shape[1]
        H, C, L = cfg.num_attention_heads, cfg.hidden_size, cfg.num_hidden_layers
        eps = cfg.layer_norm_eps
        dev = ids_i32.device
        cdt = p["layers"][0]["qkv_w"].dtype
        if cross is not None and cross.NP == 0 and cross.last_vt is None:
            raise K.VidilHipError("encode_cls: row-major cross values need project_cross_kv(last_layer_vt=True)")
        h32, h16 = self.embed(ids_i32.reshape(-1), T, 0)
        shared = pair_text is not None and cross is not None and L > 1
        fold = self._text_fold_ok(cdt) and cross is not None and L > 1
        state = None
        if shared:
            U = ids_i32.shape[0]
            uk, uv, NPs = self.scratch_kv(U, T, cdt, dev)
            kw = dict(rows=U, T=T, self_k=uk, self_vt=uv, t_off=0, Tk_cap=T, NPs=NPs, causal=False, kv_len=kv_len_i32, n_layers=1,
                      stop_after_self=True)
            if fold:     # the text-only front leaves the raw sum + partials, exactly as the expanded batch's layer 0 would
                h32, h16, st0, pend0 = self._run_layers_fused(h32, h16, **kw)
                state = (st0.view(U, T, -1).index_select(0, pair_text).view(-1, st0.shape[1], 2).contiguous(), pend0)
            else:
                self.run_layers(h32, h16, cross=None, **kw)
            h32 = h32.view(U, T, C).index_select(0, pair_text).view(-1, C)
            h16 = h16.view(U, T, C).index_select(0, pair_text).view(-1, C)
            kv_len_i32 = kv_len_i32.index_select(0, pair_text).contiguous()
        elif pair_text is not None:
            h32 = h32.view(-1, T, C).index_select(0, pair_text).view(-1, C)
            h16 = h16.view(-1, T, C).index_select(0, pair_text).view(-1, C)
            kv_len_i32 = kv_len_i32.index_select(0, pair_text).contiguous()
        P = h32.shape[0] // T
        sk_l, sv_l, NPs = self.scratch_kv(P, T, cdt, dev)
        sk, sv = sk_l[0], sv_l[0]
        route = CrossRoute(self, cross, P, index=cross_index, groups=cross_groups, max_group=cross_max_group)
        kw = dict(rows=P, T=T, self_k=sk_l, self_vt=sv_l, t_off=0, Tk_cap=T, NPs=NPs, causal=False, kv_len=kv_len_i32, route=route,
                  n_layers=L - 1, self_done_first=shared)
        if state is not None:
            self._run_layers_fused(h32, h16, state_in=state, **kw)
        else:
            self.run_layers(h32, h16, cross=cross, **kw)
        d = p["layers"][L - 1]
        q1 = torch.empty((P, H, 1, 64), dtype=cdt, device=dev)
        o1 = torch.empty((P, C), dtype=cdt, device=dev)
        tmp = torch.empty((P, C), dtype=torch.float32, device=dev)
        c16 = torch.empty((P, C), dtype=cdt, device=dev)
        c32 = h32.view(P, T, C)[:, 0].contiguous()
        # self-attention: keys / values of every token, query of token 0 (A rows p*T of h16: strided operand)
        K.gemm(h16, d["qkv_w"][C:], d["qkv_b"][C:], heads=dict(k=sk, vt=sv, T=T, H=H, part0=1, t_off=0, Tk_cap=T, NP=NPs))
        K.gemm(h16.view(-1), d["qkv_w"][:C], d["qkv_b"][:C], M=P, lda=T * C,
               heads=dict(q=q1, T=1, H=H, part0=0, Tq_cap=1, q_scale=0.125))
        K.attention(q1, sk, sv, o1, Bq=P, H=H, Nq=1, Nk=T, Tq_cap=1, Tk_cap=T, NP=NPs, causal=False, causal_off=0,
                    kv_len=kv_len_i32)
        K.gemm(o1, d["ao_w"], d["ao_b"], out=tmp, resid=c32)
        K.layernorm(tmp, d["ao_g"], d["ao_bt"], eps, out16=c16, out32=c32)
        if cross is not None:
            vt, NP = (cross.vt[L - 1], cross.NP) if cross.last_vt is None else (cross.last_vt, cross.last_NP)
            K.gemm(c16, d["cq_w"], d["cq_b"], heads=dict(q=q1, T=1, H=H, part0=0, Tq_cap=1, q_scale=0.125))
            # (over LONG_KEYS encoder states: the bound becomes max(max_group, 33) — one query row per pair)
            K.attention(q1, cross.k[L - 1], vt, o1, Bq=P, H=H, Nq=1, Nk=cross.Te, Tq_cap=1, Tk_cap=cross.Te, NP=NP,
                        kv_index=route.index, group_start=route.groups, max_group=route.bound(1))
            K.gemm(o1, d["co_w"], d["co_b"], out=tmp, resid=c32)
            K.layernorm(tmp, d["co_g"], d["co_bt"], eps, out16=c16, out32=c32)
        inter = K.gemm(c16, d["i_w"], d["i_b"], act=K.ACT_GELU_ERF)
        K.gemm(inter, d["o_w"], d["o_b"], out=tmp, resid=c32)
        K.layernorm(tmp, d["o_g"], d["o_bt"], eps, out16=c16, out32=c32)
        return c32, c16

    def cls_last_parity_ok(self, cross):
        """encode_cls_parity serves this model and these cross K / V: the parity mode with an f32-row attention kind (cross K | V
        as f32 rows: project_cross_kv's parity form) and more than one layer."""
        return (self.parity and parity_attention_f32(self) and self.config.num_hidden_layers > 1
                and (cross is None or cross.f32))

    def encode_cls_parity(self, ids_i32, kv_len_i32, cross: CrossKV, cross_index=None, cross_groups=None, cross_max_group=0):
        """encode_cls in the parity precision mode (f32-row attention kinds; cls_last_parity_ok): layers 0..L-2 on every token
        (parity_layers), the last layer's keys / values of the self-attention over every token, and everything else of that
        layer — the query, both attentions, the three dense + LayerNorm blocks and the feed-forward — on the P [CLS] rows alone.
        Same operands per [CLS] row as encode(); the one-row self-attention is vidil_attention_f32's one-row-per-unit form.
        Returns (c32 f32 [P, C], c3 [P, 3C] = its [hi | lo | hi] rows)."""
        require_cuda(ids_i32, "BertModel.encode_cls_parity")
        if not self.cls_last_parity_ok(cross):
            raise K.VidilHipError("encode_cls_parity: needs the parity mode with the 'split' or 'f32' attention kind, more than one "
                                  "layer and f32-row cross K | V (project_cross_kv in the same mode)")
        p = self.packed()
        cfg = self.config
        P, T = ids_i32.shape
        H, C, L = cfg.num_attention_heads, cfg.hidden_size, cfg.num_hidden_layers
        eps = cfg.layer_norm_eps
        dev = ids_i32.device
        arith = parity_attention_arith(self)
        h32, h3 = self.embed(ids_i32.reshape(-1), T, 0)
        cdt = h3.dtype
        ws = {}
        route = CrossRoute(self, cross, P, index=cross_index, groups=cross_groups, max_group=cross_max_group)
        parity_layers(self, p, h32, h3, rows=P, T=T, causal=False, kv_len=kv_len_i32, route=route, ws=ws, n_layers=L - 1)
        planes_h = ws["planes_h"]            # (planes of h3 the last LayerNorm wrote; the [CLS] side below writes all three)
        d = p["layers"][L - 1]
        kv32 = torch.empty((P * T, 2 * C), dtype=torch.float32, device=dev)
        K.gemm(h3, d["qkv_w3"][C:], d["qkv_b"][C:], out=kv32, split_k=True, a_planes=planes_h)
        c32 = h32.view(P, T, C)[:, 0].contiguous()
        c3 = h3.view(P, T, 3 * C)[:, 0].contiguous()
        q32 = torch.empty((P, C), dtype=torch.float32, device=dev)
        o3 = torch.empty((P, 3 * C), dtype=cdt, device=dev)
        tmp = torch.empty((P, C), dtype=torch.float32, device=dev)
        K.gemm(c3, d["qkv_w3"][:C], d["qkv_b"][:C], out=q32, split_k=True, a_planes=planes_h)
        K.attention_f32(q32, kv32[:, :C], kv32[:, C:], o3, Bq=P, H=H, Nq=1, Nk=T, kv_rows=T, kv_len=kv_len_i32, arith=arith)
        K.gemm(o3, d["ao_w3"], d["ao_b"], out=tmp, resid=c32, split_k=True)
        K.layernorm(tmp, d["ao_g"], d["ao_bt"], eps, out16=c3, out32=c32, split3=True)
        if cross is not None:
            K.gemm(c3, d["cq_w3"], d["cq_b"], out=q32, split_k=True)
            kv = cross.k[L - 1]                                     # f32 [B, Te, 2C]: keys | values
            K.attention_f32(q32, kv[..., :C], kv[..., C:], o3, Bq=P, H=H, Nq=1, Nk=cross.Te, kv_rows=cross.Te, kv_index=route.index,
                            group_start=route.groups, max_group=route.max_group, arith=arith)
            K.gemm(o3, d["co_w3"], d["co_b"], out=tmp, resid=c32, split_k=True)
            K.layernorm(tmp, d["co_g"], d["co_bt"], eps, out16=c3, out32=c32, split3=True)
        inter3 = torch.empty((P, 3 * cfg.intermediate_size), dtype=cdt, device=dev)
        K.gemm(c3, d["i_w3"], d["i_b"], split3_out=inter3, act=K.ACT_GELU_ERF, split_k=True)
        K.gemm(inter3, d["o_w3"], d["o_b"], out=tmp, resid=c32, split_k=True)
        K.layernorm(tmp, d["o_g"], d["o_bt"], eps, out16=c3, out32=c32, split3=True)
        return c32, c3

    # ------------------------------------------------------------------ the reference's call surface
    def masked_pass(self, h32, h16, B, T, keep=None, *, causal=False, cross=None, cross_kv_len=None, hidden_out=None):
        """The stack on embedded rows (h32, h16) [B*T, C] under a 0/1 key mask ``keep`` (bool [B, T], device; None: all ones):
        the rows with mask 1 are moved to the front of their sequence in their original order (attention does not depend on
        the order of its keys, and the positions are already in the embedding), the stack runs with their count as ``kv_len``
        (``bidirectional_pass``, or ``causal_pass`` — the stable order keeps the causal relation among the kept rows), and the
        rows are moved back.  A mask whose ones form a prefix moves nothing: the launches and bits are those of ``encode`` /
        ``causal_pass`` on the same lengths.  The permutation is computed on the device; nothing is read back.
        Returns new (h32, h16); hidden_out receives the per-layer states in the caller's row order."""
        if keep is None:
            rows, kv_len = None, None
        else:
            order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)          # kept rows first, original order
            rows = (torch.arange(B, device=keep.device)[:, None] * T + order).reshape(-1)
            kv_len = keep.sum(1).to(torch.int32).contiguous()
            h32, h16 = h32.index_select(0, rows), h16.index_select(0, rows)
        kw = {} if cross_kv_len is None else dict(cross_kv_len=cross_kv_len)
        states = None if hidden_out is None else []
        if causal:
            self.causal_pass(h32, h16, B, T, cross, kv_len=kv_len, hidden_out=states, **kw)
        else:
            self.bidirectional_pass(h32, h16, B, T, kv_len, cross, hidden_out=states, **kw)
        if rows is not None:
            def back(x):
                return torch.empty_like(x).index_copy_(0, rows, x)
            h32, h16 = back(h32), back(h16)
            states = None if states is None else [back(x) for x in states]
        if states is not None:
            hidden_out.extend(states)
        return h32, h16

    def _cross_for_forward(self, encoder_hidden_states, encoder_attention_mask, B, Tq):
        """forward's cross-attention keys / values: encoder states [B, Te, width] (f32 or the 16-bit type) under a 0/1 mask
        [B, Te] -> (CrossKV, cross_kv_len).  With a mask the kept rows of each unit are moved to its front before the K | V
        projection and their count becomes cross_kv_len.  More than LONG_KEYS states: plain rows for more than 32 query rows
        per unit (the long-key form), fragment tiles otherwise (the key-split form)."""
        enc = encoder_hidden_states
        Te, W = enc.shape[1], enc.shape[2]
        enc16 = enc.to(self.cdt).reshape(B * Te, W)
        ckl = None
        if encoder_attention_mask is not None:
            keep = encoder_attention_mask.to(enc.device) != 0
            order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)
            rows = (torch.arange(B, device=enc.device)[:, None] * Te + order).reshape(-1)
            enc16 = enc16.index_select(0, rows)
            ckl = keep.sum(1).to(torch.int32).contiguous()
        long_keys = Te > self.LONG_KEYS
        kw = dict(tiled=True) if long_keys and Tq <= 32 else dict(v_rowmajor=Tq > 32)
        return self.project_cross_kv(enc16.contiguous(), B, Te, kv_len=ckl, **kw), ckl

    def _forward_states(self, name, input_ids, attention_mask, encoder_hidden_states, encoder_attention_mask, output_hidden_states,
                        is_decoder, mode, refused):
        """What both ``forward``s run: checks first (nothing is launched that would fail), then the embedding and ``masked_pass``.
        Returns (h32, h16, Tp, last, hidden): h32 / h16 [B*Tp, C] are the states of B blocks of Tp >= T tokens (a causal call
        runs on blocks of at least SCORE_MIN_TOKENS tokens, as ``BertLMHeadModel.score`` does; the added positions are padding);
        ``last`` f32 [B, T, C] and ``hidden`` (a tuple of L + 1 such tensors, or None) are cut to the caller's T tokens."""
        for arg, value in refused:
            if value is not None and value is not False:
                raise NotImplementedError(f"{name}: {arg}{'=True' if value is True else ''} is not served (BertModel.forward's "
                                          "docstring lists what is)")
        if isinstance(encoder_hidden_states, (list, tuple)):
            raise NotImplementedError(f"{name}: a list as encoder_hidden_states (the NLVR encoder's call, models/med.py:748) is not served")
        if mode not in ("text", "multimodal"):
            raise NotImplementedError(f"{name}: mode={mode!r} is not served (text | multimodal)")
        if input_ids is None:
            raise ValueError(f"{name}: input_ids is required")
        if self.parity:
            raise NotImplementedError(f"{name}: the parity precision mode is not served (BertModel.encode / BertLMHeadModel.score are)")
        require_cuda(input_ids, name)
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"{name}: input_ids must be int64 or int32 [B, T], got {input_ids.dtype} {tuple(input_ids.shape)}")
        cfg = self.config
        B, T = input_ids.shape
        dev = input_ids.device
        Tp = max(SCORE_MIN_TOKENS, T) if is_decoder else T
        enc = encoder_hidden_states if mode == "multimodal" else None
        if enc is not None and not hasattr(self.encoder.layer[0], "crossattention"):
            raise ValueError(f"{name}: encoder_hidden_states given to a model built without cross-attention layers")
        if enc is not None and (enc.dim() != 3 or enc.shape[0] != B or enc.shape[2] != cfg.encoder_width or not enc.is_cuda):
            raise ValueError(f"{name}: encoder_hidden_states must be [{B}, Te, {cfg.encoder_width}] on the device, got {tuple(enc.shape)}")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, T):
            raise ValueError(f"{name}: attention_mask must be [{B}, {T}] of 0 / 1, got {tuple(attention_mask.shape)}")
        if enc is not None and encoder_attention_mask is not None and tuple(encoder_attention_mask.shape) != (B, enc.shape[1]):
            raise ValueError(f"{name}: encoder_attention_mask must be [{B}, {enc.shape[1]}] of 0 / 1, got "
                             f"{tuple(encoder_attention_mask.shape)}")
        # ---- the attention kernels' own limits
        if Tp > self.LONG_KEYS:
            raise K.VidilHipError(f"{name}: {B} x {T} tokens: self-attention over more than {self.LONG_KEYS} keys"
                                  f"{' under a causal mask' if is_decoder else ''} is not served by the attention kernels")
        if Tp > cfg.max_position_embeddings:
            raise ValueError(f"{name}: a block of {Tp} tokens exceeds max_position_embeddings={cfg.max_position_embeddings}")
        if enc is not None and enc.shape[1] > MAX_VIDEO_TOKENS:
            raise K.VidilHipError(f"{name}: {T} query rows over {enc.shape[1]} encoder states: more than {MAX_VIDEO_TOKENS} keys are not "
                                  "served by the attention kernels")
        ids = input_ids.to(torch.int32)
        keep = None if attention_mask is None else attention_mask.to(dev) != 0
        if Tp != T:
            ids = torch.cat([ids, torch.full((B, Tp - T), cfg.pad_token_id, dtype=torch.int32, device=dev)], 1)
            keep = torch.arange(Tp, device=dev)[None, :].expand(B, -1) < T if keep is None else \
                torch.cat([keep, torch.zeros((B, Tp - T), dtype=torch.bool, device=dev)], 1)
        cross, ckl = (None, None) if enc is None else self._cross_for_forward(enc, encoder_attention_mask, B, Tp)
        h32, h16 = self.embed(ids.reshape(-1).contiguous(), Tp, 0)
        hidden = [h32.clone()] if output_hidden_states else None
        h32, h16 = self.masked_pass(h32, h16, B, Tp, keep, causal=bool(is_decoder), cross=cross, cross_kv_len=ckl, hidden_out=hidden)

        def cut(x):
            x = x.view(B, Tp, -1)
            return x if Tp == T else x[:, :T].contiguous()
        return h32, h16, Tp, cut(h32), None if hidden is None else tuple(cut(x) for x in hidden)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, head_mask=None, inputs_embeds=None,
                encoder_embeds=None, encoder_hidden_states=None, encoder_attention_mask=None, past_key_values=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None, is_decoder=False,
                mode='multimodal'):
        """The reference's call (models/med.py:670-807) over the library's kernels.

        Served: input_ids int64 / int32 [B, T] on the device; attention_mask [B, T] of 0 / 1 (default: ones);
        encoder_hidden_states f32 or 16-bit [B, Te, width] with encoder_attention_mask [B, Te] (default: ones); mode 'text'
        (no cross-attention) or 'multimodal'; is_decoder False (bidirectional) or True (causal and padding mask, :609-668);
        output_hidden_states; return_dict (None: True).  Returns an object with ``last_hidden_state`` f32 [B, T, C],
        ``hidden_states`` (a tuple of L + 1 f32 [B, T, C] when asked, else None) and ``pooler_output`` None (no model here
        builds the pooler); with return_dict=False the tuple (last_hidden_state, None[, hidden_states]).
        Refused by a NotImplementedError that names the argument, before any launch: position_ids, head_mask, inputs_embeds,
        encoder_embeds, past_key_values, use_cache=True, output_attentions=True, a list as encoder_hidden_states, and the
        parity precision mode.

        Masks (``masked_pass``).  A mask whose ones form a prefix of every row is what the kernels' ``kv_len`` expresses: the
        call issues the launches of ``encode`` on the same ids and lengths, with the same bits.  is_decoder: the kernels and, for
        the rows inside a sequence, the bits of the teacher-forced pass of ``BertLMHeadModel.score``; the self-attention launch
        is not identical — ``kv_len`` is passed besides the causal mask (``score`` passes none), so that padded rows agree with
        the reference too.  With a prefix mask EVERY row agrees with the reference, padded positions included.  With any other
        0 / 1 pattern (left padding, holes) only the positions whose mask is 1 are specified.  A row whose mask is all zero is
        outside the contract.  encoder_attention_mask: the same, on the encoder states of each batch element.
        Limits (VidilHipError naming the shape, nothing launched): more than LONG_KEYS tokens; more than 16,384 encoder states.
        Cost: the cross K | V of every layer are projected in every call (the library's own entry points project them once per
        image).  No backward pass."""
        refused = (("position_ids", position_ids), ("head_mask", head_mask), ("inputs_embeds", inputs_embeds),
                   ("encoder_embeds", encoder_embeds), ("past_key_values", past_key_values), ("use_cache", use_cache),
                   ("output_attentions", output_attentions))
        _, _, _, last, hidden = self._forward_states("BertModel.forward", input_ids, attention_mask, encoder_hidden_states,
                                                     encoder_attention_mask, bool(output_hidden_states), is_decoder, mode, refused)
        if return_dict is not None and not return_dict:
            return (last, None) + (() if hidden is None else (hidden,))
        return ModelOutput(last_hidden_state=last, pooler_output=None, past_key_values=None, hidden_states=hidden,
                           attentions=None, cross_attentions=None)


class _LMTransform(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _LMPredictions(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.transform = _LMTransform(cfg)
        self.decoder = nn.Linear(cfg.hidden_size, cfg.vocab_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.decoder.bias = self.bias  # same aliasing as models/med.py:527-530


class _LMHead(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.predictions = _LMPredictions(cfg)


class BertLMHeadModel(PackedCache, nn.Module):
    """Caption decoder: ``bert`` trunk + ``cls`` LM head (models/med.py:811-955).

    ``precise_head`` (default: $VIDIL_PRECISE_LM_HEAD == "1"): run the two GEMMs of the LM head with
    error-compensated operands — activations and weights split into hi + lo 16-bit parts, the three significant
    cross terms accumulated by ONE GEMM with K tripled — so that the head adds ~2^-20 instead of ~2^-11 (f16) /
    2^-8 (bf16) relative rounding to the logits.  It is what the "caption logits within 1e-3" budget can afford
    to spend on precision: the head is 19 % of a decode step's FLOPs (x3 here), the trunk's operand rounding is
    untouched (DESIGN.md §4 has the measured split)."""

    def __init__(self, config):
        super().__init__()
        import os

        self.precise_head = os.environ.get("VIDIL_PRECISE_LM_HEAD", "0") == "1"
        self.config = config
        self.bert = BertModel(config, add_pooling_layer=False)
        self.cls = _LMHead(config)
        self.cls.apply(lambda m: _init_bert(m, config.initializer_range))

    def _pack(self):
        pr = self.cls.predictions
        c = self.cdt
        p = dict(t_w=w16(pr.transform.dense.weight, dtype=c), t_b=v32(pr.transform.dense.bias),
                 t_g=v32(pr.transform.LayerNorm.weight), t_bt=v32(pr.transform.LayerNorm.bias),
                 dec_w=w16(pr.decoder.weight, dtype=c), dec_b=v32(pr.bias), precise=self.precise_head or self.parity)
        if p["precise"]:
            p.update(t_w3=w3(pr.transform.dense.weight, dtype=c), dec_w3=w3(pr.decoder.weight, dtype=c))
        return p

    def pack_flags(self):
        return (self.precise_head, self.parity)

    def lm_logits(self, h16, rows, T, out=None, h32=None):
        """LM head (models/med.py:501-545) on the LAST token of each of ``rows`` sequences of length T:
        dense -> erf-GELU -> LayerNorm -> decoder(+bias).  h16: T16 [rows*T, C]; h32: the same hidden states in f32
        (used by the precise head).  Returns f32 [rows, V].
        (The reference computes logits for all T positions and HF generate() keeps only the last.)"""
        p = self.packed()
        cfg = self.config
        C = cfg.hidden_size
        dev = h16.device
        cdt = h16.dtype
        if p["precise"]:
            if h32 is None:
                raise K.VidilHipError("lm_logits: the error-compensated head (precise_head / parity mode) needs the f32 hidden states")
            last32 = h32.view(rows, T, C)[:, T - 1].contiguous()
            a3 = K.split3(last32, torch.empty((rows, 3 * C), dtype=cdt, device=dev))
            t32 = torch.empty((rows, C), dtype=torch.float32, device=dev)
            K.gemm(a3, p["t_w3"], p["t_b"], out=t32, act=K.ACT_GELU_ERF, split_k=True)
            tn32 = torch.empty((rows, C), dtype=torch.float32, device=dev)
            K.layernorm(t32, p["t_g"], p["t_bt"], cfg.layer_norm_eps, out32=tn32)
            K.split3(tn32, a3)
            if out is None:
                out = torch.empty((rows, cfg.vocab_size), dtype=torch.float32, device=dev)
            K.gemm(a3, p["dec_w3"], p["dec_b"], out=out, split_k=True)
            return out
        last = h16.view(-1)[(T - 1) * C:]  # row r of the strided view = token T-1 of sequence r
        t32 = torch.empty((rows, C), dtype=torch.float32, device=dev)
        K.gemm(last, p["t_w"], p["t_b"], out=t32, act=K.ACT_GELU_ERF, M=rows, lda=T * C)
        t16 = torch.empty((rows, C), dtype=cdt, device=dev)
        K.layernorm(t32, p["t_g"], p["t_bt"], cfg.layer_norm_eps, out16=t16)
        if out is None:
            out = torch.empty((rows, cfg.vocab_size), dtype=torch.float32, device=dev)
        K.gemm(t16, p["dec_w"], p["dec_b"], out=out)
        return out

    def lm_logits_rows(self, h16, row_index, out=None, h32=None):
        """LM head on an arbitrary list of hidden-state rows: row_index int [n] (device) into h16 [M, C] (h32 [M, C] for the
        error-compensated head) -> f32 [n, V].  The rows are gathered first, then the same two GEMMs and LayerNorm as
        ``lm_logits`` run on them; the vocabulary GEMM is issued HEAD_GEMM_ROWS rows at a time, always that many (the tail is
        padded with a repeated row), so every launch is the same kernel whatever n is.
        out: an f32 buffer of at least ceil(n / HEAD_GEMM_ROWS) * HEAD_GEMM_ROWS rows of V to write into (the result is its
        first n rows)."""
        p = self.packed()
        cfg = self.config
        C, V, G = cfg.hidden_size, cfg.vocab_size, HEAD_GEMM_ROWS
        dev, cdt = h16.device, h16.dtype
        n = row_index.numel()
        n_pad = (n + G - 1) // G * G
        if out is None:
            out = torch.empty((n_pad, V), dtype=torch.float32, device=dev)
        elif out.dim() != 2 or out.shape[0] < n_pad or out.shape[1] != V or out.dtype != torch.float32 or not out.is_contiguous():
            raise K.VidilHipError(f"lm_logits_rows: out must be a contiguous f32 [>= {n_pad}, {V}] buffer, got {out.dtype} {tuple(out.shape)}")
        if n == 0:
            return out[:0]
        idx = row_index.to(torch.int64)
        if n_pad != n:
            idx = torch.cat([idx, idx[:1].expand(n_pad - n)])
        t32 = torch.empty((n_pad, C), dtype=torch.float32, device=dev)
        if p["precise"]:
            if h32 is None:
                raise K.VidilHipError("lm_logits_rows: the error-compensated head (precise_head / parity mode) needs the f32 hidden states")
            a3 = K.split3(h32.index_select(0, idx), torch.empty((n_pad, 3 * C), dtype=cdt, device=dev))
            K.gemm(a3, p["t_w3"], p["t_b"], out=t32, act=K.ACT_GELU_ERF, split_k=True)
            tn32 = torch.empty((n_pad, C), dtype=torch.float32, device=dev)
            K.layernorm(t32, p["t_g"], p["t_bt"], cfg.layer_norm_eps, out32=tn32)
            K.split3(tn32, a3)
            for r0 in range(0, n_pad, G):
                K.gemm(a3[r0:r0 + G], p["dec_w3"], p["dec_b"], out=out[r0:r0 + G], split_k=True)
            return out[:n]
        K.gemm(h16.index_select(0, idx), p["t_w"], p["t_b"], out=t32, act=K.ACT_GELU_ERF)
        t16 = torch.empty((n_pad, C), dtype=cdt, device=dev)
        K.layernorm(t32, p["t_g"], p["t_bt"], cfg.layer_norm_eps, out16=t16)
        for r0 in range(0, n_pad, G):
            K.gemm(t16[r0:r0 + G], p["dec_w"], p["dec_b"], out=out[r0:r0 + G])
        return out[:n]

    def _causal_block_pass(self, ids_i32, rows, T, cross, **cross_kw):
        """The ONE stack pass of ``score`` and ``start_logits``: ids i32 [rows*T] (device) -> (h32, h16) [rows*T, C] after the
        embedding and ``BertModel.causal_pass``."""
        h32, h16 = self.bert.embed(ids_i32, T, 0)
        return self.bert.causal_pass(h32, h16, rows, T, cross, **cross_kw)

    @torch.no_grad()
    def start_logits(self, enc16, B, start_id, *, cross_kv_len=None):
        """Logits of the first generated token: one decoder pass of the start token alone per encoder unit
        (models/blip_vqa.py:123-130).  enc16: 16-bit [B*Te, width] encoder states of B units; cross_kv_len int [B]: real states
        per unit (the rest is padding, masked).  Returns f32 [B, V].

        Schedule: the pass ``score`` runs — the start token heads a causal block of SCORE_MIN_TOKENS tokens whose other
        positions are padding it never sees —, so both stages of an answer ranking go through the same kernels whatever the
        batch holds, and position 0 goes through the LM head in HEAD_GEMM_ROWS-row launches (``lm_logits_rows``)."""
        require_cuda(enc16, "BertLMHeadModel.start_logits")
        bert, cfg = self.bert, self.config
        dev = enc16.device
        T = SCORE_MIN_TOKENS
        if B <= 0 or enc16.shape[0] % B:
            raise ValueError(f"start_logits: {enc16.shape[0]} encoder rows do not divide into B={B} units")
        Te = enc16.shape[0] // B
        ckl = None
        if cross_kv_len is not None:
            ckl = torch.as_tensor(cross_kv_len).cpu().long().view(-1)
            if ckl.numel() != B or int(ckl.min()) < 1 or int(ckl.max()) > Te:
                raise ValueError(f"start_logits: cross_kv_len must hold {B} lengths in [1, {Te}]")
            ckl = ckl.to(torch.int32).to(dev)
        out = torch.empty((B, cfg.vocab_size), dtype=torch.float32, device=dev)
        for b0 in range(0, B, bert.MAX_IMAGES_PER_LAUNCH):
            b1 = min(B, b0 + bert.MAX_IMAGES_PER_LAUNCH)
            n = b1 - b0
            kw_p, kw_r = ({}, {}) if ckl is None else (dict(kv_len=ckl[b0:b1]), dict(cross_kv_len=ckl[b0:b1].contiguous()))
            cross = bert.project_cross_kv(enc16[b0 * Te:b1 * Te], n, Te, v_rowmajor=True, **kw_p)
            blk = torch.full((n, T), cfg.pad_token_id, dtype=torch.int32, device=dev)
            blk[:, 0] = int(start_id)
            h32, h16 = self._causal_block_pass(blk.view(-1), n, T, cross, **kw_r)
            rows = torch.arange(n, device=dev) * T
            out[b0:b1].copy_(self.lm_logits_rows(h16, rows, h32=h32))
        return out

    @torch.no_grad()
    def score(self, enc16, B, ids, lens, *, image_index=None, group_start=None, max_group=0, label_smoothing=0.1,
              prompt_length, cross_kv_len=None):
        """Teacher-forced scores of GIVEN captions (models/med.py:886-917 with labels; models/blip.py:104-125 builds them).

        enc16: image tokens of B images, 16-bit [B*Te, width] ([hi | lo | hi] rows in the parity mode).  ids int [P, T]
        right-padded caption ids ([DEC] first), lens int [P].  Caption p describes image ``image_index[p]`` (any order;
        default: image p), or — IMAGE-MAJOR caption order — image j owns captions group_start[j] .. group_start[j+1]-1
        (at most max_group each; 0: taken from the table).  The logits at position t are scored against token t + 1 for
        prompt_length - 1 <= t <= lens - 2 (``teacher_forced_targets``); a caption's loss is the sum over its targets of
        (1 - eps) * (-lp[label]) + eps * (-mean_j lp[j]), eps = label_smoothing.  Returns a ``CaptionScores``.
        ``cross_kv_len`` (int [B]): encoder unit b holds cross_kv_len[b] real states followed by padding up to Te (question
        states, models/blip_vqa.py:69-76,153-159); every caption attends to the real states of its unit only — the length is
        expanded per caption through image_index / group_start.  Not built for the parity mode.

        Schedule: one causal pass over blocks of T = max(lens) tokens (at least SCORE_MIN_TOKENS) per caption — no KV arena,
        the right padding is hidden by the causal mask —, the stack a DecoderSession runs (LN-folded / parity); cross K/V
        and the stack over at most BertModel.MAX_IMAGES_PER_LAUNCH images at a time; the LM head on the target rows only,
        in row blocks of LOGITS_BLOCK_BYTES of logits that one kernel reduces in one read (kernels.token_logprobs)."""
        require_cuda(enc16, "BertLMHeadModel.score")
        bert, cfg = self.bert, self.config
        dev = enc16.device
        V, H, L = cfg.vocab_size, cfg.num_attention_heads, cfg.num_hidden_layers
        eps_ls = float(label_smoothing)
        if not 0.0 <= eps_ls < 1.0:
            raise ValueError(f"score: label_smoothing={label_smoothing} must be in [0, 1)")
        ids_c = torch.as_tensor(ids).cpu().long()
        lens_c = torch.as_tensor(lens).cpu().long().view(-1)
        if ids_c.dim() != 2 or lens_c.numel() != ids_c.shape[0]:
            raise ValueError(f"score: ids [P, T] and lens [P] expected, got {tuple(ids_c.shape)} / {tuple(lens_c.shape)}")
        P, Tin = ids_c.shape
        if P and (int(lens_c.min()) < 0 or int(lens_c.max()) > Tin):
            raise ValueError(f"score: lens must be in [0, {Tin}]")
        if B <= 0 or enc16.shape[0] % B:
            raise ValueError(f"score: {enc16.shape[0]} image-token rows do not divide into B={B} images")
        Te = enc16.shape[0] // B
        ckl_c = None
        if cross_kv_len is not None:
            ckl_c = torch.as_tensor(cross_kv_len).cpu().long().view(-1)
            if ckl_c.numel() != B or int(ckl_c.min()) < 1 or int(ckl_c.max()) > Te:
                raise ValueError(f"score: cross_kv_len must hold {B} lengths in [1, {Te}]")
        n_img = bert.MAX_IMAGES_PER_LAUNCH
        # ---- passes: (first image, last image + 1, caption indices, their image within the block | group table, max group)
        passes = []
        if group_start is not None:
            if image_index is not None:
                raise ValueError("score: image_index and group_start are mutually exclusive")
            gs = torch.as_tensor(group_start).cpu().long().view(-1)
            if gs.numel() != B + 1 or int(gs[0]) != 0 or int(gs[-1]) != P or bool((gs[1:] < gs[:-1]).any()):
                raise ValueError(f"score: group_start must be a non-decreasing table of {B + 1} entries from 0 to {P}")
            if max_group and int((gs[1:] - gs[:-1]).max()) > max_group:
                raise ValueError(f"score: a group holds more than max_group={max_group} captions")
            for b0 in range(0, B, n_img):
                b1 = min(B, b0 + n_img)
                p0, p1 = int(gs[b0]), int(gs[b1])
                if p1 > p0:
                    g = gs[b0:b1 + 1] - p0
                    passes.append((b0, b1, torch.arange(p0, p1), None, g, int((g[1:] - g[:-1]).max())))
        else:
            if image_index is None:
                if P != B:
                    raise ValueError(f"score: {P} captions for {B} images need image_index or group_start")
                img = torch.arange(P)
            else:
                img = torch.as_tensor(image_index).cpu().long().view(-1)
            if img.numel() != P or (P and (int(img.min()) < 0 or int(img.max()) >= B)):
                raise ValueError(f"score: image_index must hold {P} entries in [0, {B})")
            for b0 in range(0, B, n_img):
                b1 = min(B, b0 + n_img)
                sel = ((img >= b0) & (img < b1)).nonzero().view(-1)
                for c0 in range(0, sel.numel(), SCORE_MAX_CAPTIONS_PER_PASS):
                    s = sel[c0:c0 + SCORE_MAX_CAPTIONS_PER_PASS]
                    passes.append((b0, b1, s, img[s] - b0, None, 0))
        labels_all = teacher_forced_targets(ids_c, lens_c, prompt_length)
        N = int((labels_all >= 0).sum())
        scores = torch.zeros((N, 2), dtype=torch.float32, device=dev)
        amax = torch.zeros((N,), dtype=torch.int32, device=dev)
        caps, poss = [], []
        block_rows = max(1, LOGITS_BLOCK_BYTES // (4 * V))
        if block_rows >= HEAD_GEMM_ROWS:
            block_rows = block_rows // HEAD_GEMM_ROWS * HEAD_GEMM_ROWS
        buf = None
        cross, cross_of = None, None
        done = 0
        for b0, b1, s, img_local, g_local, mg in passes:
            if cross_of != (b0, b1):         # (more than 32 query rows per image in every launch: row-major values)
                cross = bert.project_cross_kv(enc16[b0 * Te:b1 * Te], b1 - b0, Te, v_rowmajor=True,
                                              **({} if ckl_c is None else dict(kv_len=ckl_c[b0:b1].to(dev))))
                cross_of = (b0, b1)
            Pb = s.numel()
            ln = lens_c[s]
            T = max(SCORE_MIN_TOKENS, int(ln.max()))
            if T > cfg.max_position_embeddings:
                raise ValueError(f"score: {T} tokens exceed max_position_embeddings={cfg.max_position_embeddings}")
            t = torch.arange(T)
            blk = torch.full((Pb, T), cfg.pad_token_id, dtype=torch.long)
            w = min(T, Tin)
            blk[:, :w] = ids_c[s][:, :w]
            blk = torch.where(t[None, :] < ln[:, None], blk, torch.full_like(blk, cfg.pad_token_id))
            lab = torch.full((Pb, T), -100, dtype=torch.long)
            lab[:, :w] = labels_all[s][:, :w]
            ci, ti = (lab >= 0).nonzero(as_tuple=True)           # caption-major, positions ascending
            n = ci.numel()
            if n == 0:
                continue
            cross_kw = dict(cross_index=None if img_local is None else img_local.to(torch.int32).to(dev).contiguous(),
                            cross_groups=None if g_local is None else g_local.to(torch.int32).to(dev).contiguous(), cross_max_group=mg)
            if ckl_c is not None:            # every caption attends to the real states of its unit only
                unit = ckl_c[b0:b1]
                per = unit[img_local] if img_local is not None else unit.repeat_interleave(g_local[1:] - g_local[:-1])
                cross_kw["cross_kv_len"] = per.to(torch.int32).to(dev).contiguous()
            h32, h16 = self._causal_block_pass(blk.to(torch.int32).to(dev).view(-1), Pb, T, cross, **cross_kw)
            d_rows = (ci * T + ti).to(dev)
            d_labels = lab[ci, ti].to(torch.int32).to(dev)
            for r0 in range(0, n, block_rows):
                k = min(block_rows, n - r0)
                need = (k + HEAD_GEMM_ROWS - 1) // HEAD_GEMM_ROWS * HEAD_GEMM_ROWS
                if buf is None or buf.shape[0] < need:
                    buf = None               # (release before growing)
                    buf = torch.empty((need, V), dtype=torch.float32, device=dev)
                lg = self.lm_logits_rows(h16, d_rows[r0:r0 + k], out=buf, h32=h32)
                K.token_logprobs(lg, d_labels[r0:r0 + k], out_scores=scores[done + r0:done + r0 + k],
                                 out_index=amax[done + r0:done + r0 + k])
            done += n
            caps.append(s[ci])
            poss.append(ti + 1)
        caption = torch.cat(caps) if caps else torch.zeros((0,), dtype=torch.long)
        position = torch.cat(poss) if poss else torch.zeros((0,), dtype=torch.long)
        lp, lpm = scores[:, 0], scores[:, 1]
        # (a handful of floats per caption from here on: the 30,524-wide rows never reach a torch op)
        token_loss = -lp if eps_ls == 0.0 else -((1.0 - eps_ls) * lp + eps_ls * lpm)
        caption_d, position_d = caption.to(dev), position.to(dev)
        table = torch.zeros((P, max(1, Tin)), dtype=torch.float64, device=dev)
        table[caption_d, position_d] = token_loss.double()
        count = torch.bincount(caption, minlength=P).to(torch.int32).to(dev)
        return CaptionScores(loss_sum=table.sum(1).float(), count=count, lp_label=lp, lp_mean=lpm, argmax=amax,
                             token_loss=token_loss, caption=caption_d, position=position_d)

    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, head_mask=None, inputs_embeds=None,
                encoder_hidden_states=None, encoder_attention_mask=None, labels=None, past_key_values=None, use_cache=None,
                output_attentions=None, output_hidden_states=None, return_dict=None, return_logits=False, is_decoder=True,
                reduction='mean', mode='multimodal'):
        """The reference's call (models/med.py:830-930) over the library's kernels: ``BertModel.forward`` (same served and
        refused arguments, same mask contract) and the LM head on every position.

        ``logits`` f32 [B, T, V]: the LM-head GEMMs over all rows (``lm_logits_rows``, in row blocks of LOGITS_BLOCK_BYTES of
        scratch).  return_logits=True returns [B, T-1, V] and nothing else (:905-906).  With ``labels`` int [B, T] (-100:
        ignored): ``loss``, the label-smoothed (0.1) cross-entropy of the logits at t against labels[t + 1], from the one-read
        reduction of kernels.token_logprobs — reduction='mean': 0-dim, over the scored tokens; 'none': [B], the sum per sequence
        (:909-917).  On right-padded captions these sums are the bits of ``score`` (loss_sum) on the same inputs (same kernels;
        the self-attention launch also carries ``kv_len``, see ``BertModel.forward``).  The logits
        of a position whose mask is 0 are outside the mask contract, so a label at t + 1 behind such a position (the first real
        token of a left-padded sequence) belongs at -100, as a prompt's tokens are (models/blip.py:114).
        Returns an object with ``loss``, ``logits``, ``hidden_states``; with return_dict=False the tuple ([loss,] logits[,
        hidden_states]).  No backward pass: the results carry no graph."""
        if reduction not in ("mean", "none"):
            raise ValueError(f"BertLMHeadModel.forward: reduction={reduction!r} (mean | none)")
        refused = (("position_ids", position_ids), ("head_mask", head_mask), ("inputs_embeds", inputs_embeds),
                   ("past_key_values", past_key_values), ("use_cache", use_cache), ("output_attentions", output_attentions))
        h32, h16, Tp, _, hidden = self.bert._forward_states("BertLMHeadModel.forward", input_ids, attention_mask,
                                                            encoder_hidden_states, encoder_attention_mask,
                                                            bool(output_hidden_states), is_decoder, mode, refused)
        cfg = self.config
        B, T = input_ids.shape
        V = cfg.vocab_size
        dev = h32.device
        if labels is not None and tuple(labels.shape) != (B, T):
            raise ValueError(f"BertLMHeadModel.forward: labels must be [{B}, {T}], got {tuple(labels.shape)}")
        rows = (torch.arange(B, device=dev)[:, None] * Tp + torch.arange(T, device=dev)[None, :]).reshape(-1)
        n = B * T
        block = max(1, LOGITS_BLOCK_BYTES // (4 * V))
        if block >= HEAD_GEMM_ROWS:
            block = block // HEAD_GEMM_ROWS * HEAD_GEMM_ROWS
        n_pad = (n + HEAD_GEMM_ROWS - 1) // HEAD_GEMM_ROWS * HEAD_GEMM_ROWS
        if n_pad <= block:                  # (one block: the head writes the result's own storage)
            store = torch.empty((n_pad, V), dtype=torch.float32, device=dev)
            logits = self.lm_logits_rows(h16, rows, out=store, h32=h32)
        else:
            logits = torch.empty((n, V), dtype=torch.float32, device=dev)
            # (the scratch of a block: its rows rounded up to whole HEAD_GEMM_ROWS-row launches, as score sizes its buffer)
            need = (min(block, n) + HEAD_GEMM_ROWS - 1) // HEAD_GEMM_ROWS * HEAD_GEMM_ROWS
            buf = torch.empty((need, V), dtype=torch.float32, device=dev)
            for r0 in range(0, n, block):
                logits[r0:r0 + block].copy_(self.lm_logits_rows(h16, rows[r0:r0 + block], out=buf, h32=h32))
        if return_logits:
            return logits.view(B, T, V)[:, :-1].contiguous()
        loss = None
        if labels is not None:
            shifted = torch.full((B, T), -100, dtype=torch.int32, device=dev)
            shifted[:, :-1] = labels.to(dev)[:, 1:].to(torch.int32)
            shifted = torch.where(shifted < 0, torch.full_like(shifted, -100), shifted).view(-1).contiguous()
            lp, lpm, _ = K.token_logprobs(logits, shifted)
            token_loss = -((1.0 - 0.1) * lp + 0.1 * lpm)                # (ignored rows score exactly 0 in both)
            if reduction == "none":
                table = torch.zeros((B, T), dtype=torch.float64, device=dev)
                table[:, 1:] = token_loss.view(B, T)[:, :-1].double()   # (at the TARGET token's position, as score does)
                loss = table.sum(1).float()
            else:
                loss = (token_loss.double().sum() / ((shifted >= 0) & (shifted < V)).sum().clamp_min(1)).float()
        logits = logits.view(B, T, V)
        if return_dict is not None and not return_dict:
            return (() if loss is None else (loss,)) + (logits,) + (() if hidden is None else (hidden,))
        return ModelOutput(loss=loss, logits=logits, past_key_values=None, hidden_states=hidden, attentions=None,
                           cross_attentions=None)
