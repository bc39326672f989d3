"""Sentence encoder on the HIP kernels: MPNet-base with masked mean pooling and L2 normalisation — what the reference loads as
``SentenceTransformer('all-mpnet-base-v2')`` to map generated answers onto an answer list (eval_video_qa_result.py:156-215), to
choose the few-shot examples of a prompt (generate_prompts_random_prefix_in_context_selection.py:131-287) and to pick the closest
candidate (eval_vlep.py:90-108).

Every consumer takes an argmax or a top-N over cosines, so the encoder runs on the parity arithmetic whatever the process-wide
precision mode is: error-compensated ``[hi | lo | hi]`` f16 operands in every GEMM (``split_k``), and ``vidil_attention_f32``
in its split-operand form with MPNet's relative-position bias (``arith = 2``): ``bias[h][key - query]``, T5-bucketed with 32
buckets, one table for all layers.  The bias is Toeplitz, so a per-head table of 2 T - 1 floats carries all of it; it is built on
the host once per pack.  Operands are f16 whatever $VIDIL_DTYPE says (bf16 hi + lo carries 16 bits, fp8 does not apply).

The module tree and the parameter names are HF ``MPNetModel``'s, so a sentence-transformers directory loads directly.
World size 1; no throughput (plain 16-bit) mode."""
from __future__ import annotations

import json
import math
import os

import torch
from torch import nn

from . import kernels as K
from .med import parity_layers
from .packing import PackedCache, require_cuda, set_parity_attention, v32, w3
from .tokenizer import init_sentence_tokenizer

#: tokens of a batch are padded to a multiple of this (the key tile of the attention kernel)
PAD_MULTIPLE = 32


class SentenceConfig:
    """all-mpnet-base-v2's configuration (HF ``MPNetConfig`` names)."""

    def __init__(self, **kw):
        self.vocab_size = 30527
        self.hidden_size = 768
        self.num_hidden_layers = 12
        self.num_attention_heads = 12
        self.intermediate_size = 3072
        self.max_position_embeddings = 514
        self.pad_token_id = 1
        self.layer_norm_eps = 1e-5
        self.relative_attention_num_buckets = 32
        self.max_seq_length = 384
        self.initializer_range = 0.02
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(f"SentenceConfig: unknown field {k!r}")
            setattr(self, k, v)
        if self.hidden_size != 64 * self.num_attention_heads:
            raise ValueError("SentenceConfig: heads of 64 only (hidden_size = 64 * num_attention_heads)")
        if self.max_seq_length + self.pad_token_id + 1 > self.max_position_embeddings:
            raise ValueError("SentenceConfig: max_seq_length exceeds the position table (position id = index + pad_token_id + 1)")


def relative_position_buckets(T, num_buckets=32, max_distance=128):
    """Bucket of every offset ``key - query`` in -(T-1) .. T-1 (int64 [2T-1], index T-1 is offset 0): T5's bidirectional buckets
    as MPNet uses them.  With n = |key - query|: n when n < 8, else min(15, 8 + int(log(n / 8) / log(16) * 8)); 16 more when
    key > query.  The logarithm is taken in float32, as the model the checkpoints were trained with takes it."""
    half = num_buckets // 2
    exact = half // 2
    rel = torch.arange(-(T - 1), T, dtype=torch.long)
    n = rel.abs()
    large = exact + (torch.log(n.float() / exact) / math.log(max_distance / exact) * (half - exact)).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, half - 1))
    return (rel > 0).long() * half + torch.where(n < exact, n, large)


def relative_bias_table(weight, T):
    """``relative_attention_bias.weight`` [buckets, H] -> (f32 [H, 2T-1], rel_off = T-1): table[h][rel_off + key - query] is the
    bias of head h — vidil_attention_f32's ``rel_bias`` / ``rel_off``."""
    b = relative_position_buckets(T, weight.shape[0]).to(weight.device)
    return weight.detach().float()[b].t().contiguous(), T - 1


class _Attn(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.q, self.k, self.v, self.o = (nn.Linear(C, C) for _ in range(4))


class _Attention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attn = _Attn(cfg.hidden_size)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class _Dense(nn.Module):
    def __init__(self, d_in, d_out, eps=None):
        super().__init__()
        self.dense = nn.Linear(d_in, d_out)
        if eps is not None:
            self.LayerNorm = nn.LayerNorm(d_out, eps=eps)


class _Layer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attention = _Attention(cfg)
        self.intermediate = _Dense(cfg.hidden_size, cfg.intermediate_size)
        self.output = _Dense(cfg.intermediate_size, cfg.hidden_size, cfg.layer_norm_eps)


class _Encoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList(_Layer(cfg) for _ in range(cfg.num_hidden_layers))
        self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_attention_heads)


class _Embeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = nn.Embedding(cfg.vocab_size, cfg.hidden_size, padding_idx=cfg.pad_token_id)
        self.position_embeddings = nn.Embedding(cfg.max_position_embeddings, cfg.hidden_size, padding_idx=cfg.pad_token_id)
        self.LayerNorm = nn.LayerNorm(cfg.hidden_size, eps=cfg.layer_norm_eps)


class SentenceEncoder(PackedCache, nn.Module):
    """MPNet + masked mean + L2 normalisation; ``encode`` is named as in sentence-transformers."""

    def __init__(self, config=None, tokenizer=None):
        super().__init__()
        self.config = config or SentenceConfig()
        self.embeddings = _Embeddings(self.config)
        self.encoder = _Encoder(self.config)
        std = self.config.initializer_range
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                m.weight.data.normal_(0.0, std)
            if isinstance(m, nn.Linear):
                m.bias.data.zero_()
        self.tokenizer = tokenizer
        set_parity_attention("split", self)       # (the layer sequence asks its owner which attention the parity mode runs)

    # ------------------------------------------------------------------ packing (always compensated f16 operands)
    def pack_flags(self):
        return ("sentence",)

    def _pack(self):
        cfg, e, c = self.config, self.embeddings, torch.float16
        p = dict(word=v32(e.word_embeddings.weight).view(cfg.vocab_size, -1),
                 pos=v32(e.position_embeddings.weight).view(cfg.max_position_embeddings, -1),
                 emb_g=v32(e.LayerNorm.weight), emb_b=v32(e.LayerNorm.bias), layers=[], parity=True)
        for l in self.encoder.layer:
            a = l.attention.attn
            p["layers"].append(dict(
                qkv_w3=w3(a.q.weight, a.k.weight, a.v.weight, dtype=c), qkv_b=v32(a.q.bias, a.k.bias, a.v.bias),
                ao_w3=w3(a.o.weight, dtype=c), ao_b=v32(a.o.bias),
                ao_g=v32(l.attention.LayerNorm.weight), ao_bt=v32(l.attention.LayerNorm.bias),
                i_w3=w3(l.intermediate.dense.weight, dtype=c), i_b=v32(l.intermediate.dense.bias),
                o_w3=w3(l.output.dense.weight, dtype=c), o_b=v32(l.output.dense.bias),
                o_g=v32(l.output.LayerNorm.weight), o_bt=v32(l.output.LayerNorm.bias)))
        p["rel_bias"], p["rel_off"] = relative_bias_table(self.encoder.relative_attention_bias.weight, cfg.max_seq_length)
        return p

    # ------------------------------------------------------------------ the model
    @torch.no_grad()
    def hidden_states(self, ids_i32, lens_i32):
        """ids int32 [B, T] right-padded with ``pad_token_id``, lens int32 [B] -> f32 [B*T, C] after the last layer (rows of padding
        tokens hold values nobody reads)."""
        require_cuda(ids_i32, "SentenceEncoder.hidden_states")
        cfg = self.config
        B, T = ids_i32.shape
        if T > cfg.max_seq_length:
            raise K.VidilHipError(f"SentenceEncoder: {T} tokens exceed max_seq_length = {cfg.max_seq_length}")
        p = self.packed()
        C, dev = cfg.hidden_size, ids_i32.device
        raw = torch.empty((B * T, C), dtype=torch.float32, device=dev)
        # position id = index + padding_idx + 1 for real tokens (right padding: a real token's index is its column)
        K.embed_tokens(ids_i32.reshape(-1), p["word"], p["pos"], raw, T=T, pos_off=cfg.pad_token_id + 1)
        h32 = torch.empty((B * T, C), dtype=torch.float32, device=dev)
        h3 = torch.empty((B * T, 3 * C), dtype=torch.float16, device=dev)
        K.layernorm(raw, p["emb_g"], p["emb_b"], cfg.layer_norm_eps, out16=h3, out32=h32, split3=True)
        # the parity layer sequence of the MED text stack without cross-attention — Q|K|V -> attention_f32 -> output GEMM +
        # residual -> LN -> fc1 + GELU -> fc2 + residual -> LN —, its self-attention with this model's bias table
        parity_layers(self, p, h32, h3, rows=B, T=T, causal=False, kv_len=lens_i32, rel_bias=p["rel_bias"], rel_off=p["rel_off"])
        return h32

    @torch.no_grad()
    def embed_ids(self, ids_i32, lens_i32, normalize=True):
        """-> f32 [B, C]: the mean of every sentence's ``lens`` token states, L2-normalised.  The mean is one query row of zeros
        through the split-operand attention (a uniform softmax over the first ``lens`` keys = the masked mean of V, per 64-column
        head): one wave per (sentence, head) walks that sentence's keys alone, so the result does not depend on the batch."""
        cfg = self.config
        B, T = ids_i32.shape
        h32 = self.hidden_states(ids_i32, lens_i32)
        zero = torch.zeros((B, cfg.hidden_size), dtype=torch.float32, device=h32.device)
        out = torch.empty_like(zero)
        K.attention_f32(zero, h32, h32, out, Bq=B, H=cfg.num_attention_heads, Nq=1, Nk=T, kv_len=lens_i32, arith=1)
        return K.l2_normalize_rows(out) if normalize else out

    def tokenize(self, sentences):
        """-> list of id lists, ``<s> ... </s>``, truncated to ``max_seq_length`` keeping ``</s>``."""
        if self.tokenizer is None:
            raise RuntimeError("SentenceEncoder: no tokenizer (sentence_encoder() builds one; or pass tokenizer=)")
        sentences = list(sentences)
        if not sentences:
            return []
        ids = self.tokenizer(sentences, truncation=True, max_length=self.config.max_seq_length)["input_ids"]
        return [list(x) for x in ids]

    @torch.no_grad()
    def encode(self, sentences, batch_size=32, convert_to_tensor=True, normalize_embeddings=True):
        """sentence-transformers' ``encode``: list[str] (or one str) -> f32 [n, C] on the model's device, in input order (numpy
        with ``convert_to_tensor=False``).  Sentences are sorted by length and run ``batch_size`` at a time, every batch padded to
        a multiple of 32 tokens; at equal padded length a sentence's embedding has the same bits whatever else is in its batch."""
        single = isinstance(sentences, str)
        ids = self.tokenize([sentences] if single else sentences)
        out = self.encode_ids(ids, batch_size=batch_size, normalize_embeddings=normalize_embeddings)
        if single:
            out = out[0]
        return out if convert_to_tensor else out.cpu().numpy()

    @torch.no_grad()
    def encode_ids(self, ids, batch_size=32, normalize_embeddings=True):
        """``encode`` from token ids (lists that already carry ``<s>`` and ``</s>``)."""
        cfg = self.config
        dev = next(self.parameters()).device
        n = len(ids)
        out = torch.empty((n, cfg.hidden_size), dtype=torch.float32, device=dev)
        order = sorted(range(n), key=lambda i: (-len(ids[i]), i))                 # longest first, as sentence-transformers
        for b0 in range(0, n, batch_size):
            idx = order[b0:b0 + batch_size]
            T = (max(len(ids[i]) for i in idx) + PAD_MULTIPLE - 1) // PAD_MULTIPLE * PAD_MULTIPLE
            T = min(T, cfg.max_seq_length)
            for i in idx:
                if not 0 < len(ids[i]) <= T:
                    raise ValueError(f"encode_ids: sentence {i} has {len(ids[i])} tokens (1 .. {cfg.max_seq_length})")
            rows = torch.tensor([list(ids[i]) + [cfg.pad_token_id] * (T - len(ids[i])) for i in idx], dtype=torch.int32)
            lens = torch.tensor([len(ids[i]) for i in idx], dtype=torch.int32)
            out[torch.tensor(idx, device=dev)] = self.embed_ids(rows.to(dev), lens.to(dev), normalize=normalize_embeddings)
        return out

    def forward(self, *a, **k):
        raise RuntimeError("SentenceEncoder runs through encode / encode_ids (HIP kernels), not forward")

    # ------------------------------------------------------------------ weights
    def load_pretrained(self, path):
        """A sentence-transformers / HF directory (``model.safetensors`` when ``safetensors`` imports, else ``pytorch_model.bin``) or one
        such file.  A leading ``mpnet.`` / ``0.auto_model.`` is stripped, ``pooler.*`` and ``embeddings.position_ids`` are ignored; any
        other missing or unexpected key raises."""
        sd = _read_state_dict(path)
        clean = {}
        for k, v in sd.items():
            for prefix in ("0.auto_model.", "mpnet."):
                if k.startswith(prefix):
                    k = k[len(prefix):]
            if k.startswith("pooler.") or k == "embeddings.position_ids":
                continue
            clean[k] = v
        own = self.state_dict()
        missing = sorted(set(own) - set(clean))
        unexpected = sorted(set(clean) - set(own))
        if missing or unexpected:
            raise RuntimeError(f"SentenceEncoder.load_pretrained({path!r}): missing keys {missing[:8]} (+{max(0, len(missing) - 8)}), "
                               f"unexpected keys {unexpected[:8]} (+{max(0, len(unexpected) - 8)})")
        self.load_state_dict(clean, strict=True)
        return self


def _read_state_dict(path):
    if os.path.isdir(path):
        st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        try:
            import safetensors.torch as sft
        except ImportError:
            sft = None
        if sft is not None and os.path.isfile(st):
            return sft.load_file(st)
        if os.path.isfile(pt):
            return torch.load(pt, map_location="cpu", weights_only=True)
        raise FileNotFoundError(f"sentence encoder: neither pytorch_model.bin nor a readable model.safetensors in {path!r}")
    if path.endswith(".safetensors"):
        import safetensors.torch as sft

        return sft.load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def sentence_encoder(pretrained="", tokenizer=None, vocab_file=None, **kw):
    """``SentenceEncoder`` with all-mpnet-base-v2's configuration (``kw`` overrides fields of ``SentenceConfig``).  ``pretrained``: a
    sentence-transformers / HF model directory (its ``config.json`` supplies ``layer_norm_eps``; its ``vocab.txt`` is the
    vocabulary unless ``vocab_file`` / ``tokenizer`` says otherwise) or a weight file.  The stand-in tokenizer is refused together
    with ``pretrained``: real weights on pseudo-word ids embed garbage without any error."""
    if pretrained and getattr(tokenizer, "is_synthetic", False) and not getattr(tokenizer, "allow_pretrained", False):
        raise RuntimeError("a pretrained sentence encoder needs the real MPNet tokenizer, not SyntheticSentenceTokenizer "
                           "(pass vocab_file= / set $VIDIL_MPNET_VOCAB)")
    if pretrained and os.path.isdir(pretrained):
        cj = os.path.join(pretrained, "config.json")
        if os.path.isfile(cj) and "layer_norm_eps" not in kw:
            with open(cj) as f:
                kw["layer_norm_eps"] = float(json.load(f).get("layer_norm_eps", 1e-5))
        if vocab_file is None and tokenizer is None and os.path.isfile(os.path.join(pretrained, "vocab.txt")):
            vocab_file = os.path.join(pretrained, "vocab.txt")
    if tokenizer is None:
        tokenizer = init_sentence_tokenizer(vocab_file)
    model = SentenceEncoder(SentenceConfig(**kw), tokenizer=tokenizer)
    if pretrained:
        model.load_pretrained(pretrained)
    return model.eval()


# ---------------------------------------------------------------------------------------------- cosines and selection
def _rows(x, what):
    x = torch.as_tensor(x)
    if x.dim() == 1:
        x = x[None]
    require_cuda(x, what)
    return x.float().contiguous()


def cos_sim(a, b):
    """sentence-transformers' ``util.cos_sim``: f32 [len(a), len(b)] cosines of the rows of ``a`` and ``b`` (normalised here, so
    un-normalised embeddings are served too), on vidil_scan_scores: an exact k-ordered f32 chain per pair, so a cosine does not
    depend on what else is scored in the call."""
    a, b = _rows(a, "cos_sim.a").clone(), _rows(b, "cos_sim.b").clone()
    return K.scan_scores(K.l2_normalize_rows(a), K.l2_normalize_rows(b))


def closest(queries, candidates, top_n=1):
    """For every query row the ``top_n`` candidates of largest cosine (all of them when there are fewer): (cosines f32 [Q, n],
    indices i32 [Q, n]) ordered by VALUE DESCENDING, INDEX ASCENDING — the order vidil_topk_rows defines.  numpy's ``argmax`` /
    ``argsort`` of the reference leave the order among equal cosines unspecified; this one is fixed."""
    s = cos_sim(queries, candidates)
    return K.topk_rows(s, min(int(top_n), s.shape[1]))
