"""Shared inputs of the sentence-encoder tests and the reference value: a restatement of MPNet (HF ``MPNetModel``: embeddings,
the shared T5-bucketed relative-position bias, 12 post-LN layers) with sentence-transformers' masked mean pooling and L2
normalisation, in the dtype the caller names (float64: the reference; float32: its own rounding error, which sizes the bounds).
tests/test_sentence_cpu.py pins the restatement to the installed ``transformers`` implementation."""
import math

import numpy as np
import torch
import torch.nn.functional as F

BOS, PAD, EOS, UNK = 0, 1, 2, 3
SMALL = dict(vocab_size=200, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
             max_position_embeddings=514)
FULL = dict(vocab_size=30527, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
            max_position_embeddings=514)
EPS = 1e-5
# token counts, specials included: both sides of every 32-token tile edge and of offset 91 (where the buckets saturate)
SUPPORT_LENS = [3, 4, 5, 7, 9, 12, 17, 24, 33, 34, 40, 64, 65, 90, 93, 94, 97, 120, 128, 129, 150, 160, 161, 200, 3, 6, 8, 10, 11,
                13, 14, 15, 16, 18, 20, 22, 26, 28, 30, 31, 32, 35, 36, 48, 50, 60, 70, 80]
QUERY_LENS = [3, 5, 8, 13, 21, 34, 55, 89, 95, 130, 144, 200, 4, 6, 10, 12]
FULL_LENS = [384, 130, 3]


def make_state(cfg=SMALL, seed=1):
    """HF ``MPNetModel`` parameter names -> f32 tensors from numpy's PCG64 stream (the same on every host): matrices N(0, 0.05),
    biases N(0, 0.1), LayerNorm gains N(1, 0.1), the relative-position table N(0, 1) — asymmetric in sign and large enough to
    matter."""
    rng = np.random.default_rng(seed)
    C, I, H = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_attention_heads"]

    def n(shape, mean, std):
        return torch.from_numpy((mean + std * rng.standard_normal(shape)).astype(np.float32))

    sd = {"embeddings.word_embeddings.weight": n((cfg["vocab_size"], C), 0, 0.05),
          "embeddings.position_embeddings.weight": n((cfg["max_position_embeddings"], C), 0, 0.05),
          "embeddings.LayerNorm.weight": n((C,), 1, 0.1), "embeddings.LayerNorm.bias": n((C,), 0, 0.1),
          "encoder.relative_attention_bias.weight": n((32, H), 0, 1.0)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        for x in "qkvo":
            sd[p + f"attention.attn.{x}.weight"] = n((C, C), 0, 0.05)
            sd[p + f"attention.attn.{x}.bias"] = n((C,), 0, 0.1)
        sd[p + "attention.LayerNorm.weight"], sd[p + "attention.LayerNorm.bias"] = n((C,), 1, 0.1), n((C,), 0, 0.1)
        sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"] = n((I, C), 0, 0.05), n((I,), 0, 0.1)
        sd[p + "output.dense.weight"], sd[p + "output.dense.bias"] = n((C, I), 0, 0.05), n((C,), 0, 0.1)
        sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"] = n((C,), 1, 0.1), n((C,), 0, 0.1)
    return sd


def sentences(lens, seed, vocab=200):
    """Random id lists ``<s> ... </s>`` of the given token counts (ids 4 .. vocab-1 inside)."""
    rng = np.random.default_rng(seed)
    return [[BOS] + [int(v) for v in rng.integers(4, vocab, size=L - 2)] + [EOS] for L in lens]


def words(ids):
    """The string the synthetic tokenizer turns back into ``ids`` (its inner ids as ``w<id>`` words)."""
    return " ".join(f"w{i}" for i in ids[1:-1])


def bucket(query, key):
    """MPNet's bucket of one (query, key) pair, 32 buckets: n = |key - query| maps to n when n < 8, else to
    min(15, 8 + int(log(n / 8) / log(16) * 8)); 16 more when key > query."""
    n = abs(key - query)
    b = n if n < 8 else min(15, 8 + int(math.log(n / 8) / math.log(16) * 8))
    return b + (16 if key > query else 0)


def position_bias(sd, T, dtype=torch.float64):
    """[H, T, T]: bias[h, i, j] = relative_attention_bias[bucket(i, j), h]."""
    by_offset = {d: bucket(0, d) for d in range(-(T - 1), T)}
    idx = torch.tensor([[by_offset[j - i] for j in range(T)] for i in range(T)], dtype=torch.long)
    return sd["encoder.relative_attention_bias.weight"].to(dtype)[idx].permute(2, 0, 1)


def hidden_states(sd, cfg, ids, mask, dtype=torch.float64, layers=None):
    """ids long [B, T] right-padded with PAD, mask [B, T] (1: a token) -> [B, T, C] after the last layer; ``layers`` (a list)
    receives the states after the embeddings and after every layer."""
    g = lambda k: sd[k].to(dtype)
    B, T = ids.shape
    H, C = cfg["num_attention_heads"], cfg["hidden_size"]
    pos = torch.cumsum(mask, 1) * mask + PAD
    h = g("embeddings.word_embeddings.weight")[ids] + g("embeddings.position_embeddings.weight")[pos]
    h = F.layer_norm(h, (C,), g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"), EPS)
    bias = position_bias(sd, T, dtype)
    neg = torch.zeros(B, 1, 1, T, dtype=dtype).masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    if layers is not None:
        layers.append(h)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{i}."
        lin = lambda x, name: x @ g(p + name + ".weight").t() + g(p + name + ".bias")
        heads = lambda x: x.view(B, T, H, C // H).transpose(1, 2)
        q, k, v = (heads(lin(h, "attention.attn." + x)) for x in "qkv")
        s = q @ k.transpose(-1, -2) / math.sqrt(C // H) + bias[None] + neg
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, C)
        h = F.layer_norm(lin(a, "attention.attn.o") + h, (C,), g(p + "attention.LayerNorm.weight"), g(p + "attention.LayerNorm.bias"), EPS)
        f = lin(F.gelu(lin(h, "intermediate.dense")), "output.dense")
        h = F.layer_norm(f + h, (C,), g(p + "output.LayerNorm.weight"), g(p + "output.LayerNorm.bias"), EPS)
        if layers is not None:
            layers.append(h)
    return h


def pad(id_lists, T=None):
    T = T or max(len(x) for x in id_lists)
    ids = torch.full((len(id_lists), T), PAD, dtype=torch.long)
    mask = torch.zeros((len(id_lists), T), dtype=torch.long)
    for r, x in enumerate(id_lists):
        ids[r, :len(x)] = torch.tensor(x)
        mask[r, :len(x)] = 1
    return ids, mask


def pool(h, mask, normalize=True):
    """sentence-transformers' mean pooling over the mask, then (optionally) L2 normalisation."""
    m = mask.to(h.dtype)[:, :, None]
    e = (h * m).sum(1) / m.sum(1).clamp(min=1e-9)
    return F.normalize(e, p=2, dim=1) if normalize else e


def embed(sd, cfg, id_lists, dtype=torch.float64, normalize=True):
    """[n, C] embeddings, every sentence run alone and unpadded (in exact arithmetic padding changes nothing: masked keys weigh 0)."""
    with torch.no_grad():
        return torch.cat([pool(hidden_states(sd, cfg, *pad([x]), dtype=dtype), torch.ones(1, len(x), dtype=torch.long), normalize)
                          for x in id_lists])


def ranking(q, s, n):
    """Indices of the ``n`` largest cosines of every row of q against the rows of s, VALUE DESCENDING, INDEX ASCENDING."""
    cos = (q @ s.t()).numpy()
    return [sorted(range(cos.shape[1]), key=lambda j: (-row[j], j))[:n] for row in cos], cos


_cache = {}


def small():
    """(state dict, support id lists, query id lists, float64 support embeddings, float64 query embeddings), computed once."""
    if "small" not in _cache:
        # (seed 1 of 12 tried: the one whose float64 top-1 / top-2 and 5th / 6th cosine gaps are widest, 5.2e-4 and 6.9e-4 — a
        #  property of the reference alone; tests/test_sentence_cpu.py asserts that the gaps suffice)
        sd = make_state(SMALL, 1)
        sup, qry = sentences(SUPPORT_LENS, 11), sentences(QUERY_LENS, 12)
        _cache["small"] = (sd, sup, qry, embed(sd, SMALL, sup), embed(sd, SMALL, qry))
    return _cache["small"]


def load_into(model, sd):
    """The state dict into a vidil_amd.sentence.SentenceEncoder (same names)."""
    model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return model


def stub_vector(text, dim=16):
    """A fixed vector per string (from its SHA-256): what the stub encoders of the consumer tests and of
    tests/golden/make_in_context_golden.py return.  Distinct strings give distinct cosines (no ties)."""
    import hashlib

    raw = hashlib.sha256(text.encode("utf-8")).digest()[:dim]
    return torch.tensor([(b - 127.5) / 127.5 for b in raw], dtype=torch.float32)


class StubEncoder:
    """``encode`` of a SentenceEncoder / SentenceTransformer for the consumer tests: ``stub_vector`` per sentence (or a vector the
    caller fixed for that sentence); ``calls`` records what was embedded."""

    def __init__(self, fixed=None):
        self.fixed, self.calls = dict(fixed or {}), []

    def eval(self):
        return self

    def to(self, device):
        return self

    def encode(self, sentences, batch_size=32, convert_to_tensor=True, normalize_embeddings=True):
        sentences = [sentences] if isinstance(sentences, str) else list(sentences)
        self.calls.append(sentences)
        return torch.stack([torch.as_tensor(self.fixed[s], dtype=torch.float32) if s in self.fixed else stub_vector(s) for s in sentences])


def host_closest(queries, candidates, top_n=1):
    """vidil_amd.sentence.closest's contract on the host, for tests without a GPU: float64 cosines, VALUE DESCENDING, INDEX
    ASCENDING.  (The GPU tests run the real one, on vidil_scan_scores + vidil_topk_rows.)"""
    q = F.normalize(torch.as_tensor(queries).double().reshape(-1, torch.as_tensor(queries).shape[-1]), dim=1)
    c = F.normalize(torch.as_tensor(candidates).double(), dim=1)
    idx, cos = ranking(q, c, min(int(top_n), c.shape[0]))
    vals = torch.tensor([[cos[r][j] for j in row] for r, row in enumerate(idx)], dtype=torch.float32)
    return vals, torch.tensor(idx, dtype=torch.int32)
