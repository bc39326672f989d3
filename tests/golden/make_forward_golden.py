"""Generate tests/golden/forward_small.npz and the name lists of the reference-signature forwards from the REFERENCE's own
models/med.py (through oracle/ref_shim.py).

Run in the build container only (needs the reference tree and `transformers`):

    python tests/golden/make_forward_golden.py           # forward_small.npz
    python tests/golden/make_forward_golden.py names     # forward_signatures.json, blip_base_keys.json, blip_embedding_keys.json

Small geometry of the existing goldens (hidden 256, 4 heads, 2 layers, vocabulary 512) with the weights ALREADY committed: the
text encoder of med_itm_small.npz and the decoder of med_decoder_small.npz.  The file written here holds inputs and the
reference's fp32 outputs only: B = 4 sequences of T = 12 tokens over Te = 26 encoder states (f16-representable values, stored
as f16), under every mask form of BertModel.forward / BertLMHeadModel.forward, and the three modes of BLIP_Base on the
committed small ViT's tokens (vit_small.npz `y`) for three captions of unequal length, each run alone at its own length —
the reference's BLIP_Base tokenises without padding (models/blip.py:48).

Where a mask is not a prefix of ones only the positions with mask 1 are specified (the library's contract), and only those
are stored: the other rows are written as zeros.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from common import load_golden  # noqa: E402
from oracle import ref_shim  # noqa: E402

SEED = 5
PAD, CLS, SEP, DEC, ENC = 0, 101, 102, 510, 509
B, T, TE = 4, 12, 26
LENS = [12, 7, 3, 1]
ENC_LENS = [26, 20, 5, 26]
BASE_LENS = [12, 5, 9]


def prefix(lens, n):
    return (np.arange(n)[None, :] < np.asarray(lens)[:, None]).astype(np.int64)


def inputs():
    rng = np.random.default_rng(SEED)
    words = rng.integers(110, 500, size=(B, T))
    right = prefix(LENS, T)
    left = right[:, ::-1].copy()
    holes = (rng.random((B, T)) < 0.6).astype(np.int64)
    holes[:, 0] = [1, 0, 1, 0]
    holes[np.arange(B), [3, 5, 11, 7]] = 1                  # (no row without a one)
    masks = dict(ones=np.ones((B, T), dtype=np.int64), right=right, left=left, holes=holes)
    ids = {}
    for name, m in masks.items():
        x = words.copy()
        if name in ("right", "left"):                       # the first real token is [CLS], the last [SEP], the padding [PAD]
            x = np.where(m == 1, x, PAD)
            for b, n in enumerate(LENS):
                first = 0 if name == "right" else T - n
                x[b, first + n - 1] = SEP
                x[b, first] = CLS
        else:
            x[:, 0] = CLS
        ids[name] = x
    enc = rng.standard_normal((B, TE, 256)).astype(np.float16)
    enc_holes = (rng.random((B, TE)) < 0.5).astype(np.int64)
    enc_holes[:, 3] = 1
    base_ids = np.zeros((len(BASE_LENS), max(BASE_LENS)), dtype=np.int64)
    for b, n in enumerate(BASE_LENS):
        base_ids[b, :n] = rng.integers(110, 500, size=n)
        base_ids[b, 0], base_ids[b, n - 1] = CLS, SEP
    return masks, ids, enc, dict(prefix=prefix(ENC_LENS, TE), holes=enc_holes), base_ids


def models():
    _, med = ref_shim.load()
    sd_e, _ = load_golden("med_itm_small.npz")
    sd_d, _ = load_golden("med_decoder_small.npz")
    cfg = ref_shim.med_config(encoder_width=256)
    cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size = 256, 4, 512
    cfg.num_hidden_layers, cfg.vocab_size, cfg.max_position_embeddings = 2, 512, 64
    text_encoder = med.BertModel(cfg, add_pooling_layer=False).eval()
    text_decoder = med.BertLMHeadModel(cfg).eval()
    for m, sd, p in ((text_encoder, sd_e, "text_encoder."), (text_decoder, sd_d, "text_decoder.")):
        msg = m.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)}, strict=False)
        assert all("position_ids" in k for k in msg.missing_keys) and not msg.unexpected_keys, msg
    return text_encoder, text_decoder


def kept(x, mask, is_prefix):
    """The rows the contract specifies: all of them under a prefix mask, else those with mask 1 (zeros elsewhere)."""
    x = x.numpy()
    return x if is_prefix else x * mask[..., None].astype(x.dtype)


def main():
    text_encoder, text_decoder = models()
    masks, ids, enc_np, enc_masks, base_ids = inputs()
    enc = torch.from_numpy(enc_np).float()
    out = dict(enc=enc_np, base_ids=base_ids, base_lens=np.asarray(BASE_LENS))
    for name in masks:
        out[f"mask_{name}"], out[f"ids_{name}"] = masks[name], ids[name]
    for name in enc_masks:
        out[f"encmask_{name}"] = enc_masks[name]
    t = torch.from_numpy
    with torch.no_grad():
        # ---- encoder, both modes, every self-attention mask (encoder_attention_mask: default ones)
        for name, m in masks.items():
            pre = name in ("ones", "right")
            o = text_encoder(t(ids[name]), attention_mask=t(m), return_dict=True, mode="text")
            out[f"text_{name}"] = kept(o.last_hidden_state, m, pre)
            o = text_encoder(t(ids[name]), attention_mask=t(m), encoder_hidden_states=enc, return_dict=True,
                             output_hidden_states=(name == "right"))
            out[f"mm_{name}"] = kept(o.last_hidden_state, m, pre)
            if name == "right":
                assert len(o.hidden_states) == 3 and torch.equal(o.hidden_states[2], o.last_hidden_state)
                out["mm_right_hidden0"], out["mm_right_hidden1"] = o.hidden_states[0].numpy(), o.hidden_states[1].numpy()
        # ---- encoder_attention_mask: prefix and with holes (self-attention mask: right-padded)
        for name, em in enc_masks.items():
            o = text_encoder(t(ids["right"]), attention_mask=t(masks["right"]), encoder_hidden_states=enc,
                             encoder_attention_mask=t(em), return_dict=True)
            out[f"mm_right_enc{name}"] = o.last_hidden_state.numpy()
        # ---- decoder: causal x padding mask, labels with -100 on the padding, both reductions
        for name, em in (("right", enc_masks["prefix"]), ("left", None)):
            m = masks[name]
            d_ids = ids[name].copy()
            d_ids[d_ids == CLS] = DEC
            labels = np.where(m == 1, d_ids, -100)
            if name == "left":              # the first real token is predicted FROM a padded position, whose logits the contract
                labels[np.arange(B), T - np.asarray(LENS)] = -100       # does not specify: ignored, as a prompt is (models/blip.py:114)
            kw = dict(attention_mask=t(m), encoder_hidden_states=enc, labels=t(labels), return_dict=True)
            if em is not None:
                kw["encoder_attention_mask"] = t(em)
            o_none = text_decoder(t(d_ids), reduction="none", **kw)
            o_mean = text_decoder(t(d_ids), **kw)
            lg = text_decoder(t(d_ids), return_logits=True, **kw)
            assert torch.equal(lg, o_none.logits[:, :-1]) and torch.equal(o_mean.logits, o_none.logits)
            out[f"dec_{name}_ids"], out[f"dec_{name}_labels"] = d_ids, labels
            out[f"dec_{name}_logits"] = kept(o_none.logits, m, name == "right")
            out[f"dec_{name}_loss_none"] = o_none.loss.numpy()
            out[f"dec_{name}_loss_mean"] = np.asarray(o_mean.loss.item(), dtype=np.float32)
        # ---- BLIP_Base (models/blip.py:45-73): each caption alone, at its own length, over its image's ViT tokens
        _, g_vit = load_golden("vit_small.npz")
        y = t(g_vit["y"])                                              # [3, 17, 256]
        base_text = np.zeros((len(BASE_LENS), max(BASE_LENS), 256), dtype=np.float32)
        base_mm = np.zeros_like(base_text)
        for b, n in enumerate(BASE_LENS):
            row = t(base_ids[b:b + 1, :n].copy())
            att = torch.ones_like(row)
            base_text[b, :n] = text_encoder(row, attention_mask=att, return_dict=True, mode="text").last_hidden_state[0].numpy()
            row[:, 0] = ENC
            image_embeds = y[b:b + 1]
            image_atts = torch.ones(image_embeds.size()[:-1], dtype=torch.long)
            base_mm[b, :n] = text_encoder(row, attention_mask=att, encoder_hidden_states=image_embeds,
                                          encoder_attention_mask=image_atts, return_dict=True).last_hidden_state[0].numpy()
        out["base_text"], out["base_mm"] = base_text, base_mm
    path = os.path.join(HERE, "forward_small.npz")
    np.savez_compressed(path, **out)
    print(f"forward_small.npz: {os.path.getsize(path) / 1e6:.2f} MB, logit scale "
          f"{max(np.abs(out['dec_right_logits']).max(), np.abs(out['dec_left_logits']).max()):.3f}")


def write_names():
    """The reference's parameter names (defaults included) of both forwards, and the state-dict key names of its BLIP_Base
    (models/blip.py:22-42) and BLIP_Embedding (models/blip_embedding.py:10-38) members at full size."""
    vit_mod, med = ref_shim.load()

    def params(f):
        return [[n, None if p.default is inspect.Parameter.empty else p.default]
                for n, p in inspect.signature(f).parameters.items() if n != "self"]

    with open(os.path.join(HERE, "forward_signatures.json"), "w") as f:
        json.dump({"BertModel.forward": params(med.BertModel.forward),
                   "BertLMHeadModel.forward": params(med.BertLMHeadModel.forward)}, f, indent=0)

    def vit(size):
        return vit_mod.VisionTransformer(img_size=size, patch_size=16, embed_dim=768, depth=12, num_heads=12,
                                         use_grad_checkpointing=False, ckpt_layer=0, drop_path_rate=0)

    enc = med.BertModel(config=ref_shim.med_config(encoder_width=768), add_pooling_layer=False)
    base = sorted([f"visual_encoder.{k}" for k in vit(224).state_dict()] + [f"text_encoder.{k}" for k in enc.state_dict()])
    heads = [f"{m}.{p}" for m in ("vision_proj", "text_proj", "itm_head") for p in ("weight", "bias")]
    emb = sorted([f"visual_encoder.{k}" for k in vit(384).state_dict()] + [f"text_encoder.{k}" for k in enc.state_dict()] + heads)
    for name, keys in (("blip_base_keys.json", base), ("blip_embedding_keys.json", emb)):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(keys, f, indent=0)
        print(f"{name}: {len(keys)} names")


if __name__ == "__main__":
    write_names() if len(sys.argv) > 1 and sys.argv[1] == "names" else main()
