"""Shared by the NLVR tests and tests/golden/make_nlvr_golden.py: the small geometry (hidden 256, 4 heads, 8 layers — six
averaging, two merging —, intermediate 512, vocabulary 512, 64 positions, encoder width 256; ViT embed 256, depth 2, 4 heads at
480 x 480 = 901 tokens), the models built from it with ``portable_init_`` weights (numpy PCG64: the same bits on every host, so
no weights are stored), and the inputs that are regenerated instead of stored (encoder states, pixels)."""
import json
import os
import tempfile

import numpy as np
import torch

import vqa_cases as vq
from common import portable_init_, synthetic_frames

HIDDEN, HEADS, LAYERS, INTER, VOCAB, POSITIONS = 256, 4, 8, 512, 512, 64
IMAGE_SIZE, TOKENS = 480, 901
PAD, SEP, ENC = vq.PAD, vq.SEP, vq.ENC
SEED = 0                                   # the golden's seed (make_nlvr_golden.py search)
HEAD_GAIN = 20.0                           # cls_head.2.weight is multiplied by this so that the logits spread
PRED_REL = 2e-3                            # the project's two-logit bound (tests/test_models_gpu.py:174)
HIDDEN_TOL = 6e-3                          # tests/test_forward_surface_gpu.py

#: (name, encoder states per image, sentence lengths, pair of each sentence or None for one pair per sentence)
CASES = (("S", 17, (3, 9, 20), None),
         ("La", TOKENS, (9, 40), None),            # more than 32 query rows per unit
         ("Lb", TOKENS, (5, 9), None),             # at most 32
         ("G17", 17, (4, 12, 7, 9, 5), (0, 0, 0, 1, 1)),
         ("G901", TOKENS, (4, 12, 7, 9, 5), (0, 0, 0, 1, 1)))
E_LENS = (7, 11)
G_LABELS = (1, 0, 0, 1, 1)                 # the labels evaluation's accuracy is checked against


def cfg_fields(layers=LAYERS):
    return dict(hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=INTER, num_hidden_layers=layers,
                vocab_size=VOCAB, max_position_embeddings=POSITIONS)


def small_cfg(layers=LAYERS):
    from vidil_amd.med import BertConfig

    return BertConfig(encoder_width=HIDDEN, **cfg_fields(layers))


def small_vit(image_size=IMAGE_SIZE):
    from vidil_amd.vit import VisionTransformer

    return VisionTransformer(img_size=image_size, patch_size=16, embed_dim=HIDDEN, depth=2, num_heads=HEADS)


def small_model(seed=SEED, image_size=IMAGE_SIZE, layers=LAYERS, init=True):
    """BLIP_NLVR at the small geometry, through its own constructor (a med_config file), on the CPU."""
    from vidil_amd.blip_nlvr import BLIP_NLVR
    from vidil_amd.nlvr_encoder import BertModel
    from vidil_amd.packing import parity_mode, set_compute_dtype, set_parity_mode

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "med_config.json")
        with open(path, "w") as f:
            json.dump(cfg_fields(layers), f)
        m = BLIP_NLVR(med_config=path, image_size=32, vit="base", tokenizer=vq.VqaTokenizer())
    m.visual_encoder = small_vit(image_size)
    m.text_encoder = BertModel(small_cfg(layers))
    set_parity_mode(parity_mode(m), m)                      # the members built here follow what the constructor pinned
    if m.__dict__.get("_compute_dtype") is not None:
        set_compute_dtype(m.__dict__["_compute_dtype"], m)
    if init:
        portable_init_(m, seed)
        with torch.no_grad():
            m.cls_head[2].weight.mul_(HEAD_GAIN)
    return m.eval()


def yardstick_encoder(seed=SEED):
    """The non-twin stack of the same geometry (med.BertModel, 8 layers): the existing plain path whose error is the yardstick."""
    from vidil_amd.med import BertModel

    return portable_init_(BertModel(small_cfg()), seed + 1000).eval()


def encoder_states(n, tokens, seed):
    """f32 [n, tokens, 256], f16-representable (the 16-bit cast inside the model is exact for f16)."""
    x = np.random.default_rng(seed).standard_normal((n, tokens, HIDDEN), dtype=np.float32)
    return torch.from_numpy(x).half().float()


def case_states(name, n_pairs, tokens):
    """(image 0 states, image 1 states) of a case: [n_pairs, tokens, 256] each."""
    salt = sum(ord(c) for c in name)
    return encoder_states(n_pairs, tokens, 7000 + salt), encoder_states(n_pairs, tokens, 8000 + salt)


def n_pairs(lens, pair_of):
    return len(lens) if pair_of is None else max(pair_of) + 1


def draw_ids(rng, lens):
    """Right-padded ids [n, max(lens)] ([ENC] .. [SEP]) and their 0 / 1 mask, int64 numpy."""
    T = max(lens)
    ids, mask = np.zeros((len(lens), T), dtype=np.int64), np.zeros((len(lens), T), dtype=np.int64)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(110, 500, size=n)
        ids[i, 0], ids[i, n - 1] = ENC, SEP
        mask[i, :n] = 1
    return ids, mask


def pixels():
    """uint8 [4, 480, 480, 3]: images 0, 1 are image0 of the two pairs of case E, images 2, 3 their image1."""
    return synthetic_frames(1, frames=4, size=IMAGE_SIZE)[0]


def sentences(ids, mask):
    return [vq.words(row[1:n - 1]) for row, n in zip(ids, mask.sum(1))]


def golden():
    from common import load_golden

    return load_golden("nlvr_small.npz")[1]
