"""Shared by the video-retrieval tests: the small BLIP_Retrieval geometry of tests/test_retrieval_gpu.py (hidden 256, 4 heads,
2 layers, embed 64) at 128 x 128 frames (65 tokens per frame), its inputs, and the fp32 oracle of the video-level evaluation
composed from the unmodified oracle/ (retrieval_ref, med_ref): eval_retrieval_video.py:37-118 with EVERY (video, text) pair
scored."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from common import perturb_, synthetic_frames

SIZE, TOKENS, LAYERS, HEADS = 128, 65, 2, 4
N_VIDEOS, K_TEST = 5, 3
TEXTS = ["w1000", "w1037 w2001", "w1074 w2002 w3003 w1200 w1300", "w3033", "w1148 w2004 w1149 w2005 w1150 w2006 w1151 w2007 w1152",
         "w1185 w2005 w3100", "w1222 w2006 w3066 w3067 w3068 w3069 w3070 w3071 w3072 w3073 w3074 w3075 w3076 w3077"]


def small_video_retrieval(tmp_path):
    from vidil_amd.blip_retrieval import BLIP_Retrieval
    from vidil_amd.med import BertModel
    from vidil_amd.tokenizer import SyntheticBertTokenizer
    from vidil_amd.vit import VisionTransformer

    cfg = dict(architectures=["BertModel"], hidden_act="gelu", hidden_size=256, initializer_range=0.02, intermediate_size=512,
               layer_norm_eps=1e-12, max_position_embeddings=64, model_type="bert", num_attention_heads=HEADS,
               num_hidden_layers=LAYERS, pad_token_id=0, type_vocab_size=2, vocab_size=30524, encoder_width=256,
               add_cross_attention=True)
    path = os.path.join(str(tmp_path), "med_small.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    torch.manual_seed(11)
    m = BLIP_Retrieval(med_config=path, image_size=SIZE, vit="base", embed_dim=64, tokenizer=SyntheticBertTokenizer())
    m.visual_encoder = VisionTransformer(img_size=SIZE, patch_size=16, embed_dim=256, depth=LAYERS, num_heads=HEADS)
    m.vision_proj = torch.nn.Linear(256, 64)
    tcfg = m.text_encoder.config
    tcfg.encoder_width = 256
    m.text_encoder = BertModel(config=tcfg, add_pooling_layer=False)
    m = m.eval()
    perturb_(m, 700)
    with torch.no_grad():                                       # spread the similarities and the ITM logits
        m.vision_proj.weight.mul_(8); m.text_proj.weight.mul_(8); m.itm_head.weight.mul_(20)
    return m


def frames(n_frames):
    """uint8 [5, N, 128, 128, 3]."""
    return synthetic_frames(N_VIDEOS, n_frames, size=SIZE, first_video=61)


def contrast_frames():
    """uint8 [2, 4, 128, 128, 3]: videos whose frames project to very different lengths (noise, black, white, a ramp), so that
    the mean of the projections and the mean of the normalised projections point apart."""
    u8 = synthetic_frames(2, 4, size=SIZE, first_video=71)
    u8[:, 1] = 0
    u8[:, 2] = 255
    u8[:, 3] = (np.arange(SIZE, dtype=np.uint8) * 2)[None, None, :, None]
    u8[1, 0] //= 8
    return u8


def cancel_black_frame_(model_cpu, u8):
    """vision_proj.bias -= 0.9 * (projection of frame [0, 1], the black one): that frame then projects to a tenth of the length
    of the others — frames of very different lengths are what tells the mean of the projections from the mean of the
    normalised projections (with the plain weights every frame projects to a length of 30..34)."""
    from oracle import clip_ref, retrieval_ref

    sd = {k: v.clone() for k, v in model_cpu.state_dict().items()}
    with torch.no_grad():
        y, _ = retrieval_ref.image_features(sd, clip_ref.preprocess_u8(u8[0, 1:2]), depth=LAYERS, heads=HEADS)
        model_cpu.vision_proj.bias -= 0.9 * F.linear(y[:, 0], sd["vision_proj.weight"], sd["vision_proj.bias"])[0]
    return model_cpu


def video_embeds_ref(sd, u8):
    """(tokens [B, N*T, C], mean-then-normalise [B, E] — eval_retrieval_video.py:64-67 —, normalise-then-mean-then-normalise)."""
    from oracle import clip_ref, retrieval_ref

    B, N = u8.shape[:2]
    x = clip_ref.preprocess_u8(u8.reshape(B * N, *u8.shape[2:]))
    with torch.no_grad():
        y, _ = retrieval_ref.image_features(sd, x, depth=LAYERS, heads=HEADS)
        proj = F.linear(y[:, 0, :], sd["vision_proj.weight"], sd["vision_proj.bias"]).view(B, N, -1)
    return (y.reshape(B, N * y.shape[1], y.shape[2]), F.normalize(proj.mean(dim=1), dim=-1),
            F.normalize(F.normalize(proj, dim=-1).mean(dim=1), dim=-1))


def oracle(model_cpu, u8):
    """dict: vid_emb [5, E], txt_emb [7, E], sims [5, 7], itm [5, 7] (logit of class 1 of every pair, ids[:, 0] := [ENC])."""
    from oracle import med_ref, retrieval_ref

    sd = {k: v.clone() for k, v in model_cpu.state_dict().items()}
    tokens, vid_emb, _ = video_embeds_ref(sd, u8)
    ids, lens = model_cpu.tokenize(TEXTS)
    ids = ids.long()
    mask = (torch.arange(ids.shape[1])[None] < lens[:, None]).long()
    with torch.no_grad():
        txt_emb = retrieval_ref.text_features(sd, ids, mask, layers=LAYERS, H=HEADS)
        ids_enc = ids.clone()
        ids_enc[:, 0] = model_cpu.tokenizer.enc_token_id
        itm = torch.empty(u8.shape[0], len(TEXTS))
        for v in range(u8.shape[0]):
            h, _ = med_ref.bert_model(sd, "text_encoder.", ids_enc, mask, layers=LAYERS, H=HEADS,
                                      enc=tokens[v].repeat(len(TEXTS), 1, 1), is_decoder=False)
            itm[v] = F.linear(h[:, 0, :], sd["itm_head.weight"], sd["itm_head.bias"])[:, 1]
    return dict(sd=sd, vid_emb=vid_emb, txt_emb=txt_emb, sims=vid_emb @ txt_emb.t(), itm=itm)
