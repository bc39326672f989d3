"""Shared by the pretraining-forward tests and tests/golden/make_pretrain_golden.py: the small geometry and builders of
tests/retrieval_loss_cases.py (hidden 256, 4 heads, ViT depth 2, two text layers, embed_dim 64, ``portable_init_`` weights — none
are stored —, the momentum members from seeds of their own, the synthetic ``VqaTokenizer``), the inputs that are regenerated
instead of stored, and the fp64 restatements the tests compare with.

What the reference's pretraining forward computes beyond the retrieval loss (whose contrastive part, ``rc.loss_ita64``, it shares):

    draw weights   for text b:  softmax_j(f_txt[b] . g_img[j] / t) + 1e-4, entry b zeroed       (g: the momentum towers' features)
                   for image b: softmax_j(f_img[b] . g_txt[j] / t) + 1e-4, entry b zeroed
    loss_itm       cross-entropy of the 3B two-class logits against B ones then 2B zeros          (``rc.loss_itm64``)
    loss_lm        ids with the first := [DEC]; the logits at position t are scored against token t + 1 for every real token
                   t + 1 >= 1; a token's loss is -(0.9 * lp[label] + 0.1 * mean_j lp[j]); the mean over ALL target tokens.
"""
import json
import os
import tempfile
from dataclasses import dataclass

import numpy as np
import torch

import nlvr_cases as nc
import retrieval_loss_cases as rc
import vqa_cases as vq
from common import load_golden, portable_init_
from vidil_amd import blip_pretrain as bp     # (at import: without the pretraining models every test that uses this file fails here)
from oracle import sample_ref

EMBED, TEXT_LAYERS, MOMENTUM, SEED = rc.EMBED, rc.TEXT_LAYERS, rc.MOMENTUM, rc.SEED
PRED_REL, TIE = rc.PRED_REL, rc.TIE
MAX_LENGTH = 30                             # models/blip_pretrain.py:105
GOLDEN = "pretrain_small.npz"
KEYS = "blip_pretrain_keys.json"
#: seeds of the own-draw test, chosen on the CPU so that no draw of the restatement on the golden's similarity blocks is within
#: TIE of a cumulative weight (tests/test_pretrain_cpu.py asserts it, for seed and seed + 1: the two calls)
DRAW_SEEDS = {"image": 3, "video": 3, "video_long": 3}


@dataclass(frozen=True)
class Case:
    name: str
    video: bool
    B: int
    frames: int
    image_size: int          # 64 -> 17 tokens per frame, 256 -> 257
    queue_size: int
    temp0: float             # the temperature parameter before the first call (0.6 is clamped to 0.5)
    alpha: tuple             # per call
    words: tuple             # words per caption, the same in both calls: words + 2 tokens, cut to MAX_LENGTH


CASES = (
    # B = 6, queue of 12: the second call wraps the pointer back to 0; alpha 0.4 then 0; a caption of 34 tokens, cut to 30 (the
    # tokenizer closes a cut caption with [SEP], as HF's does), and one of 3 tokens ([DEC] w [SEP]: two targets)
    Case("image", False, 6, 1, 64, 12, 0.07, (0.4, 0.0), (3, 32, 10, 1, 5, 18)),
    # 2 frames x 17 tokens; queue of 16: the second call continues behind the first
    Case("video", True, 4, 2, 64, 16, 0.07, (0.4, 0.25), (4, 9, 2, 7)),
    # 3 frames x 257 tokens = 771 keys, past BertModel.LONG_KEYS: the matching pairs go image-major and the decoder's
    # cross-attention takes the long-key form; temp 0.6 is clamped to 0.5
    Case("video_long", True, 4, 3, 256, 8, 0.6, (0.4, 0.1), (3, 6, 11, 4)),
)
CALLS = 2
pixels = rc.pixels                          # f32 [B,3,S,S] (video: [B,N,3,S,S]) of (case name, call)


def case(name):
    return next(c for c in CASES if c.name == name)


def lens(c):
    return [min(MAX_LENGTH, w + 2) for w in c.words]


def small_model(c, seed=SEED):
    """BLIP_Pretrain / BLIP_Pretrain_Video at the small geometry, on the CPU.  The class's own constructor runs (on the meta
    device: names only), then every member is rebuilt small the way the constructor builds it: encoder and decoder tied, the
    momentum state from ``ensure_momentum_state``.  The online members get ``portable_init_(seed)``, every momentum member a seed
    of its own, the queues unit columns from numpy, ``temp`` the case's start value."""
    from vidil_amd.blip_retrieval import MOMENTUM_PAIRS
    from vidil_amd.med import BertLMHeadModel, BertModel
    from vidil_amd.packing import set_parity_mode

    cls = bp.BLIP_Pretrain_Video if c.video else bp.BLIP_Pretrain
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "med_config.json")
        with open(path, "w") as f:
            json.dump(rc.cfg_fields(), f)
        with torch.device("meta"):
            m = cls(med_config=path, image_size=32, vit="base", embed_dim=EMBED, queue_size=c.queue_size, momentum=MOMENTUM,
                    tokenizer=vq.VqaTokenizer())
    for _, name_m in MOMENTUM_PAIRS:
        delattr(m, name_m)
    for name in ("image_queue", "text_queue", "queue_ptr"):
        delattr(m, name)
    cfg = nc.small_cfg(TEXT_LAYERS)
    m.visual_encoder = nc.small_vit(c.image_size)
    m.text_encoder = BertModel(config=cfg, add_pooling_layer=False)
    m.text_decoder = BertLMHeadModel(config=cfg)
    m.vision_proj, m.text_proj = torch.nn.Linear(nc.HIDDEN, EMBED), torch.nn.Linear(nc.HIDDEN, EMBED)
    m.itm_head = torch.nn.Linear(nc.HIDDEN, 2)
    m.temp = torch.nn.Parameter(torch.zeros([]))
    bp.tie_encoder_decoder_weights(m.text_encoder, m.text_decoder.bert)
    set_parity_mode(False, m)
    portable_init_(m, seed)
    with torch.no_grad():
        m.temp.fill_(c.temp0)
    m.ensure_momentum_state()
    rng = np.random.default_rng(seed + 500)
    with torch.no_grad():
        for i, (_, name_m) in enumerate(MOMENTUM_PAIRS):
            portable_init_(getattr(m, name_m), seed + 100 + i)
        for name in ("image_queue", "text_queue"):
            q = rng.standard_normal((EMBED, c.queue_size)).astype(np.float32)
            getattr(m, name).copy_(torch.from_numpy(q / np.linalg.norm(q, axis=0, keepdims=True)))
    return m.eval()


def captions(c, call):
    rng = np.random.default_rng([sum(map(ord, c.name)), call, 79])
    return [vq.words(rng.integers(110, 500, size=n)) for n in c.words]


def token_ids(c, call):
    """(ids int64 [B, 30] with [CLS] first, mask) as the tokenizer pads and cuts the captions."""
    enc = vq.VqaTokenizer()(captions(c, call), padding="max_length", truncation=True, max_length=MAX_LENGTH, return_tensors="pt")
    return enc.input_ids, enc.attention_mask


def golden():
    return load_golden(GOLDEN)[1]


# ------------------------------------------------------------------------------------------------ the restatements, fp64
loss_ita64, loss_itm64 = rc.loss_ita64, rc.loss_itm64


def lm_targets(ids, mask):
    """Labels [B, T] of the LM loss: labels[b, t] = ids[b, t + 1] where t + 1 is a real token, -100 elsewhere (:199-201 and the
    shift of models/med.py:912-913)."""
    lab = torch.full_like(ids, -100)
    lab[:, :-1] = torch.where(mask[:, 1:] > 0, ids[:, 1:], torch.full_like(ids[:, 1:], -100))
    return lab


def loss_lm64(lp_label, lp_mean):
    """From the per-target log-probability of the label and the mean log-probability over the vocabulary."""
    return float(-(0.9 * lp_label.double() + 0.1 * lp_mean.double()).sum() / lp_label.numel())


def loss_lm_of_logits64(logits, ids, mask):
    """logits [B, T, V] -> (loss, lp_label [n], lp_mean [n]) over the targets in caption-major order."""
    lp = torch.log_softmax(logits.double(), -1)
    lab = lm_targets(ids, mask)
    b, t = (lab >= 0).nonzero(as_tuple=True)
    lp_label, lp_mean = lp[b, t, lab[b, t]], lp[b, t].mean(-1)
    return loss_lm64(lp_label, lp_mean), lp_label, lp_mean


def draw_weights(sim):
    """f32 softmax of a [B,B] block (already / temp) + 1e-4 with the diagonal zeroed (models/blip_pretrain.py:155-158)."""
    return (torch.softmax(sim.float().cpu(), 1) + 1e-4).fill_diagonal_(0)


def draws(sim, seed, stream):
    """The inverse-CDF draws of this library's contract on a block: c = cumulative sums of ``draw_weights`` in index order (f32,
    sequential), u = Philox uniform of (seed, row, stream); the draw is the first j with c_j > u * c_last.  -> (draws int64 [B],
    close bool [B]: the threshold is within TIE of some c_j, so another order of summation may decide otherwise)."""
    w = draw_weights(sim).numpy()
    out, close = [], []
    for b in range(w.shape[0]):
        c = np.cumsum(w[b], dtype=np.float32)
        t = np.float32(sample_ref.uniform(seed, b, stream)) * c[-1]
        out.append(int(np.argmax(c > t)))
        close.append(bool((np.abs(c.astype(np.float64) - float(t)) < TIE).any()))
    return torch.tensor(out), torch.tensor(close)


# ------------------------------------------------------------------------------------------------ select_frame
SELECT_FRAMES, SELECT_SIZE = 3, 64
#: (seed of the frames, caption): two and three sentences after pretrain_video.py's sentence_tokenization
SELECT_CASES = ((21, "w120 w121 w122. w300 w301 w302 w303 w304"), (28, "w130 w131 w132: w310 w311 w312 w313\nw400 w401 w402 w403 w404"))
ITM_HEAD_GAIN = 20.0                        # itm_head.weight is multiplied by this so that the scores spread ...
ITM_BIAS_SHIFT = -0.6                       # ... and this is added to the bias of class 1, which centres them around 0.5


def small_filterer(seed=SEED + 40):
    """BLIP_ITM at the small geometry at 64 x 64 (17 tokens per frame), on the CPU."""
    from vidil_amd.blip_itm import BLIP_ITM
    from vidil_amd.med import BertModel
    from vidil_amd.packing import parity_mode, set_parity_mode

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "med_config.json")
        with open(path, "w") as f:
            json.dump(rc.cfg_fields(), f)
        with torch.device("meta"):
            m = BLIP_ITM(med_config=path, image_size=32, vit="base", embed_dim=EMBED, tokenizer=vq.VqaTokenizer())
    m.visual_encoder = nc.small_vit(SELECT_SIZE)
    m.text_encoder = BertModel(config=nc.small_cfg(TEXT_LAYERS), add_pooling_layer=False)
    m.vision_proj, m.text_proj = torch.nn.Linear(nc.HIDDEN, EMBED), torch.nn.Linear(nc.HIDDEN, EMBED)
    m.itm_head = torch.nn.Linear(nc.HIDDEN, 2)
    set_parity_mode(parity_mode(m), m)
    portable_init_(m, seed)
    with torch.no_grad():
        m.itm_head.weight.mul_(ITM_HEAD_GAIN)
        m.itm_head.bias[1] += ITM_BIAS_SHIFT
    return m.eval()


def select_pixels(seed):
    """f32 [3, 3, 64, 64], standard normal from numpy."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((SELECT_FRAMES, 3, SELECT_SIZE, SELECT_SIZE), dtype=np.float32))


class NaiveNlp:
    """A sentence splitter with spaCy's call shape (``nlp(text).sents`` of objects with ``.text``) that splits on '. '."""

    class _Span:
        def __init__(self, text):
            self.text = text

    def __call__(self, text):
        self.sents = [self._Span(s) for s in text.split(". ")]
        return self


def select_oracle(filterer_cpu, frames, sentences):
    """softmax(ITM logits)[:, 1] f32 [S, N] of every sentence against every frame, composed from oracle/ on the CPU."""
    from oracle import med_ref, retrieval_ref

    sd = {k: v.clone() for k, v in filterer_cpu.state_dict().items()}
    ids, ln = filterer_cpu.tokenize(sentences)
    ids = ids.long()
    mask = (torch.arange(ids.shape[1])[None] < ln[:, None]).long()
    N = frames.shape[0]
    with torch.no_grad():
        tokens, _ = retrieval_ref.image_features(sd, frames, depth=2, heads=nc.HEADS)
        out = torch.empty(len(sentences), N)
        for s in range(len(sentences)):
            h, _ = med_ref.bert_model(sd, "text_encoder.", ids[s:s + 1].repeat(N, 1), mask[s:s + 1].repeat(N, 1), layers=TEXT_LAYERS,
                                      H=nc.HEADS, enc=tokens, is_decoder=False)
            lg = torch.nn.functional.linear(h[:, 0, :], sd["itm_head.weight"], sd["itm_head.bias"])
            out[s] = torch.softmax(lg, 1)[:, 1]
    return out
