"""Shared by the retrieval-loss tests and tests/golden/make_retrieval_loss_golden.py: the small geometry (tests/nlvr_cases.py:
hidden 256, 4 heads, ViT depth 2; two text layers; embed_dim 64), the models built from it with ``portable_init_`` weights (no
weights are stored), the inputs that are regenerated instead of stored (pixels, queue contents), and the restatement of the
loss in fp64 that the tests compare with.

What the reference's training forward computes, in this file's words.  With unit-norm features f (online) and g (momentum
towers) of the two modalities, keys K_x = [g_x of the batch ; queue_x before the call] for modality x, and temperature t:

    row b, image -> text:  s = f_img[b] . K_txt / t,   m = g_img[b] . K_txt / t,
                           target = alpha * softmax(m) + (1 - alpha) * e_b          (e_b: 1 at the batch's own column b)
                           loss   = - sum_j target_j * log_softmax(s)_j
    text -> image alike with the roles swapped; loss_ita = (mean_b i2t + mean_b t2i) / 2.

(The reference first builds targets from ``idx`` and then overwrites them with the diagonal: ``idx`` never enters this loss.)
After the loss, queue columns ptr .. ptr + B := g of the batch, idx_queue likewise := idx, ptr := (ptr + B) mod queue_size.
Negatives: for text b an image is drawn with weights softmax(f_txt[b] . f_img / t) where entries of the same idx are zero, and
for image b a text likewise.  loss_itm = cross-entropy of the 3B two-class logits against B ones then 2B zeros.
"""
import json
import os
import tempfile
from dataclasses import dataclass

import numpy as np
import torch

import nlvr_cases as nc
import vqa_cases as vq
from common import load_golden, portable_init_
from oracle import sample_ref

EMBED, TEXT_LAYERS, MOMENTUM = 64, 2, 0.995
SEED = 0
PRED_REL = nc.PRED_REL                      # the project's two-logit bound
TIE = 1e-5                                  # a draw whose threshold lies this close to a cumulative weight may be excluded
GOLDEN = "retrieval_loss_small.npz"
#: seeds of the own-draw test, chosen on the CPU so that no draw of the restatement on the golden's similarities is within TIE
#: of a cumulative weight (tests/test_retrieval_loss_cpu.py asserts it)
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
    idx: tuple               # per call
    alpha: tuple             # per call
    lens: tuple              # caption token counts ([CLS] .. [SEP] included), the same in both calls


CASES = (
    # B = 6, queue of 12: the second call wraps the pointer back to 0; one duplicate idx; alpha 0.4 then 0
    Case("image", False, 6, 1, 64, 12, 0.07, ((3, 7, 7, 1, 9, 4), (5, 2, 8, 8, 6, 0)), (0.4, 0.0), (5, 9, 12, 4, 7, 20)),
    # 2 frames x 17 tokens; queue of 16: the second call continues behind the first
    Case("video", True, 4, 2, 64, 16, 0.07, ((0, 1, 2, 3), (4, 4, 5, 6)), (0.4, 0.25), (6, 11, 4, 9)),
    # 3 frames x 257 tokens = 771 keys, past BertModel.LONG_KEYS: the matching pairs go image-major; temp 0.6 is clamped to 0.5
    Case("video_long", True, 4, 3, 256, 8, 0.6, ((10, 11, 11, 12), (13, 14, 15, 16)), (0.4, 0.1), (5, 8, 13, 6)),
)
CALLS = 2


def case(name):
    return next(c for c in CASES if c.name == name)


def cfg_fields():
    return nc.cfg_fields(TEXT_LAYERS)


def small_model(c, seed=SEED, momentum_state=True):
    """BLIP_Retrieval / BLIP_Retrieval_Video at the small geometry through its own constructor, on the CPU.  The online members
    get ``portable_init_(seed)``, every momentum member a seed of its own (so that the EMA and the momentum features are
    observable), the queues unit columns from numpy, ``temp`` the case's start value."""
    from vidil_amd.blip_retrieval import MOMENTUM_PAIRS, BLIP_Retrieval, BLIP_Retrieval_Video
    from vidil_amd.med import BertModel
    from vidil_amd.packing import parity_mode, set_parity_mode

    cls = BLIP_Retrieval_Video if c.video else BLIP_Retrieval
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "med_config.json")
        with open(path, "w") as f:
            json.dump(cfg_fields(), f)
        m = cls(med_config=path, image_size=32, vit="base", embed_dim=EMBED, queue_size=c.queue_size, momentum=MOMENTUM,
                tokenizer=vq.VqaTokenizer())
    m.visual_encoder = nc.small_vit(c.image_size)
    cfg = nc.small_cfg(TEXT_LAYERS)
    m.text_encoder = BertModel(config=cfg, add_pooling_layer=False)
    m.vision_proj = torch.nn.Linear(nc.HIDDEN, EMBED)
    set_parity_mode(parity_mode(m), m)
    portable_init_(m, seed)
    with torch.no_grad():
        m.temp.fill_(c.temp0)
    if momentum_state:
        m.ensure_momentum_state()
        rng = np.random.default_rng(seed + 500)
        with torch.no_grad():
            for i, (_, name_m) in enumerate(MOMENTUM_PAIRS):
                portable_init_(getattr(m, name_m), seed + 100 + i)
            for name in ("image_queue", "text_queue"):
                q = rng.standard_normal((EMBED, c.queue_size)).astype(np.float32)
                getattr(m, name).copy_(torch.from_numpy(q / np.linalg.norm(q, axis=0, keepdims=True)))
    return m.eval()


def pixels(c, call):
    """f32 [B,3,S,S] (video: [B,N,3,S,S]), standard normal from numpy."""
    rng = np.random.default_rng([sum(map(ord, c.name)), call, 77])
    shape = (c.B, c.frames, 3, c.image_size, c.image_size) if c.video else (c.B, 3, c.image_size, c.image_size)
    return torch.from_numpy(rng.standard_normal(shape, dtype=np.float32))


def draw_ids(c, call):
    """Right-padded ids [B, 35] ([CLS] words [SEP]) and their mask, as the synthetic tokenizer returns them for ``captions``."""
    rng = np.random.default_rng([sum(map(ord, c.name)), call, 78])
    ids, mask = np.zeros((c.B, 35), dtype=np.int64), np.zeros((c.B, 35), dtype=np.int64)
    for i, n in enumerate(c.lens):
        ids[i, :n] = rng.integers(110, 500, size=n)
        ids[i, 0], ids[i, n - 1] = 101, vq.SEP
        mask[i, :n] = 1
    return ids, mask


def captions(c, call):
    ids, mask = draw_ids(c, call)
    return [vq.words(row[1:n - 1]) for row, n in zip(ids, mask.sum(1))]


def golden():
    return load_golden(GOLDEN)[1]


# ------------------------------------------------------------------------------------------------ the restatement, fp64
def itc_rows64(f, g, keys, temp, alpha):
    """Row losses of one direction: f, g [B,D] online / momentum rows, keys [B+Q,D] (the batch's momentum rows first)."""
    f, g, keys = f.double(), g.double(), keys.double()
    s, m = f @ keys.T / temp, g @ keys.T / temp
    target = alpha * torch.softmax(m, 1)
    target[:, :f.shape[0]] += (1 - alpha) * torch.eye(f.shape[0], dtype=torch.float64)
    return -(target * torch.log_softmax(s, 1)).sum(1)


def loss_ita64(image_feat, text_feat, image_feat_m, text_feat_m, image_queue, text_queue, temp, alpha):
    """queues [D,Q] as they were BEFORE the call."""
    k_txt = torch.cat([text_feat_m.double(), text_queue.double().T])
    k_img = torch.cat([image_feat_m.double(), image_queue.double().T])
    i2t = itc_rows64(image_feat, image_feat_m, k_txt, temp, alpha).mean()
    t2i = itc_rows64(text_feat, text_feat_m, k_img, temp, alpha).mean()
    return float((i2t + t2i) / 2)


def loss_itm64(logits):
    """logits [3B,2]: B matching pairs, then 2B non-matching."""
    lg = logits.double()
    B = lg.shape[0] // 3
    label = torch.cat([torch.ones(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long)])
    return float((torch.logsumexp(lg, 1) - lg[torch.arange(3 * B), label]).mean())


def draws(sim, idx, seed, stream):
    """The inverse-CDF draws of this library's contract on sim f32 [B,B] (already / temp): weights = f32 softmax with the
    same-idx entries zeroed, c = cumulative sums in index order (f32, sequential), u = Philox uniform of (seed, row, stream);
    the draw is the first j with c_j > u * c_last.  -> (draws int64 [B], close bool [B]: the threshold is within TIE of some
    c_j, so another order of summation may decide otherwise)."""
    sim = sim.float().cpu()
    idx = torch.as_tensor(idx).view(-1)
    w = torch.softmax(sim, 1).masked_fill(idx.view(-1, 1) == idx.view(1, -1), 0.0).numpy()
    out, close = [], []
    for b in range(w.shape[0]):
        c = np.cumsum(w[b], dtype=np.float32)
        t = np.float32(sample_ref.uniform(seed, b, stream)) * c[-1]
        out.append(int(np.argmax(c > t)))
        close.append(bool((np.abs(c.astype(np.float64) - float(t)) < TIE).any()))
    return torch.tensor(out), torch.tensor(close)
