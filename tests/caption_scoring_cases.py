"""Shared inputs of the caption-scoring tests (small geometry of tests/golden/med_decoder_small.npz: hidden 256, 4 heads,
2 layers, vocabulary 512, 3 images of 17 tokens) and the reference value composed from the existing oracle."""
import numpy as np
import torch

from common import load_golden
from oracle import med_ref
from vidil_amd.tokenizer import SyntheticBertTokenizer

PROMPT = "w7 w8 w9 "                 # the golden decoder's prompt ids 7 8 9 behind [DEC] = 510 (tests/golden/make_golden.py)
PROMPT_LENGTH = 4
IMAGE_INDEX = [0, 2, 2, 1, 0, 2, 1]
TOKEN_COUNTS = [PROMPT_LENGTH + 1, 6, 9, 17, 40, 55, 12]     # [DEC] .. [SEP] per caption; the 55-token string truncates to 40
LAYERS, HEADS, V = 2, 4, 512


class SmallTokenizer(SyntheticBertTokenizer):
    """The synthetic tokenizer with [DEC] inside the 512-entry vocabulary of the small geometry."""
    vocab_size = 512
    bos_token_id = 510


def captions():
    """Seven strings that contain the prompt, of TOKEN_COUNTS tokens each (words w10 .. w499, never a special id)."""
    rng = np.random.default_rng(11)
    out = []
    for n in TOKEN_COUNTS:
        words = [int(w) for w in rng.integers(110, 500, size=n - 2 - 3)]
        out.append((PROMPT + " ".join(f"w{w}" for w in words)).strip())
    return out


def small_state():
    sd, g = load_golden("med_decoder_small.npz")
    return sd, torch.from_numpy(g["enc"])                     # enc f32 [3, 17, 256]


def reference_targets(tokenizer, caps, prompt_length):
    """models/blip.py:109-114 restated literally: (input_ids, attention_mask, decoder_targets)."""
    text = tokenizer(caps, padding="longest", truncation=True, max_length=40, return_tensors="pt")
    text.input_ids[:, 0] = tokenizer.bos_token_id
    decoder_targets = text.input_ids.masked_fill(text.input_ids == tokenizer.pad_token_id, -100)
    decoder_targets[:, :prompt_length] = -100
    return text.input_ids, text.attention_mask, decoder_targets


def oracle_logits(sd, enc, ids, attention_mask, image_index):
    with torch.no_grad():
        h, _ = med_ref.bert_model(sd, "text_decoder.bert.", ids, attention_mask, enc=enc[torch.as_tensor(image_index)],
                                  is_decoder=True, layers=LAYERS, H=HEADS)
        return med_ref.lm_head(sd, "text_decoder.cls.", h)


def oracle_loss(logits, labels, reduction, label_smoothing=0.1):
    """models/med.py:912-917 on the oracle's logits, float32 on the CPU."""
    P = logits.shape[0]
    loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1),
                                             label_smoothing=label_smoothing, reduction=reduction)
    return loss.view(P, -1).sum(1) if reduction == "none" else loss


_REF = {}


def reference():
    """Computed once, shared, never modified: dict(ids, mask, labels, logits, none, mean, counts, lp) of the 7-caption batch."""
    if not _REF:
        sd, enc = small_state()
        ids, mask, labels = reference_targets(SmallTokenizer(), captions(), PROMPT_LENGTH)
        logits = oracle_logits(sd, enc, ids, mask, IMAGE_INDEX)
        _REF.update(ids=ids, mask=mask, labels=labels, logits=logits, none=oracle_loss(logits, labels, "none"),
                    mean=oracle_loss(logits, labels, "mean"), counts=(labels[:, 1:] >= 0).sum(1),
                    lp=torch.log_softmax(logits.double(), -1))
    return _REF
