"""NLVR2 evaluation on the library's own schedule.  The reference's call shape (``BLIP_NLVR.forward``: one ViT pass over both
images of every sentence) costs a ViT pass per sentence, while NLVR2 asks several sentences about the same image pair and
shows the same image in several pairs.  ``evaluation`` instead

  * runs the ViT once per DISTINCT image;
  * takes the distinct ordered pairs (i0, i1) as the cross-attention units and sorts the sentences pair-major
    (``video.group_table``, ``video.blocks``);
  * per block of pairs projects the two K | V sets once per pair and runs ONE twin pass over the block's sentences with the
    ``group_start`` table, so one staging of a pair's K / V serves all its sentences.

Every block is launched with the same token count (the longest sentence of all) and the same ``max_group`` bound, so a
sentence's bits do not depend on the block size (as ``video_retrieval.evaluation`` guarantees for its pairs)."""
from __future__ import annotations

import json

import numpy as np
import torch

from . import video as V
from .video_retrieval import pre_caption

VIT_IMAGES = 64                  # images per ViT pass of ``evaluation``


def load_nlvr_annotations(path):
    """A JSON list of objects with ``images`` (two file names), ``sentence`` and ``label`` (data/nlvr_dataset.py:37-52) ->
    (image_names, examples): the distinct file names in order of first appearance, and per annotation (i0, i1,
    pre_caption(sentence, 40), label == 'True') with i0 / i1 indices into image_names.  The dataset's random left / right swap
    (:54-75) is training augmentation and is not applied."""
    with open(path, "r") as f:
        ann = json.load(f)
    index, examples = {}, []
    for a in ann:
        i0, i1 = (index.setdefault(name, len(index)) for name in a["images"][:2])
        examples.append((i0, i1, pre_caption(a["sentence"], 40), 1 if a["label"] == "True" else 0))
    return list(index), examples


def pair_major_order(examples, n_images):
    """The pair-major order of the examples (host; pure).  Returns a dict: ``pairs`` int64 [U, 2] — the distinct ordered image
    pairs, sorted; ``order`` int64 [n] — the caller's index of the example at every sorted position (stable); ``group_start``
    int32 [U+1] / ``max_group`` — the sorted examples of pair u are group_start[u] .. group_start[u+1]-1."""
    ij = torch.tensor([[e[0], e[1]] for e in examples], dtype=torch.int64).view(-1, 2)
    if ij.numel() and not (0 <= int(ij.min()) and int(ij.max()) < n_images):
        raise ValueError(f"nlvr.evaluation: an example names an image outside 0..{n_images - 1}")
    keys, unit = torch.unique(ij[:, 0] * n_images + ij[:, 1], sorted=True, return_inverse=True)
    pairs = torch.stack([torch.div(keys, n_images, rounding_mode="floor"), keys % n_images], 1)
    group_start, max_group = V.group_table(unit, keys.numel(), "pair_of_example")
    return dict(pairs=pairs, order=torch.argsort(unit, stable=True), group_start=group_start, max_group=max_group)


def default_pairs_per_block(model, tokens_per_image):
    """Pairs whose two K | V sets fit video.KV_BLOCK_BYTES."""
    return max(1, V.videos_per_block(model.text_encoder.config, tokens_per_image) // 2)


@torch.no_grad()
def evaluation(model, images_u8, examples, *, pairs_per_block=None):
    """``model``: a BLIP_NLVR on the GPU; ``images_u8``: uint8 [I, S, S, 3] (numpy or torch; already S x S; /255 and the
    normalisation are fused into the patch kernel); ``examples``: (i0, i1, sentence, label) per example, i0 / i1 indices
    into the images.  Returns (predictions f32 numpy [n, 2] in input order, accuracy = mean(argmax == label))."""
    model._require_plain()
    n = len(examples)
    if n == 0:
        return np.zeros((0, 2), dtype=np.float32), float("nan")
    dev = next(model.parameters()).device
    images = torch.as_tensor(images_u8)
    if images.dim() != 4 or images.shape[-1] != 3 or images.dtype != torch.uint8:
        raise ValueError(f"nlvr.evaluation: uint8 [I,S,S,3] expected, got {images.dtype} {tuple(images.shape)}")
    n_images = images.shape[0]
    sched = pair_major_order(examples, n_images)
    order = sched["order"]
    ids, lens = model.tokenize([examples[int(i)][2] for i in order])          # (before any launch: may refuse a long sentence)
    T = ids.shape[1]
    max_group = max(sched["max_group"], -(-33 // T))
    parts = [model.visual_encoder.forward_u8(images[i:i + VIT_IMAGES].to(dev), V.CLIP_MEAN, V.CLIP_STD)[1]
             for i in range(0, n_images, VIT_IMAGES)]
    tokens = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    Te = tokens.shape[0] // n_images
    tokens = tokens.view(n_images, Te, -1)
    if pairs_per_block is None:
        pairs_per_block = default_pairs_per_block(model, Te)
    if pairs_per_block < 1:
        raise ValueError(f"nlvr.evaluation: pairs_per_block={pairs_per_block}")
    pairs = sched["pairs"].to(dev)
    preds = []
    for b0, b1, p0, p1, groups in V.blocks(sched["group_start"], pairs.shape[0], pairs_per_block):
        side = [tokens.index_select(0, pairs[b0:b1, j]).view((b1 - b0) * Te, -1) for j in (0, 1)]
        preds.append(model.predict(side[0], side[1], b1 - b0, ids[p0:p1], lens[p0:p1], groups=groups, max_group=max_group))
    sorted_pred = (preds[0] if len(preds) == 1 else torch.cat(preds, 0)).cpu()
    out = torch.empty_like(sorted_pred)
    out[order] = sorted_pred
    labels = torch.tensor([int(e[3]) for e in examples])
    return out.numpy(), float((out.argmax(1) == labels).float().mean())
