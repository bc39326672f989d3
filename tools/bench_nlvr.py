"""Developer benchmark: two-image reasoning at full size, two schedules through the SAME model — a random-init BLIP_NLVR
(ViT-B/16, bf16) at 384^2 and at the reference's 480^2 (901 image tokens: the long-key attention form), ``--pairs`` synthetic
image pairs with ``--per-pair`` synthetic sentences each (in a shuffled order).

  forward     the reference's call shape: ``model(cat([image0, image1]), text, None, train=False)`` on batches of 8 (pair,
              sentence) examples, so the ViT and both K | V projections run once per SENTENCE.
  evaluation  ``nlvr.evaluation``: the ViT once per distinct image, the K | V once per pair, one twin pass per block of pairs.

Each schedule runs once to warm up and once between two HIP events.  Recorded, not asserted: one JSON line with a run per image
size, also written to ``--out`` (default profiles/nlvr_bench.json).

usage: python tools/bench_nlvr.py [--pairs 64] [--per-pair 4] [--sizes 384,480] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vidil_amd import nlvr  # noqa: E402
from vidil_amd.blip_nlvr import BLIP_NLVR  # noqa: E402
from vidil_amd.packing import set_compute_dtype  # noqa: E402
from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402
from vidil_amd.video import CLIP_MEAN, CLIP_STD  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--per-pair", type=int, default=4)
ap.add_argument("--sizes", default="384,480")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlvr_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_nlvr: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
BATCH = 8                                         # examples per forward call


def whole(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, res


def bench(size):
    torch.manual_seed(0)
    model = BLIP_NLVR(image_size=size, vit="base", tokenizer=SyntheticBertTokenizer()).eval().to(dev)
    set_compute_dtype("bf16", model)
    rng = np.random.default_rng(0)
    P, n = args.pairs, args.pairs * args.per_pair
    images = torch.from_numpy(rng.integers(0, 256, size=(2 * P, size, size, 3), dtype=np.uint8)).to(dev)
    pair_of = rng.permutation(np.repeat(np.arange(P), args.per_pair))
    text = [" ".join(f"w{w}" for w in rng.integers(1000, 30000, size=int(k))) for k in rng.integers(6, 24, size=n)]
    examples = [(2 * int(p), 2 * int(p) + 1, t, int(rng.integers(0, 2))) for p, t in zip(pair_of, text)]
    mean = torch.tensor(CLIP_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, device=dev).view(1, 3, 1, 1)

    def forward_all(count):
        out = []
        for b0 in range(0, count, BATCH):
            ex = examples[b0:b0 + BATCH]
            idx = torch.tensor([e[0] for e in ex] + [e[1] for e in ex], device=dev)
            image = (images[idx].permute(0, 3, 1, 2).float() / 255.0 - mean) / std           # the caller's preprocessing
            out.append(model(image, [e[2] for e in ex], None, train=False))
        return torch.cat(out).cpu().numpy()

    forward_all(2 * BATCH)
    nlvr.evaluation(model, images, examples[:2 * BATCH])
    t_fwd, p_fwd = whole(lambda: forward_all(n))
    t_eval, (p_eval, _) = whole(lambda: nlvr.evaluation(model, images, examples))
    tokens = (size // 16) ** 2 + 1
    return dict(size=size, image_tokens=tokens, pairs=P, sentences_per_pair=args.per_pair, examples=n,
                dtype="bf16", weights="random-init", longest_sentence_tokens=int(model.tokenize(text)[0].shape[1]),
                forward=dict(batch=BATCH, total_s=round(t_fwd, 3), examples_per_s=round(n / t_fwd, 1)),
                evaluation=dict(pairs_per_block=nlvr.default_pairs_per_block(model, tokens), total_s=round(t_eval, 3),
                                examples_per_s=round(n / t_eval, 1)),
                evaluation_over_forward=round(t_fwd / t_eval, 2),
                max_abs_difference=round(float(np.abs(p_fwd - p_eval).max()), 5),
                same_argmax_share=round(float((p_fwd.argmax(1) == p_eval.argmax(1)).mean()), 4))


commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
box = dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__)
runs = []
for s in (int(x) for x in args.sizes.split(",")):
    runs.append(bench(s))
    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
result = dict(bench="nlvr", runs=runs, box=box, commit=commit or "unknown")
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
