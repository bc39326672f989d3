"""Developer benchmark: one end-to-end ``video_retrieval.evaluation`` at full size — a random-init BLIP_Retrieval (ViT-B/16),
``--videos`` synthetic videos of ``--frames`` frames at ``--size``^2 and as many synthetic texts, ``--k-test`` candidates per
row — with the split ViT / text features / cross K|V projection / pair stack (each phase synchronised).  One JSON line.

usage: python tools/bench_video_retrieval.py [--videos 1000] [--frames 8] [--size 224] [--k-test 64] [--batch 50]
                                             [--videos-per-block N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vidil_amd import video_retrieval as VR  # noqa: E402
from vidil_amd.blip_retrieval import BLIP_Retrieval  # noqa: E402
from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=1000)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--k-test", type=int, default=64)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--videos-per-block", type=int, default=0)
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_video_retrieval: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
torch.manual_seed(0)
model = BLIP_Retrieval(image_size=args.size, vit="base", tokenizer=SyntheticBertTokenizer()).eval().to(dev)
rng = np.random.default_rng(0)
texts = [" ".join(f"w{rng.integers(1000, 9000)}" for _ in range(rng.integers(3, 30))) for _ in range(args.videos)]


def videos():
    g = torch.Generator(device=dev).manual_seed(1)
    for b0 in range(0, args.videos, args.batch):
        b = min(args.batch, args.videos - b0)
        yield torch.randint(0, 256, (b, args.frames, args.size, args.size, 3), dtype=torch.uint8, device=dev, generator=g)


vpb = args.videos_per_block or None
# warm-up: a small evaluation through every kernel form of the timed one (same frames per video, same token counts)
VR.evaluation(model, [next(videos())[:4]], texts[:8], min(args.k_test, 4), videos_per_block=vpb)
torch.cuda.synchronize()
timings = {}
t0 = time.perf_counter()
v2t, t2v = VR.evaluation(model, videos(), texts, args.k_test, videos_per_block=vpb, timings=timings)
torch.cuda.synchronize()
total = time.perf_counter() - t0
union = int(((v2t != VR.FILL) | (t2v.T != VR.FILL)).sum())
line = dict(bench="video_retrieval_evaluation", videos=args.videos, texts=len(texts), frames=args.frames, size=args.size,
            k_test=args.k_test, keys_per_video=args.frames * ((args.size // 16) ** 2 + 1), pairs_scored=union,
            videos_per_block=vpb or VR.default_videos_per_block(model, args.frames * ((args.size // 16) ** 2 + 1)),
            total_s=round(total, 3), **{k + "_s": round(v, 3) for k, v in timings.items()})
print(json.dumps(line), flush=True)
if args.out:
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
