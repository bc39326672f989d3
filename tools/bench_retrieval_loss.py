"""Developer benchmark: the whole loss forward of the retrieval models on random-init full-size weights (ViT-B/16, embed_dim 256,
queue 57,600) — ``BLIP_Retrieval`` at 384^2 with B = 32 and ``BLIP_Retrieval_Video`` at 224^2 x 8 frames with B = 16.  One call
is what a training step's forward is: both towers of both kinds (online and momentum), the EMA update (after which the momentum
towers re-pack their 16-bit operands), the contrastive loss over batch + queue, the enqueue, the negative draws and the matching
pass over 3B pairs.

Each model runs ``--warmup`` calls and then ``--iters`` calls between two HIP events, ``--rounds`` times; the median round is
reported with the spread.  Recorded, not asserted: one JSON line, also written to ``--out`` (default
profiles/retrieval_loss_bench.json).

usage: python tools/bench_retrieval_loss.py [--iters 5] [--rounds 3] [--warmup 2] [--dtype f16] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vidil_amd.blip_retrieval import BLIP_Retrieval, BLIP_Retrieval_Video  # noqa: E402
from vidil_amd.packing import set_compute_dtype  # noqa: E402
from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dtype", default="f16")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_loss_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_retrieval_loss: needs a GPU (a CPU run measures nothing)")
dev = "cuda"


def bench(name, cls, size, B, frames):
    torch.manual_seed(0)
    model = cls(image_size=size, vit="base", tokenizer=SyntheticBertTokenizer(), momentum_state=True).eval().to(dev)
    set_compute_dtype(args.dtype, model)
    rng = np.random.default_rng(0)
    shape = (B, 3, size, size) if frames == 1 else (B, frames, 3, size, size)
    x = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(dev)
    caps = [" ".join(f"w{w}" for w in rng.integers(1000, 30000, size=int(k))) for k in rng.integers(6, 24, size=B)]
    idx = torch.arange(B)

    def call(i):
        if frames == 1:
            return model(x, caps, alpha=0.4, idx=idx + i * B, seed=i)
        return model(x, caps, 0.4, idx + i * B, seed=i)

    for i in range(args.warmup):
        losses = call(i)
    times = []
    for r in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(args.iters):
            losses = call(args.warmup + r * args.iters + i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / args.iters)
    med = statistics.median(times)
    tokens = frames * ((size // 16) ** 2 + 1)
    return dict(model=name, image_size=size, frames=frames, B=B, keys_per_unit=tokens, dtype=args.dtype, weights="random-init",
                queue=model.queue_size, iters=args.iters, rounds=args.rounds, seconds_per_call=round(med, 4),
                seconds_per_call_min_max=[round(min(times), 4), round(max(times), 4)], pairs_per_s=round(B / med, 1),
                loss_ita=float(losses[0]), loss_itm=float(losses[1]), ptr_queue=int(model.ptr_queue))


commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
box = dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__)
runs = []
for spec in (("BLIP_Retrieval", BLIP_Retrieval, 384, 32, 1), ("BLIP_Retrieval_Video", BLIP_Retrieval_Video, 224, 16, 8)):
    runs.append(bench(*spec))
    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
result = dict(bench="retrieval_loss", runs=runs, box=box, commit=commit or "unknown")
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
