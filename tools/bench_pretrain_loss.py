"""Developer benchmark: the whole forward of the pretraining models on random-init full-size weights (ViT-B/16 at 224^2, embed_dim
256, queue 57,600) — ``BLIP_Pretrain`` with B = 32 and ``BLIP_Pretrain_Video`` at 8 frames with B = 16.  One call is what a
training step's forward is: one online ViT pass, the text feature, the EMA over the momentum parameters (in torch), the re-pack of
both momentum towers' 16-bit operands, the momentum features, the contrastive loss over batch + queue with the enqueue, the
matching pass over 3B pairs and the language-modelling pass.

Per model:
  * ``--warmup`` calls, then ``--iters`` calls between two HIP events, ``--rounds`` times: the median round with the spread, pairs/s;
  * for comparison, in the same rounds and alternating with it, the existing public pieces computing the same three losses
    separately on the same inputs: the loss forward of ``BLIP_Retrieval(_Video)`` plus ``BLIP_(Video_)Decoder.forward``, which
    runs the ViT a second time;
  * ``--iters`` more calls with ``timings=`` (video.phase_timer: HIP events, every phase synchronised): the median seconds per
    phase — vit, text, ema, repack, momentum, itc, itm, lm — and the share of ema + repack in their sum.

Recorded, not asserted: one JSON line, also written to ``--out`` (default profiles/pretrain_loss_bench.json).

usage: python tools/bench_pretrain_loss.py [--iters 5] [--rounds 3] [--warmup 2] [--dtype f16] [--commit ID] [--out FILE]"""
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

from vidil_amd.blip import BLIP_Decoder, BLIP_Video_Decoder  # noqa: E402
from vidil_amd.blip_pretrain import BLIP_Pretrain, BLIP_Pretrain_Video  # noqa: E402
from vidil_amd.blip_retrieval import BLIP_Retrieval, BLIP_Retrieval_Video  # noqa: E402
from vidil_amd.packing import set_compute_dtype  # noqa: E402
from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402

PHASES = ("vit", "text", "ema", "repack", "momentum", "itc", "itm", "lm")

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dtype", default="f16")
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_loss_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pretrain_loss: needs a GPU (a CPU run measures nothing)")
dev = "cuda"


def timed(calls):
    """Every call of ``calls`` (name -> function of the call number) ``--warmup`` times, then ``--rounds`` rounds in which each
    runs ``--iters`` times between two HIP events, one after the other (alternating: a drift of the box meets all of them alike)
    -> name -> (median seconds per call, [min, max], the last result)."""
    res, times = {}, {n: [] for n in calls}
    for n, call in calls.items():
        for i in range(args.warmup):
            res[n] = call(i)
    for r in range(args.rounds):
        for n, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(args.iters):
                res[n] = call(args.warmup + r * args.iters + i)
            e1.record()
            torch.cuda.synchronize()
            times[n].append(e0.elapsed_time(e1) / 1e3 / args.iters)
    return {n: (statistics.median(t), [round(min(t), 4), round(max(t), 4)], res[n]) for n, t in times.items()}


def bench(name, cls, retrieval_cls, decoder_cls, size, B, frames):
    tok = SyntheticBertTokenizer()
    rng = np.random.default_rng(0)
    shape = (B, 3, size, size) if frames == 1 else (B, frames, 3, size, size)
    x = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32)).to(dev)
    caps = [" ".join(f"w{w}" for w in rng.integers(1000, 30000, size=int(k))) for k in rng.integers(6, 24, size=B)]
    tokens = frames * ((size // 16) ** 2 + 1)
    out = dict(model=name, image_size=size, frames=frames, B=B, keys_per_unit=tokens, dtype=args.dtype, weights="random-init",
               iters=args.iters, rounds=args.rounds)

    torch.manual_seed(0)
    model = cls(image_size=size, vit="base", tokenizer=tok).eval().to(dev)
    # the same three losses from the existing public pieces, each with a ViT pass of its own
    retrieval = retrieval_cls(image_size=size, vit="base", tokenizer=tok, momentum_state=True).eval().to(dev)
    decoder = decoder_cls(image_size=size, vit="base", tokenizer=tok).eval().to(dev)
    set_compute_dtype(args.dtype, model, retrieval, decoder)
    idx = torch.arange(B)

    def separate(i):
        if frames == 1:
            ita, itm = retrieval(x, caps, alpha=0.4, idx=idx + i * B, seed=i)
        else:
            ita, itm = retrieval(x, caps, 0.4, idx + i * B, seed=i)
        return ita, itm, decoder(x, caps)

    t = timed(dict(forward=lambda i: model(x, caps, 0.4, seed=i), separate=separate))
    (med, spread, losses), (med_s, spread_s, _) = t["forward"], t["separate"]
    out.update(queue=model.queue_size, seconds_per_call=round(med, 4), seconds_per_call_min_max=spread, pairs_per_s=round(B / med, 1),
               loss_ita=float(losses[0]), loss_itm=float(losses[1]), loss_lm=float(losses[2]),
               separate_pieces=dict(what=f"{retrieval_cls.__name__} loss forward + {decoder_cls.__name__}.forward",
                                    seconds_per_call=round(med_s, 4), seconds_per_call_min_max=spread_s,
                                    pairs_per_s=round(B / med_s, 1)),
               time_vs_separate_pieces=round(med / med_s, 3))
    per_call = []
    for i in range(args.iters):
        t = {}
        model(x, caps, 0.4, seed=1000 + i, timings=t)
        per_call.append(t)
    phases = {p: round(statistics.median(t[p] for t in per_call), 5) for p in PHASES}
    total = sum(phases.values())
    out.update(phase_seconds=phases, phase_seconds_sum=round(total, 4),
               ema_repack_share=round((phases["ema"] + phases["repack"]) / total, 4), queue_ptr=int(model.queue_ptr))
    return out


commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
box = dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__)
runs = []
for spec in (("BLIP_Pretrain", BLIP_Pretrain, BLIP_Retrieval, BLIP_Decoder, 224, 32, 1),
             ("BLIP_Pretrain_Video", BLIP_Pretrain_Video, BLIP_Retrieval_Video, BLIP_Video_Decoder, 224, 16, 8)):
    runs.append(bench(*spec))
    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
result = dict(bench="pretrain_loss", runs=runs, box=box, commit=commit or "unknown")
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
