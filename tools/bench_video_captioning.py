"""Developer benchmark: video captioning at full size through ``video_captioning.evaluation`` — a random-init BLIP_Video_Decoder
(ViT-B/16, bf16), ``--videos`` synthetic videos of ``--frames`` frames at ``--size``^2, beam search with ``--beams`` beams,
``max_length`` 30, ``min_length`` 5.

  concat_frame   every video's N*T frame tokens as ONE encoder sequence: the decode steps' cross-attention is the key-split form
                 of vidil_attention (3 rows per video over 1,576 keys at the defaults).
  single_frame   frame int(N/2) alone through BLIP_Decoder's path (197 keys), next to it.

Each runs twice after a warm-up of the same shapes (which also captures the step graphs): once whole between two HIP events
(``total_s``, ``videos_per_s``), once phase by phase, each phase between HIP events and synchronised — ``vit_s``, ``kv_s`` (the
cross K | V projection of the blocks, timed on its own) and ``search_s`` (the searches minus that).  No threshold.  One JSON line.

usage: python tools/bench_video_captioning.py [--videos 256] [--frames 8] [--size 224] [--beams 3] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vidil_amd import video_captioning as VC  # noqa: E402
from vidil_amd.blip import BLIP_Video_Decoder  # noqa: E402
from vidil_amd.packing import set_compute_dtype  # noqa: E402
from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402
from vidil_amd.video import phase_timer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=256)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--beams", type=int, default=3)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_video_captioning: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
MAX_LENGTH, MIN_LENGTH = 30, 5
torch.manual_seed(0)
model = BLIP_Video_Decoder(image_size=args.size, vit="base", tokenizer=SyntheticBertTokenizer()).eval().to(dev)
set_compute_dtype("bf16", model)
V, N = args.videos, args.frames
videos = torch.randn(V, N, 3, args.size, args.size, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
ids = [f"video{i}" for i in range(V)]
T = (args.size // 16) ** 2 + 1


def cfg(rep):
    return dict(video_representation=rep, num_beams=args.beams, max_length=MAX_LENGTH, min_length=MIN_LENGTH)


def whole(rep):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = VC.evaluation(model, [(videos, ids)], cfg(rep))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, res


def kv_alone(rep):
    """The cross K | V projection of the run's blocks on its own (fragment tiles, as the searches' sessions hold them)."""
    Te = T * (N if rep == "concat_frame" else 1)
    per = model.videos_per_block(Te) if rep == "concat_frame" else V
    tok = torch.zeros(min(per, V) * Te, model.text_decoder.config.encoder_width, dtype=torch.bfloat16, device=dev)
    ph = {}
    lap = phase_timer(ph)
    for b0 in range(0, V, per):
        b = min(V, b0 + per) - b0
        t0 = lap()
        model.text_decoder.bert.project_cross_kv(tok[:b * Te], b, Te, tiled=True)
        lap("kv", t0)
    return ph["kv"], per


def report(rep):
    whole(rep)                                                  # warm-up: every kernel form; the second search of a shape captures
    whole(rep)                                                  # its step graphs, the timed ones replay them
    total, res = whole(rep)
    ph = {}
    VC.evaluation(model, [(videos, ids)], cfg(rep), timings=ph)
    kv, per = kv_alone(rep)
    assert len(res) == V and all(isinstance(r["caption"], str) for r in res)
    return dict(keys_per_video=T * (N if rep == "concat_frame" else 1), videos_per_block=int(per), total_s=round(total, 3),
                videos_per_s=round(V / total, 1), vit_s=round(ph["vit"], 3), kv_s=round(kv, 3), search_s=round(ph["search"] - kv, 3),
                split_sum_s=round(ph["vit"] + ph["search"], 3))


concat = report("concat_frame")
print(f"concat_frame: {concat}", file=sys.stderr, flush=True)
single = report("single_frame")
commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
line = dict(bench="video_captioning_evaluation", videos=V, frames=N, size=args.size, dtype="bf16", weights="random-init",
            num_beams=args.beams, max_length=MAX_LENGTH, min_length=MIN_LENGTH, concat_frame=concat, single_frame=single,
            box=dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__),
            commit=commit or "unknown")
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
