"""Developer microbenchmark of the beam kernels at 5..16 beams (csrc/beam.hip), next to the 4-beam kernels in the same run.

  selection    `logsoftmax_topk` over ``--rows`` logits rows x ``--vocab`` (10,752 x 30,524: the shape the narrow kernel's 347 us was
               taken at), whole images only (rows // nb images): nb = 4 on lsm_topk_kernel<4>, nb = 5, 8, 16 on
               lsm_topk_wide_kernel.  Every kernel reads each row once, so the figure to compare is bytes/s = rows * V * 4 / t
               against the nb = 4 line of the SAME run.
  beam_update  nb = 4 (one thread per image) and nb = 16 (one wave per image) on the same ``--images`` images, at ``--cur-len``.

``--reps`` repetitions of ``--iters`` launches between two HIP events per variant, the variants alternating inside a repetition
(other work shares the box); reported: the median over the repetitions and their min / max.  ``--captioning FILE ...`` folds the
JSON lines of tools/bench_video_captioning.py --beams N --out FILE runs into the result.  One JSON line; no threshold.

usage: python tools/bench_wide_beam.py [--rows 10752] [--vocab 30524] [--images 2688] [--out FILE] [--captioning FILE ...]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vidil_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10752)
ap.add_argument("--vocab", type=int, default=30524)
ap.add_argument("--images", type=int, default=2688)
ap.add_argument("--cur-len", type=int, default=20)
ap.add_argument("--max-len", type=int, default=30)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
ap.add_argument("--captioning", nargs="*", default=[])
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_wide_beam: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
V = args.vocab
torch.manual_seed(0)
logits = torch.randn(args.rows, V, device=dev) * 3.0
EOS = 102


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters                   # us per launch


def spread(samples):
    return dict(us=round(statistics.median(samples), 1), us_min=round(min(samples), 1), us_max=round(max(samples), 1))


# ---------------------------------------------------------------------------------------------------------- selection
sel = {}
for nb in (4, 5, 8, 16):
    B = args.rows // nb
    bs = -torch.rand(B * nb, device=dev) * 4.0
    seqs = torch.randint(1000, 30000, (B * nb, args.max_len), dtype=torch.int32, device=dev)
    out = (torch.empty((B, 2 * nb), dtype=torch.float32, device=dev), torch.empty((B, 2 * nb), dtype=torch.int32, device=dev))
    sel[nb] = dict(B=B, plain=lambda B=B, nb=nb, bs=bs, out=out: K.logsoftmax_topk(logits[:B * nb], bs, B, nb, EOS, *out),
                   penalty=lambda B=B, nb=nb, bs=bs, out=out, seqs=seqs: K.logsoftmax_topk(logits[:B * nb], bs, B, nb, EOS, *out, seqs=seqs,
                                                                                          cur_len=args.cur_len, penalty=1.3),
                   samples=dict(plain=[], penalty=[]), out=out)
for v in sel.values():                                          # warm-up: every kernel once, then a window each
    for form in ("plain", "penalty"):
        v[form]()
        timed(v[form], 3)
for _ in range(args.reps):
    for form in ("plain", "penalty"):
        for nb, v in sel.items():
            v["samples"][form].append(timed(v[form], args.iters))
selection = []
for nb, v in sel.items():
    rows = v["B"] * nb
    v["plain"]()
    torch.cuda.synchronize()
    line = dict(num_beams=nb, kernel="lsm_topk_kernel<4>" if nb <= 4 else "lsm_topk_wide_kernel", images=v["B"], rows=rows, vocab=V,
                bytes=rows * V * 4, digest=[float(v["out"][0].double().sum()), int(v["out"][1].long().sum())])
    for form in ("plain", "penalty"):
        s = spread(v["samples"][form])
        s["TB_per_s"] = round(rows * V * 4 / s["us"] / 1e6, 3)
        line[form] = s
    selection.append(line)
    print(f"selection {line}", file=sys.stderr, flush=True)
base = selection[0]["plain"]["TB_per_s"]
for line in selection:
    line["bytes_per_s_vs_nb4"] = round(line["plain"]["TB_per_s"] / base, 3)

# -------------------------------------------------------------------------------------------------------- beam_update
Bi = args.images
upd = {}
for nb in (4, 16):
    bufs = K.BeamBuffers(Bi, nb, args.max_len, dev)
    bufs.reset(torch.randint(1000, 30000, (Bi, 4), dtype=torch.int32, device=dev))
    g = torch.Generator(device=dev).manual_seed(nb)
    cs = torch.sort(-torch.rand(Bi, 2 * nb, device=dev, generator=g) * 30.0, dim=1, descending=True)[0].contiguous()
    ci = torch.randint(0, nb * V, (Bi, 2 * nb), device=dev, generator=g).to(torch.int32)      # ~1 in 30,524 is [SEP]
    upd[nb] = dict(fn=lambda bufs=bufs, cs=cs, ci=ci: K.beam_update(bufs, cs, ci, V, args.cur_len, EOS, 0), samples=[])
for v in upd.values():
    timed(v["fn"], 4)
for _ in range(args.reps):
    for v in upd.values():
        v["samples"].append(timed(v["fn"], 4 * args.iters))
update = [dict(num_beams=nb, kernel="beam_update_kernel" if nb <= 4 else "beam_update_wide_kernel", images=Bi, cur_len=args.cur_len,
               **spread(v["samples"])) for nb, v in upd.items()]
for line in update:
    print(f"beam_update {line}", file=sys.stderr, flush=True)

captioning = []
for path in args.captioning:
    with open(path) as f:
        c = json.loads(f.readline())
    captioning.append(dict(num_beams=c["num_beams"], videos=c["videos"], frames=c["frames"], dtype=c["dtype"],
                           concat_frame_videos_per_s=c["concat_frame"]["videos_per_s"], concat_frame_search_s=c["concat_frame"]["search_s"],
                           single_frame_videos_per_s=c["single_frame"]["videos_per_s"], single_frame_search_s=c["single_frame"]["search_s"]))
commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
result = dict(bench="wide_beam", reps=args.reps, iters=args.iters, timing="HIP events around iters launches; median (min, max) of reps",
              selection=selection, beam_update=update, captioning=captioning,
              box=dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__),
              commit=commit or "unknown")
print(json.dumps(result), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
