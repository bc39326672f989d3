"""Developer benchmark: the backward forms of the GEMM (dX = dY · W: ``kernels.gemm_grad_input``; dW = dY^T · X:
``kernels.gemm_grad_weight``) in bf16 against two baselines on the same 16-bit operands, measured in the same run:

  torch     ``dy @ w`` / ``dy.t() @ x`` (16-bit result: torch's own kernels)
  nt        the existing forward kernel C = A · W^T fed with ``.t().contiguous()`` copies, the copies counted in the time

Shapes: the ViT-B backward at B = 32, 224^2 (M = 6,304 rows; four (Nout, Kin) pairs), an LM-head-like product and the
projection heads' shape.  The three are timed alternately, ``--rounds`` rounds of ``--iters`` calls each between two HIP events
after a warm-up; the median round is reported with the spread.  FLOP/s of the new form against the 2.5 PFLOP/s 16-bit peak is a
kernel figure only.  Recorded, not asserted: one JSON line, also written to ``--out`` (default profiles/gemm_grad_bench.json).

usage: python tools/bench_gemm_grad.py [--iters 20] [--rounds 5] [--commit ID] [--out FILE]"""
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
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_grad_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_gemm_grad: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
PEAK_16 = 2.5e15
SHAPES = [("vit_qkv", 6304, 2304, 768), ("vit_proj", 6304, 768, 768), ("vit_fc1", 6304, 3072, 768), ("vit_fc2", 6304, 768, 3072),
          ("lm_head_like", 1024, 30528, 768), ("heads", 96, 256, 768)]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, out                              # microseconds per call


def stats(ts):
    return dict(median_us=round(statistics.median(ts), 1), min_us=round(min(ts), 1), max_us=round(max(ts), 1))


def bench(name, M, Nout, Kin):
    g = torch.Generator(device="cpu").manual_seed(M + Nout)
    dy = torch.randn(M, Nout, generator=g).to(torch.bfloat16).to(dev)
    x = torch.randn(M, Kin, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(Nout, Kin, generator=g) * 0.05).to(torch.bfloat16).to(dev)
    runs = {}
    for form in ("grad_input", "grad_weight"):
        if form == "grad_input":
            ws = torch.empty(max(1, K.gemm_grad_ws_bytes(K.EPI_GRAD_IN, M, Kin, Nout)), dtype=torch.uint8, device=dev)
            out = torch.empty((M, Kin), dtype=torch.float32, device=dev)
            new = lambda: K.gemm_grad_input(dy, w, out=out, workspace=ws)
            ref = lambda: dy @ w
            nt_ok = Nout % 64 == 0                                             # the forward kernel's K rule
            nt = lambda: K.gemm(dy, w.t().contiguous(), out=out)               # [M, Nout] · ([Kin, Nout])^T
            plan = K.gemm_grad_plan(K.EPI_GRAD_IN, M, Kin, Nout)
        else:
            ws = torch.empty(max(1, K.gemm_grad_ws_bytes(K.EPI_GRAD_W, M, Nout, Kin)), dtype=torch.uint8, device=dev)
            out = torch.empty((Nout, Kin), dtype=torch.float32, device=dev)
            new = lambda: K.gemm_grad_weight(dy, x, out=out, workspace=ws)
            ref = lambda: dy.t() @ x
            nt_ok = M % 64 == 0
            nt = lambda: K.gemm(dy.t().contiguous(), x.t().contiguous(), out=out)   # [Nout, M] · ([Kin, M])^T
            plan = K.gemm_grad_plan(K.EPI_GRAD_W, M, Nout, Kin)
        arms = dict(new=new, torch=ref)
        if nt_ok:
            arms["nt"] = nt
        for fn in arms.values():
            timed(fn, 3)
        ts = {k: [] for k in arms}
        for _ in range(args.rounds):                                           # alternating: the box is shared
            for k, fn in arms.items():
                ts[k].append(timed(fn, args.iters)[0])
        diff = float((new().double() - ref().double()).abs().max())
        flop = 2.0 * M * Nout * Kin
        med = statistics.median(ts["new"])
        r = dict(tile=plan[0], nsplit=plan[1], split_len=plan[2], workspace_bytes=int(ws.numel()) if plan[1] > 1 else 0,
                 new=stats(ts["new"]), torch=stats(ts["torch"]),
                 new_over_torch=round(med / statistics.median(ts["torch"]), 3),
                 new_tflops=round(flop / med / 1e6, 1), new_share_of_16bit_peak=round(flop / med * 1e6 / PEAK_16, 4),
                 max_abs_difference_to_torch_bf16_result=diff)
        if nt_ok:
            r["nt_with_transposes"] = stats(ts["nt"])
            r["new_over_nt_with_transposes"] = round(med / statistics.median(ts["nt"]), 3)
        else:
            r["nt_with_transposes"] = "not run: the forward kernel needs a contraction that is a multiple of 64"
        runs[form] = r
    return dict(shape=name, M=M, Nout=Nout, Kin=Kin, dtype="bf16", iters=args.iters, rounds=args.rounds, **runs)


commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
box = dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__)
runs = []
for s in SHAPES:
    runs.append(bench(*s))
    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
result = dict(bench="gemm_grad", runs=runs, box=box, commit=commit or "unknown")
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
