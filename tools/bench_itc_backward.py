"""Developer benchmark: forward + backward of the two-direction soft-target contrastive (ITC) loss at D = 256 and a queue of
57,600, B = 64 and B = 256, written two ways on the same inputs:

  fused         ``losses.itc_loss(...).backward()``: the paired softmax-statistics form of the scan forward, the gradient form
                (vidil_scan_topk with topk == VIDIL_SCAN_FORM_GRAD) backward; no [B, B + 57,600] matrix either way.
  materialised  torch: matmul of the student rows against the same key buffers (batch rows in front of the queue),
                ``log_softmax`` of the student and ``softmax`` of the momentum similarities, autograd backward.

Both return the loss and the gradients with respect to the two student features and the temperature.  The two are timed
alternately, ``--rounds`` rounds of ``--iters`` calls each between two HIP events after a warm-up; the median round is reported
with the spread.  Also recorded: the peak of ``torch.cuda.max_memory_allocated`` over a call of either path (above what the
inputs hold), and the gradient kernels alone (both launches of one direction) with their achieved FLOP/s from
2·(2P)·NC·D + 2·P·NC·D — a kernel figure against the 157.3 TFLOP/s f32-matrix peak, not a figure of the loss.
Recorded, not asserted: one JSON line, also written to ``--out`` (default profiles/itc_backward_bench.json).

usage: python tools/bench_itc_backward.py [--batches 64,256] [--iters 50] [--rounds 5] [--commit ID] [--out FILE]"""
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

from vidil_amd import kernels as K, losses  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,256")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "itc_backward_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_itc_backward: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
D, Q, HEAD, TEMP, ALPHA = 256, 57600, losses.QUEUE_HEAD, 0.07, 0.4
PEAK_F32_MATRIX = 157.3e12


def unit(rng, n):
    x = rng.standard_normal((n, D)).astype(np.float32)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(dev)


def materialised_direction(a, a_m, store, B, temp):
    keys = (store[:B], store[HEAD:])
    with torch.no_grad():
        m = torch.cat([a_m @ k.t() for k in keys], 1) / temp
        target = ALPHA * torch.softmax(m, 1)
        target[:, :B] += (1.0 - ALPHA) * torch.eye(B, device=dev)
    s = torch.cat([a @ k.t() for k in keys], 1) / temp                         # [B, B + Q]
    return -(torch.log_softmax(s, 1) * target).sum(1).mean()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, out                              # microseconds per call


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def bench(B):
    rng = np.random.default_rng(B)
    img, txt, img_m, txt_m = (unit(rng, B) for _ in range(4))
    image_store, text_store = (torch.zeros((HEAD + Q, D), dtype=torch.float32, device=dev) for _ in range(2))
    image_store[:B], image_store[HEAD:] = img_m, unit(rng, Q)
    text_store[:B], text_store[HEAD:] = txt_m, unit(rng, Q)

    def leaves():
        return (img.clone().requires_grad_(True), txt.clone().requires_grad_(True),
                torch.tensor(TEMP, dtype=torch.float32, device=dev, requires_grad=True))

    def fused():
        a, b, t = leaves()
        loss = losses.itc_loss(a, b, img_m, txt_m, image_store, text_store, t, ALPHA, Q)
        return (loss.detach(),) + torch.autograd.grad(loss, (a, b, t))

    def mat():
        a, b, t = leaves()
        loss = (materialised_direction(a, img_m, text_store, B, t) + materialised_direction(b, txt_m, image_store, B, t)) / 2
        return (loss.detach(),) + torch.autograd.grad(loss, (a, b, t))

    for fn in (fused, mat):
        timed(fn, 3)
    tf, tm = [], []
    for _ in range(args.rounds):                                               # alternating: the box is shared
        t, of = timed(fused, args.iters)
        tf.append(t)
        t, om = timed(mat, args.iters)
        tm.append(t)
    med_f, med_m = statistics.median(tf), statistics.median(tm)
    peak_f, peak_m = peak_bytes(fused), peak_bytes(mat)

    # the gradient form alone: both launches of one direction, workspace allocated once
    q, q_m = img / TEMP, img_m / TEMP
    st, _ = K.scan_softmax_stats(q, q_m, text_store, [0, HEAD], [B, Q])
    lse = torch.logsumexp(st[..., 0] + torch.log(st[..., 1]), 1)
    lse_m = torch.logsumexp(st[..., 2] + torch.log(st[..., 3]), 1)
    ones = torch.ones_like(lse)
    ws = torch.empty(K.scan_topk_ws_bytes(2 * B, HEAD + Q, K.SCAN_FORM_GRAD), dtype=torch.uint8, device=dev)
    kernel = lambda: K.scan_softmax_grad(q, q_m, text_store, [0, HEAD], [B, Q], lse, lse_m, ones, ALPHA * ones, workspace=ws)
    timed(kernel, 3)
    tk = [timed(kernel, args.iters)[0] for _ in range(args.rounds)]
    med_k = statistics.median(tk)
    flop = 2 * (2 * B) * (B + Q) * D + 2 * B * (B + Q) * D
    diff = [float((x.double() - y.double()).abs().max()) for x, y in zip(of, om)]
    return dict(B=B, D=D, queue=Q, temp=TEMP, alpha=ALPHA, iters=args.iters, rounds=args.rounds,
                fused_us=round(med_f, 1), fused_us_min_max=[round(min(tf), 1), round(max(tf), 1)],
                materialised_us=round(med_m, 1), materialised_us_min_max=[round(min(tm), 1), round(max(tm), 1)],
                fused_over_materialised=round(med_f / med_m, 3),
                fused_peak_bytes=peak_f, materialised_peak_bytes=peak_m, one_matrix_bytes=B * (B + Q) * 4,
                grad_workspace_bytes=ws.numel(),
                grad_kernel_us=round(med_k, 1), grad_kernel_us_min_max=[round(min(tk), 1), round(max(tk), 1)],
                grad_kernel_flop=flop, grad_kernel_tflops=round(flop / med_k / 1e6, 2),
                grad_kernel_share_of_f32_matrix_peak=round(flop / med_k * 1e6 / PEAK_F32_MATRIX, 3),
                loss_fused=float(of[0]), loss_materialised=float(om[0]),
                max_difference=dict(loss=diff[0], image_feat=diff[1], text_feat=diff[2], temp=diff[3]),
                max_gradient=dict(image_feat=float(om[1].abs().max()), text_feat=float(om[2].abs().max()), temp=float(om[3].abs())))


commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
box = dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__)
runs = []
for b in (int(x) for x in args.batches.split(",")):
    runs.append(bench(b))
    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
result = dict(bench="itc_backward", runs=runs, box=box, commit=commit or "unknown")
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
