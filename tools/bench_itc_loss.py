"""Developer benchmark: the two-direction soft-target contrastive (ITC) loss of the retrieval training forward at D = 256 and a
queue of 57,600, B = 64 and B = 256, written two ways on the same inputs:

  fused         ``kernels.scan_softmax_stats`` (vidil_scan_topk with topk == 0): the keys are read once per direction and five
                numbers per row and segment come back; the loss follows from them with a handful of [B]-sized torch ops.
  materialised  the same loss with the kernels the library had before: ``kernels.scan_scores`` writes the four [B, B + 57,600]
                matrices, torch's log_softmax / softmax / sum pass over them.

Both read the same key buffers (batch rows in front of the queue, no concatenation).  The two are timed alternately, ``--rounds``
rounds of ``--iters`` calls each between two HIP events after a warm-up; the median round is reported with the spread.
Recorded, not asserted: one JSON line, also written to ``--out`` (default profiles/itc_loss_bench.json).

usage: python tools/bench_itc_loss.py [--batches 64,256] [--iters 100] [--rounds 5] [--commit ID] [--out FILE]"""
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

from vidil_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,256")
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "itc_loss_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_itc_loss: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
D, Q, HEAD, TEMP, ALPHA = 256, 57600, 512, 0.07, 0.4


def unit(rng, n):
    x = rng.standard_normal((n, D)).astype(np.float32)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(dev)


def fused_direction(a, a_m, store, B):
    q, q_m = a / TEMP, a_m / TEMP
    st, _ = K.scan_softmax_stats(q, q_m, store, [0, HEAD], [B, Q])
    m, mw = st[..., 0].amax(1, keepdim=True), st[..., 2].amax(1, keepdim=True)
    ev, ew = torch.exp(st[..., 0] - m), torch.exp(st[..., 2] - mw)
    lse = m[:, 0] + torch.log((st[..., 1] * ev).sum(1))
    soft = (st[..., 4] * ew).sum(1) / (st[..., 3] * ew).sum(1)
    diag = K.scan_scores(q, store[:B]).diagonal()
    return (lse - ALPHA * soft - (1.0 - ALPHA) * diag).mean()


def materialised_direction(a, a_m, store, B):
    q, q_m = a / TEMP, a_m / TEMP
    s = torch.cat([K.scan_scores(q, store[:B]), K.scan_scores(q, store[HEAD:])], 1)          # [B, B + Q]
    m = torch.cat([K.scan_scores(q_m, store[:B]), K.scan_scores(q_m, store[HEAD:])], 1)
    target = ALPHA * torch.softmax(m, 1)
    target[:, :B] += (1.0 - ALPHA) * torch.eye(B, device=dev)
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


def bench(B):
    rng = np.random.default_rng(B)
    img, txt, img_m, txt_m = (unit(rng, B) for _ in range(4))
    stores = []
    for feats in (txt_m, img_m):
        store = torch.zeros((HEAD + Q, D), dtype=torch.float32, device=dev)
        store[:B], store[HEAD:] = feats, unit(rng, Q)
        stores.append(store)

    def both(direction):
        return lambda: (direction(img, img_m, stores[0], B) + direction(txt, txt_m, stores[1], B)) / 2

    fused, mat = both(fused_direction), both(materialised_direction)
    for fn in (fused, mat):
        timed(fn, 3)
    tf, tm = [], []
    for _ in range(args.rounds):                                               # alternating: the box is shared
        t, lf = timed(fused, args.iters)
        tf.append(t)
        t, lm = timed(mat, args.iters)
        tm.append(t)
    med_f, med_m = statistics.median(tf), statistics.median(tm)
    key_bytes = 2 * (B + Q) * D * 4                                            # both directions' keys, read once
    return dict(B=B, D=D, queue=Q, temp=TEMP, alpha=ALPHA, iters=args.iters, rounds=args.rounds,
                fused_us=round(med_f, 1), fused_us_min_max=[round(min(tf), 1), round(max(tf), 1)],
                materialised_us=round(med_m, 1), materialised_us_min_max=[round(min(tm), 1), round(max(tm), 1)],
                fused_over_materialised=round(med_f / med_m, 3),
                key_bytes=key_bytes, fused_key_GBps_whole_call=round(key_bytes / med_f / 1e3, 1),
                materialised_matrix_bytes=4 * B * (B + Q) * 4,
                loss_fused=float(lf), loss_materialised=float(lm), loss_difference=abs(float(lf) - float(lm)))


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
result = dict(bench="itc_loss", runs=runs, box=box, commit=commit or "unknown")
print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(result) + "\n")
