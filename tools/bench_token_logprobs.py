"""Developer microbenchmark: the teacher-forced one-pass reduction (kernels.token_logprobs) at 16,384 rows x 30,524 logits
(2.0 GB read once), beside torch.log_softmax + gather on the same buffer.  HIP events around 20 alternating launches each
after 3 warm-up launches; prints one JSON line (and writes it to the file given as the second argument)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vidil_amd import kernels as K  # noqa: E402

R, V, N = int(sys.argv[1]) if len(sys.argv) > 1 else 16384, 30524, 20
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # bytes/s: the MI355X's specified HBM3E rate, and the float4-copy rate measured on it
torch.manual_seed(0)
logits = torch.randn(R, V, device="cuda") * 4.0
labels = torch.randint(0, V, (R,), device="cuda", dtype=torch.int32)
lab64 = labels.long()[:, None]


def ours():
    return K.token_logprobs(logits, labels)


def eager():
    lp = torch.log_softmax(logits, -1)
    return lp.gather(1, lab64)[:, 0], lp.mean(1), logits.argmax(-1)


for _ in range(3):
    a, b = ours(), eager()
torch.cuda.synchronize()
assert (a[0] - b[0]).abs().max().item() < 1e-4 and torch.equal(a[2].long(), b[2])
t = {"ours": 0.0, "eager": 0.0}
for _ in range(N):                               # alternating, so both see the same machine
    for name, fn in (("ours", ours), ("eager", eager)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t[name] += e0.elapsed_time(e1) * 1e3 / N
nbytes = R * V * 4
out = dict(rows=R, V=V, bytes_read=nbytes, token_logprobs_us=round(t["ours"], 1), token_logprobs_TBps=round(nbytes / t["ours"] / 1e6, 2),
           floor_us_at_8TBps=round(nbytes / HBM_PEAK * 1e6, 1), share_of_8TBps_read=round(nbytes / HBM_PEAK * 1e6 / t["ours"], 3),
           share_of_measured_copy_rate=round(nbytes / HBM_COPY * 1e6 / t["ours"], 3),
           torch_log_softmax_gather_mean_argmax_us=round(t["eager"], 1), launches=N, warmup=3)
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
