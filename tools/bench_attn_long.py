"""Developer microbenchmark: the long-key form of vidil_attention (attn_long_kernel) at the video-level ITM cross shape against
its comparator — N launches at one frame's key count over the same query rows (the same Q.K^T and P.V work, Q read and O
written N times, what a per-frame schedule would launch).

Shape: 32 units x 12 heads, 64 texts x 35 tokens per unit (2,240 query rows), f16, row-major V, kv_group = 64;
N = 8 frames of 577 keys (384^2) and of 197 keys (224^2): one launch at Nk = 4,616 / 1,576 vs 8 launches at 577 / 197.
The two are timed alternately in one process (rounds of `--reps` launches each, the median round is reported), after a warm-up
of both.  ``--comparator-lib PATH``: run the comparator through another build of the library (same ABI), e.g. the parent
commit's; default: this build (launches with Nk <= 768 dispatch as they always did).  One JSON line per shape.

usage: python tools/bench_attn_long.py [--units 32] [--texts 64] [--frames 8] [--reps 100] [--rounds 7] [--comparator-lib PATH]
                                       [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vidil_amd import _lib  # noqa: E402
from vidil_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--units", type=int, default=32)
ap.add_argument("--texts", type=int, default=64)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--comparator-lib", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_attn_long: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
H, Nq = 12, 35
U, G, N = args.units, args.texts, args.frames
Bq = U * G

cmp_lib = None
if args.comparator_lib:
    cmp_lib = ctypes.CDLL(args.comparator_lib)
    cmp_lib.vidil_attention.restype, cmp_lib.vidil_attention.argtypes = _lib.SIGNATURES["vidil_attention"]
    assert cmp_lib.vidil_abi_version() == _lib.ABI_VERSION, "comparator library of another ABI"


def short_launch(q, k, v, out, Nk):
    if cmp_lib is None:
        return K.attention(q, k, v, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Nk, NP=0, kv_group=G)
    rc = cmp_lib.vidil_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), None, None, None, 0, 0, Bq, H, Nq, Nk, Nq,
                                 Nk, 0, G, 0, 0, H * 64, 0, _lib.DT_F16, _lib.DT_F16, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


lines = []
g = torch.Generator().manual_seed(0)
q = (torch.randn(Bq, H, Nq, 64, generator=g) * 0.125).half().to(dev)
for T in (577, 197):
    Nk = N * T
    k = torch.randn(U, H, Nk, 64, generator=g).half().to(dev)
    v = torch.randn(U, H, Nk, 64, generator=g).half().to(dev)
    kf = [k[:, :, f * T:(f + 1) * T].contiguous() for f in range(N)]       # the frames as K / V batches of their own
    vf = [v[:, :, f * T:(f + 1) * T].contiguous() for f in range(N)]
    o_long = torch.zeros(Bq * Nq, H * 64, dtype=torch.float16, device=dev)
    o_short = torch.zeros_like(o_long)

    def long_fn():
        K.attention(q, k, v, o_long, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Nk, NP=0, kv_group=G)

    def short_fn():
        for f in range(N):
            short_launch(q, kf[f], vf[f], o_short, T)

    for _ in range(3):                                                      # warm both (code objects, LDS opt-in, clocks)
        long_fn()
        short_fn()
    # the long launch against fp64 on a slice (unit 0, head 0, the first query batch)
    s = q[0, 0].double().cpu() @ k[0, 0].double().cpu().t()
    ref = torch.softmax(s, -1) @ v[0, 0].double().cpu()
    err = (o_long[:Nq, :64].double().cpu() - ref).abs().max().item()
    assert err < 3e-3, err
    tl, ts = [], []
    for _ in range(args.rounds):                                            # alternate: A B A B ...
        tl.append(window(long_fn, args.reps))
        ts.append(window(short_fn, args.reps))
    flop = 4.0 * U * H * (G * Nq) * Nk * 64
    t_long, t_short = statistics.median(tl), statistics.median(ts)
    lines.append(dict(bench="attn_long", units=U, heads=H, rows_per_unit=G * Nq, frames=N, keys_per_frame=T, Nk=Nk,
                      long_us=round(t_long, 1), long_us_min=round(min(tl), 1), long_us_max=round(max(tl), 1),
                      comparator_us=round(t_short, 1), comparator_us_min=round(min(ts), 1), comparator_us_max=round(max(ts), 1),
                      comparator="%d launches at Nk=%d%s" % (N, T, " (comparator library)" if cmp_lib is not None else ""),
                      long_over_comparator=round(t_long / t_short, 4), long_tflops=round(flop / t_long / 1e6, 1),
                      max_abs_err_vs_fp64_slice=err, reps=args.reps, rounds=args.rounds))
    print(json.dumps(lines[-1]), flush=True)
    del k, v, kf, vf
if args.out:
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
