"""Developer microbenchmark: the key-split form of vidil_attention (kv_tiled = 2: attn_dsplit_kernel) at a beam step of the video
captioner against its comparator — the only route the library offered these rows before: the long-key form (attn_long_kernel)
with the ``group_start`` bound rounded up to 33, over the same Q rows on row-major K / V^T copies of the same K / V.

Shape: 64 units x 12 heads, 3 rows per unit (kv_group = 3, Nq = 1), bf16; Nk = 1,576 (8 frames x 197 tokens) and 4,616 (8 x 577).
The two are timed alternately in one process (rounds of ``--reps`` launches each, the median round is reported), after a warm-up
of both.  Also recorded: the bytes per second the new form moves (K and V once, Q and the output rows), next to the 5.5 - 5.7
TB/s the 197-key decode kernel reaches (docs/history/negative_results.md) — information, nobody has measured what this shape
can reach.  One JSON line per shape.

usage: python tools/bench_attn_decode_long.py [--units 64] [--rows 3] [--reps 100] [--rounds 7] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vidil_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--units", type=int, default=64)
ap.add_argument("--rows", type=int, default=3)
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_attn_decode_long: needs a GPU (a CPU run measures nothing)")
dev, dt = "cuda", torch.bfloat16
H, U, G = 12, args.units, args.rows
Bq = U * G


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
box = dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__)
lines = []
g = torch.Generator().manual_seed(0)
q = (torch.randn(Bq, H, 1, 64, generator=g) * 0.125).to(dt).to(dev)
gs = (torch.arange(U + 1, dtype=torch.int32) * G).to(dev)
for Nk in (1576, 4616):
    k = torch.randn(U, H, Nk, 64, generator=g).to(dt)
    v = torch.randn(U, H, Nk, 64, generator=g).to(dt)
    Tc = (Nk + 31) // 32 * 32
    k_off, v_off = K.kv_tile_offsets(Nk)
    kt = torch.zeros(U, H, Tc * 64, dtype=dt)
    vt = torch.zeros(U, H, Tc * 64, dtype=dt)
    kt[:, :, k_off] = k
    vt[:, :, v_off] = v
    NP = (Nk + 15) // 16 * 16
    v_t = torch.zeros(U, H, 64, NP, dtype=dt)
    v_t[..., K.vt_columns(Nk)] = v.transpose(-1, -2)
    kt, vt, k_rm, v_t = kt.to(dev), vt.to(dev), k.to(dev).contiguous(), v_t.to(dev)
    o_new = torch.zeros(Bq, H * 64, dtype=dt, device=dev)
    o_cmp = torch.zeros_like(o_new)

    def new_fn():
        K.attention(q, kt, vt, o_new, Bq=Bq, H=H, Nq=1, Nk=Nk, Tq_cap=1, Tk_cap=Tc, NP=0, kv_group=G, kv_tiled=2)

    def cmp_fn():
        K.attention(q, k_rm, v_t, o_cmp, Bq=Bq, H=H, Nq=1, Nk=Nk, Tq_cap=1, Tk_cap=Nk, NP=NP, group_start=gs, max_group=33)

    for _ in range(3):                                                      # warm both (code objects, LDS opt-in, clocks)
        new_fn()
        cmp_fn()
    # both against fp64 on a slice (unit 0, head 0), and against each other
    s = q[:G, 0, 0].double().cpu() @ k[0, 0].double().t()
    ref = torch.softmax(s, -1) @ v[0, 0].double()
    err_new = (o_new[:G, :64].double().cpu() - ref).abs().max().item()
    err_cmp = (o_cmp[:G, :64].double().cpu() - ref).abs().max().item()
    assert err_new < 2e-2 and err_cmp < 2e-2, (err_new, err_cmp)
    assert torch.allclose(o_new.float(), o_cmp.float(), rtol=2e-2, atol=2e-2)
    tn, tc = [], []
    for _ in range(args.rounds):                                            # alternate: A B A B ...
        tn.append(window(new_fn, args.reps))
        tc.append(window(cmp_fn, args.reps))
    t_new, t_cmp = statistics.median(tn), statistics.median(tc)
    nbytes = 2 * U * H * Nk * 64 * 2 + 2 * Bq * H * 64 * 2                  # K and V once; Q rows in, output rows out
    lines.append(dict(bench="attn_decode_long", units=U, heads=H, rows_per_unit=G, dtype="bf16", Nk=Nk,
                      key_split_us=round(t_new, 1), key_split_us_min=round(min(tn), 1), key_split_us_max=round(max(tn), 1),
                      comparator_us=round(t_cmp, 1), comparator_us_min=round(min(tc), 1), comparator_us_max=round(max(tc), 1),
                      comparator="long-key form, group_start with max_group=33, row-major K / V^T",
                      key_split_over_comparator=round(t_new / t_cmp, 4), requirement="key_split_over_comparator <= 1.03",
                      key_split_tb_per_s=round(nbytes / t_new / 1e6, 2), bytes_per_launch=nbytes,
                      max_abs_err_vs_fp64_slice=dict(key_split=err_new, comparator=err_cmp), reps=args.reps, rounds=args.rounds,
                      box=box, commit=commit or "unknown"))
    print(json.dumps(lines[-1]), flush=True)
    del k, v, kt, vt, k_rm, v_t
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
