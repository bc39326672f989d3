"""Developer benchmark of the sentence encoder (vidil_amd/sentence.py) on one MI355X.

  1. The price of the relative-position bias: vidil_attention_f32 with arith = 2 against arith = 1 on the same operands —
     Bq = 64, H = 12, Nq = Nk = 128 and 384, f32 Q | K | V read in place from one [M, 3C] matrix, [hi | lo] f16 output rows —
     alternated in one process (rounds of ``--reps`` launches each after a warm-up of every form; the median round is reported).
     ``--comparator-lib PATH`` adds arith = 1 through another build of the library (same ABI; the parent commit's) to the same
     alternation: the split-operand kernel must not have become slower for its present callers.
  2. Sentences per second of the full-size encoder (random weights from a seed, the synthetic tokenizer): 1,500 short answers
     (3 to 8 tokens) plus 6,144 predictions — the answer-mapping workload of video_qa.map_answers, cosines and argmax included —
     and 1,000 caption strings of 100 to 300 tokens.  Tokenisation is inside the timed window; each workload runs once untimed
     first (every padded length it uses), then ``--runs`` times.

usage: python tools/bench_sentence.py [--reps 200] [--rounds 7] [--runs 3] [--comparator-lib PATH] [--out profiles/sentence_bench.json]"""
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
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--comparator-lib", default="")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sentence_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_sentence: needs a GPU (a CPU run measures nothing)")
dev = "cuda"

cmp_lib = None
if args.comparator_lib:
    cmp_lib = ctypes.CDLL(args.comparator_lib)
    cmp_lib.vidil_attention_f32.restype, cmp_lib.vidil_attention_f32.argtypes = _lib.SIGNATURES["vidil_attention_f32"]
    cmp_lib.vidil_last_error.restype = ctypes.c_char_p
    assert cmp_lib.vidil_abi_version() == _lib.ABI_VERSION, "comparator library of another ABI"


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "attention": [], "encoder": []}
Bq, H = 64, 12
C = H * 64
g = torch.Generator().manual_seed(0)
for N in (128, 384):
    qkv = torch.randn(Bq * N, 3 * C, generator=g).to(dev)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    table = torch.randn(H, 2 * N - 1, generator=g).to(dev)
    outs = [torch.zeros(Bq * N, 3 * C, dtype=torch.float16, device=dev) for _ in range(3)]
    forms = {"arith1_us": lambda: K.attention_f32(q, k, v, outs[0], Bq=Bq, H=H, Nq=N, Nk=N, arith=1, planes=2),
             "arith2_us": lambda: K.attention_f32(q, k, v, outs[1], Bq=Bq, H=H, Nq=N, Nk=N, rel_bias=table, rel_off=N - 1, planes=2)}
    if cmp_lib is not None:
        a = _lib.AttnF32Args()             # (arith = 1: the library reads the struct as far as kv16, whichever build it is)
        a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), outs[2].data_ptr()
        a.ldq = a.ldk = a.ldv = a.ldo = 3 * C
        a.out_mode, a.dtype16, a.Bq, a.H, a.Nq, a.Nk, a.kv_rows, a.kv_group, a.scale, a.arith = 3, _lib.DT_F16, Bq, H, N, N, N, 1, 0.125, 1
        stream = torch.cuda.current_stream().cuda_stream

        def parent():
            rc = cmp_lib.vidil_attention_f32(ctypes.byref(a), stream)
            assert rc == 0, cmp_lib.vidil_last_error()
        forms["arith1_comparator_lib_us"] = parent
    for fn in forms.values():
        window(fn, 20)
    if cmp_lib is not None:
        assert torch.equal(outs[0], outs[2]), "arith = 1 of this build and of the comparator library differ"
    rounds = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            rounds[name].append(window(fn, args.reps))
    row = {"Bq": Bq, "H": H, "Nq": N, "Nk": N, "output": "[hi | lo] f16 rows"}
    for name, xs in rounds.items():
        row[name] = round(statistics.median(xs), 2)
        row[name.replace("_us", "_rounds_us")] = [round(x, 2) for x in xs]
    row["arith2_over_arith1"] = round(row["arith2_us"] / row["arith1_us"], 4)
    if cmp_lib is not None:
        row["arith1_over_comparator"] = round(row["arith1_us"] / row["arith1_comparator_lib_us"], 4)
    result["attention"].append(row)
    print(json.dumps(row), flush=True)

# ---------------------------------------------------------------------------------------------- sentences per second
from vidil_amd.sentence import SentenceEncoder, closest  # noqa: E402
from vidil_amd.tokenizer import SyntheticSentenceTokenizer  # noqa: E402

torch.manual_seed(0)
model = SentenceEncoder(tokenizer=SyntheticSentenceTokenizer()).eval().to(dev)


def strings(n, lo, hi, seed):
    gg = torch.Generator().manual_seed(seed)
    lens = torch.randint(lo, hi + 1, (n,), generator=gg).tolist()
    return [" ".join(f"w{int(i)}" for i in torch.randint(4, 30527, (L - 2,), generator=gg)) for L in lens]     # (L counts <s> and </s>)


answers, preds = strings(1500, 3, 8, 1), strings(6144, 3, 8, 2)
captions = strings(1000, 100, 300, 3)


def map_workload():
    a = model.encode(answers)
    p = model.encode(preds)
    return closest(p, a, 1)


def caption_workload():
    return model.encode(captions)


for name, fn, n, what in (("answer_mapping", map_workload, len(answers) + len(preds),
                           "1,500 answers + 6,144 predictions of 3..8 tokens, batch_size 32, cosines + argmax"),
                          ("captions", caption_workload, len(captions), "1,000 strings of 100..300 tokens, batch_size 32")):
    fn()
    times = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    row = {"workload": name, "shapes": what, "sentences": n, "seconds": [round(t, 4) for t in times],
           "sentences_per_second": round(n / statistics.median(times), 1)}
    result["encoder"].append(row)
    print(json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
