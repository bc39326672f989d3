"""Developer microbenchmark of the answer-ranking path of BLIP_VQA.

1. The candidate form of the one-read log-softmax kernel (kernels.candidate_logprobs) at 16,384 rows x 30,524 logits (2.0 GB
   read once) with A = 3,128 candidates (the VQAv2 answer-list size), beside ``torch.log_softmax(...).index_select(1, cand)`` on
   the same buffer in the same run: HIP events around 20 alternating launches each after 3 warm-up launches.  The kernel must
   not be slower than the torch composition (asserted).
2. No threshold: questions/s of ``BLIP_VQA.forward(train=False, inference='rank')`` at full size — 256 questions x 128
   candidates out of 3,128 answers, ViT-B/16 at 384 px (the ViT's attention kernels serve at most 768 tokens: the reference's 480 px
   default has 901), random-init weights, bf16 — with the ViT included and for the ranking
   alone, and the share of the scorer's stack rows that are padding under its 33-token block floor (med.SCORE_MIN_TOKENS).

Prints one JSON line (and writes it to the file given as the first argument).  ``--no-rank`` skips part 2."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vidil_amd import kernels as K  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
R, V, A, N = 16384, 30524, 3128, 20
HBM_PEAK = 8.0e12                                # bytes/s: the MI355X's specified HBM3E rate
torch.manual_seed(0)
logits = torch.randn(R, V, device="cuda") * 4.0
cand = torch.randperm(V, device="cuda")[:A].to(torch.int32)
cand64 = cand.long()
out = torch.empty((R, A), dtype=torch.float32, device="cuda")


def ours():
    return K.candidate_logprobs(logits, cand, out=out)


def eager():
    return torch.log_softmax(logits, -1).index_select(1, cand64)


for _ in range(3):
    a, b = ours(), eager()
torch.cuda.synchronize()
assert (a - b).abs().max().item() < 1e-4
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
res = dict(rows=R, V=V, candidates=A, bytes_read=nbytes, candidate_logprobs_us=round(t["ours"], 1),
           candidate_logprobs_TBps=round(nbytes / t["ours"] / 1e6, 2), floor_us_at_8TBps=round(nbytes / HBM_PEAK * 1e6, 1),
           share_of_8TBps_read=round(nbytes / HBM_PEAK * 1e6 / t["ours"], 3),
           torch_log_softmax_index_select_us=round(t["eager"], 1), launches=N, warmup=3)
print(json.dumps(res), flush=True)
del logits, out, a, b
torch.cuda.empty_cache()

if "--no-rank" not in sys.argv:
    from vidil_amd import med  # noqa: E402
    from vidil_amd.blip_vqa import BLIP_VQA  # noqa: E402
    from vidil_amd.packing import set_compute_dtype  # noqa: E402
    from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402

    Q, k, n_ans = 256, 128, 3128
    rng = np.random.default_rng(0)
    model = BLIP_VQA(image_size=384, vit="base", tokenizer=SyntheticBertTokenizer()).to("cuda").eval()
    set_compute_dtype("bf16", model)
    questions = [" ".join(f"w{w}" for w in rng.integers(1000, 30000, size=int(n))) for n in rng.integers(4, 20, size=Q)]
    firsts = rng.permutation(np.arange(1000, 30000))[:n_ans]
    answers = [" ".join([f"w{f}"] + [f"w{w}" for w in rng.integers(1000, 30000, size=int(n))])
               for f, n in zip(firsts, rng.integers(0, 4, size=n_ans))]            # 1..4 words: 3..6 tokens with [DEC] and [SEP]
    image = torch.randn(Q, 3, 384, 384, device="cuda")
    a_ids, a_lens = model.tokenize_answers(answers)

    def timed(fn, n=2):
        fn()                                                                         # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3 / n, r

    s_all, _ = timed(lambda: model(image, questions, answers, train=False, inference="rank", k_test=k))
    _, y16 = model.visual_encoder.forward_both(image)
    ids, lens = model.tokenize_questions(questions)
    _, st = model.question_states(y16, Q, ids, lens)
    s_rank, (_, topk_ids, _) = timed(lambda: model.rank_answer(st, Q, lens, a_ids, a_lens, k))
    sel = a_lens[topk_ids.cpu().long().view(-1)]
    T = max(med.SCORE_MIN_TOKENS, int(sel.max()))
    res.update(rank=dict(questions=Q, k_test=k, answers=n_ans, image_size=384, dtype="bf16", weights="random-init",
                         forward_s=round(s_all, 4), forward_questions_per_s=round(Q / s_all, 1), rank_answer_s=round(s_rank, 4),
                         rank_answer_questions_per_s=round(Q / s_rank, 1), stack_rows=int(Q * k * T), real_token_rows=int(sel.sum()),
                         padding_share_of_stack_rows=round(1.0 - float(sel.sum()) / (Q * k * T), 4), block_tokens=T))
print(json.dumps(res))
assert t["ours"] <= t["eager"], f"candidate_logprobs ({t['ours']:.1f} us) is slower than torch ({t['eager']:.1f} us)"
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
