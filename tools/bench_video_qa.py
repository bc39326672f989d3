"""Developer benchmark: video question answering at full size, two schedules through the SAME model — a random-init
BLIP_Video_VQA (ViT-B/16, bf16), ``--videos`` synthetic videos of ``--frames`` frames at ``--size``^2, ``--per-video`` synthetic
questions about each (in a shuffled order), an answer list of ``--answers``, ``inference='rank'`` with ``--k-test``.

  shared     ``video_qa.evaluation``: every video passed once; the ViT and the cross K|V projection run once per video, the
             question encoder over a video's questions with one staging of its K / V, the ranking once per question.
  reference  the reference's call shape (train_vqa_video.py:81-102, ``batch_size_test: 8``): ``model(video, question, answers,
             train=False, inference='rank')`` on batches of 8 (video, question) pairs, so the ViT and the K|V projection run
             once per QUESTION; the answer candidates are tokenised once, outside the loop, as there.  ``--ref-questions K`` times the first K questions only (default: all).

Every schedule runs twice after a warm-up through the kernel forms of the timed runs: once whole between two HIP events
(``total_s``, ``questions_per_s``), once phase by phase, each phase between HIP events and synchronised (``vit_s``,
``kv_s``, ``encoder_s``, ``stage1_s``, ``stage2_s``; ``video.phase_timer`` throughout).
stage 1 is ``first_token_logprobs`` + ``topk_rows`` timed on its own; stage 2 is ``rank_answer`` minus that.  One JSON line.

usage: python tools/bench_video_qa.py [--videos 256] [--frames 8] [--size 224] [--per-video 24] [--answers 1500] [--k-test 64]
                                      [--ref-questions K] [--commit ID] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vidil_amd import kernels as K  # noqa: E402
from vidil_amd import video_qa as VQ  # noqa: E402
from vidil_amd.blip_vqa import BLIP_Video_VQA  # noqa: E402
from vidil_amd.packing import set_compute_dtype  # noqa: E402
from vidil_amd.tokenizer import SyntheticBertTokenizer  # noqa: E402
from vidil_amd.video import phase_timer, videos_per_block  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--videos", type=int, default=256)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--per-video", type=int, default=24)
ap.add_argument("--answers", type=int, default=1500)
ap.add_argument("--k-test", type=int, default=64)
ap.add_argument("--ref-questions", type=int, default=0)
ap.add_argument("--commit", default="")
ap.add_argument("--out", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_video_qa: needs a GPU (a CPU run measures nothing)")
dev = "cuda"
REF_BATCH = 8                                     # configs/train_blip_video_vqa_msrvtt.yaml: batch_size_test
torch.manual_seed(0)
model = BLIP_Video_VQA(image_size=args.size, vit="base", tokenizer=SyntheticBertTokenizer()).eval().to(dev)
set_compute_dtype("bf16", model)
rng = np.random.default_rng(0)
V, Q = args.videos, args.videos * args.per_video
voq = torch.from_numpy(rng.permutation(np.repeat(np.arange(V), args.per_video)))
questions = [" ".join(f"w{w}" for w in rng.integers(1000, 30000, size=int(n))) for n in rng.integers(4, 20, size=Q)]
firsts = rng.permutation(np.arange(1000, 30000))[:args.answers]
answers = [" ".join([f"w{f}"] + [f"w{w}" for w in rng.integers(1000, 30000, size=int(n))])
           for f, n in zip(firsts, rng.integers(0, 3, size=args.answers))]           # 1..3 words
videos = torch.randn(V, args.frames, 3, args.size, args.size, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
a_ids, a_lens = model.tokenize_answers(answers)
# the candidates tokenised ONCE, outside the loop, and handed over as an object — what the reference's loop does
# (train_vqa_video.py:76-79); a list of strings would be tokenised again by every forward call
answer_candidates = types.SimpleNamespace(input_ids=a_ids.to(dev),
                                          attention_mask=(torch.arange(a_ids.shape[1])[None, :] < a_lens[:, None]).long().to(dev))
keys = args.frames * ((args.size // 16) ** 2 + 1)


class Phases(dict):
    """with phases("name"): ... adds the HIP-event seconds of the block (video.phase_timer: synchronised at its end)."""

    def __call__(self, name):
        lap = phase_timer(self)

        class _P:
            def __enter__(self):
                self.t0 = lap()

            def __exit__(self, *exc):
                lap(name, self.t0)
        return _P()


def stage1(states16, n, lens):
    return K.topk_rows(model.first_token_logprobs(states16, n, lens, a_ids), args.k_test)


# ------------------------------------------------------------------------------------------------ the shared schedule
def shared_whole(nv=V, qsel=None):
    qsel = range(Q) if qsel is None else qsel
    return VQ.evaluation(model, videos[:nv], [questions[i] for i in qsel], list(qsel), voq[list(qsel)], answer_list=answers,
                         k_test=args.k_test)


def shared_split():
    ph = Phases()
    ids, lens = model.tokenize_questions(questions)
    with ph("vit"):
        tokens = torch.cat([model.video_tokens(videos[i:i + VQ.VIT_VIDEOS]) for i in range(0, V, VQ.VIT_VIDEOS)], 0)
    _, st = model.question_states_grouped(tokens, V, ids, lens, voq, timings=ph)
    Tq = ids.shape[1]
    for q0 in range(0, Q, VQ.RANK_QUESTIONS):
        q1 = min(Q, q0 + VQ.RANK_QUESTIONS)
        with ph("stage1"):
            stage1(st[q0 * Tq:q1 * Tq], q1 - q0, lens[q0:q1])
        with ph("rank"):
            model.rank_answer(st[q0 * Tq:q1 * Tq], q1 - q0, lens[q0:q1], a_ids, a_lens, args.k_test)
    return ph


# ------------------------------------------------------------------------------------------------ the reference's call shape
def reference_whole(n):
    out = []
    for q0 in range(0, n, REF_BATCH):
        sel = list(range(q0, min(n, q0 + REF_BATCH)))
        ids = model(videos[voq[sel].to(dev)], [questions[i] for i in sel], answer_candidates, train=False, inference="rank",
                    k_test=args.k_test)
        out.append(ids)
    return [{"question_id": i, "answer": answers[int(a)]} for i, a in enumerate(torch.cat(out).cpu().tolist())]


def reference_split(n):
    ph = Phases()
    for q0 in range(0, n, REF_BATCH):
        sel = list(range(q0, min(n, q0 + REF_BATCH)))
        b = len(sel)
        video = videos[voq[sel].to(dev)]
        ids, lens = model.tokenize_questions([questions[i] for i in sel])
        with ph("vit"):
            tokens = model.video_tokens(video)
        _, st = model.question_states_grouped(tokens, b, ids, lens, torch.arange(b), timings=ph)
        with ph("stage1"):
            stage1(st, b, lens)
        with ph("rank"):
            model.rank_answer(st, b, lens, a_ids, a_lens, args.k_test)
    return ph


def whole(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3, res


def report(total, n, ph):
    d = dict(questions=n, total_s=round(total, 3), questions_per_s=round(n / total, 1), vit_s=round(ph["vit"], 3),
             kv_s=round(ph["kv"], 3), encoder_s=round(ph["encoder"], 3), stage1_s=round(ph["stage1"], 3),
             stage2_s=round(ph["rank"] - ph["stage1"], 3))
    d["split_sum_s"] = round(sum(d[k] for k in ("vit_s", "kv_s", "encoder_s", "stage1_s", "stage2_s")), 3)
    return d


n_ref = min(Q, args.ref_questions or Q)
# warm-up: both schedules, small, through the kernel forms of the timed runs (same keys per video, same Tq range, same k_test)
first = [i for i in range(Q) if int(voq[i]) < 4]
shared_whole(4, first)
reference_whole(2 * REF_BATCH)
torch.cuda.synchronize()
print("warm-up done", file=sys.stderr, flush=True)
t_shared, res_shared = whole(shared_whole)
print(f"shared: {t_shared:.2f} s", file=sys.stderr, flush=True)
ph_shared = shared_split()
print(f"shared split: {dict(ph_shared)}", file=sys.stderr, flush=True)
t_ref, res_ref = whole(lambda: reference_whole(n_ref))
print(f"reference call shape: {t_ref:.2f} s for {n_ref} questions", file=sys.stderr, flush=True)
ph_ref = reference_split(n_ref)
same = sum(1 for a, b in zip(res_shared[:n_ref], res_ref) if a["answer"] == b["answer"]) / n_ref
commit = args.commit
if not commit:
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
prop = torch.cuda.get_device_properties(0)
line = dict(bench="video_qa_evaluation", videos=V, frames=args.frames, size=args.size, keys_per_video=keys, questions=Q,
            questions_per_video=args.per_video, answers=args.answers, k_test=args.k_test, dtype="bf16", weights="random-init",
            longest_question_tokens=int(model.tokenize_questions(questions)[0].shape[1]),
            videos_per_block=int(videos_per_block(model.text_encoder.config, keys)),
            shared=report(t_shared, Q, ph_shared), reference_call_shape=dict(batch=REF_BATCH, **report(t_ref, n_ref, ph_ref)),
            shared_over_reference_questions_per_s=round((Q / t_shared) / (n_ref / t_ref), 3), same_answers_share=round(same, 4),
            box=dict(device=prop.name, compute_units=prop.multi_processor_count, hip=torch.version.hip, torch=torch.__version__),
            commit=commit or "unknown")
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(line) + "\n")
