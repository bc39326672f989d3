"""Video question-answering evaluation on the HIP kernels — the reference's ``train_vqa_video.py`` (``evaluation`` :66-104) with
``data/vqa_dataset.py:88-148`` (``msrvtt_qa_dataset``) and the exact-match accuracy of ``eval_video_qa_result.py:93-111``, for a
``BLIP_Video_VQA`` (vidil_amd/blip_vqa.py).

The reference's loader yields one (video, question) pair per question, so its loop (``batch_size_test: 8``) runs the N-frame
ViT and the text encoder's K | V projection over the video's N*T keys once per QUESTION — about 24 times per video on
MSRVTT-QA.  Schedule of ``evaluation``:

  * the caller passes every video ONCE and says which video each question asks about (``video_of_question``);
  * the ViT runs once per video, batch by batch of ``videos``; the tokens of all videos stay on the device (N*T x width x 2
    bytes per video: 2.4 MB at 224^2 x 8 frames), the frames themselves are consumed batch by batch;
  * ``BLIP_Video_VQA.question_states_grouped``: the questions sorted video-major, the videos walked in blocks of
    ``videos_per_block`` (default: what fits ``video.KV_BLOCK_BYTES``), a block's cross-attention K / V projected
    once per video, the text encoder over the block's questions with one staging of a video's K / V for all of them.  Every
    block runs with the token count of the call's longest question and the call's ``max_group``: a question's bits do not
    depend on the block size, nor on the order the caller lists the questions in;
  * ``inference='rank'``: stage 1 and stage 2 of ``BLIP_VQA.rank_answer`` once per question, RANK_QUESTIONS at a time;
    ``inference='generate'``: the device beam search over the UNMASKED question states, which — as in the reference — depend
    on the longest question they were padded with: here the longest of the CALL, there the longest of a batch of 8.

World size 1; plain f16 / bf16 operands (the model refuses the parity precision mode and fp8)."""
from __future__ import annotations

import json
import re

import torch

from .video import VIT_VIDEOS, middle_frame, phase_timer  # (VIT_VIDEOS: videos per ViT pass when ``videos`` is one tensor)

#: questions per ``rank_answer`` / ``generate_answer_ids`` call of ``evaluation`` (bounds the [questions, vocabulary] f32 logits)
RANK_QUESTIONS = 1024


# ---------------------------------------------------------------------------------------------- annotations
def pre_question(question, max_ques_words=50):
    """The reference's question cleaning (data/utils.py:78-91): lower case, the punctuation . ! " ( ) * # : ; ~ REMOVED, trailing
    blanks stripped, at most ``max_ques_words`` words."""
    question = re.sub(r"([.!\"()*#:;~])", "", question.lower()).rstrip(" ")
    words = question.split(" ")
    return " ".join(words[:max_ques_words]) if len(words) > max_ques_words else question


def load_qa_annotations(jsonl):
    """One JSON object per line with ``video_id``, ``question`` and ``answer`` (data/vqa_dataset.py:115-124,145-148) -> a list
    of dicts ``video_id`` / ``question`` (= pre_question(question)) / ``answer`` / ``question_id``: the index of the line, as
    the reference assigns it."""
    out = []
    with open(jsonl, "r") as f:
        for line in f:
            if not line.strip():
                continue
            obj = json.loads(line)
            out.append({"video_id": obj["video_id"], "question": pre_question(obj["question"]), "answer": obj["answer"],
                        "question_id": len(out)})
    return out


def accuracy(result, annotations):
    """Exact-match accuracy (eval_video_qa_result.py:93-111): over the question ids present in BOTH ``result`` ([{question_id,
    answer}]) and ``annotations`` ([{question_id, answer}]), the fraction whose answers are equal strings."""
    pred = {r["question_id"]: r["answer"] for r in result}
    truth = {a["question_id"]: a["answer"] for a in annotations}
    common = [k for k in truth if k in pred]
    if not common:
        raise ValueError("accuracy: result and annotations share no question_id")
    return sum(1 for k in common if pred[k] == truth[k]) / len(common)


def map_answers(result, answer_list, encoder):
    """eval_video_qa_result.py:172-196: every GENERATED answer of ``result`` ([{question_id, answer}]) replaced by the entry of
    ``answer_list`` whose sentence embedding has the largest cosine with the answer's (``encoder``: a vidil_amd.sentence
    SentenceEncoder) — what the reference scores for ``inference='generate'``.  Returns [{question_id, answer}], ready for
    ``accuracy``.  Among equal cosines the entry of lowest index wins (numpy's argmax: the first maximum)."""
    from .sentence import closest

    result, answer_list = list(result), list(answer_list)
    if not result:
        return []
    answers = encoder.encode(answer_list, convert_to_tensor=True)
    preds = encoder.encode([r["answer"] for r in result], convert_to_tensor=True)
    _, idx = closest(preds, answers, 1)
    return [{"question_id": r["question_id"], "answer": answer_list[j]} for r, (j,) in zip(result, idx.cpu().tolist())]


# ---------------------------------------------------------------------------------------------- evaluation
def _video_batches(videos):
    if torch.is_tensor(videos):
        if videos.dim() != 5:
            raise ValueError(f"evaluation: videos must be [V,N,3,S,S] (f32) or [V,N,S,S,3] (uint8), got {tuple(videos.shape)}")
        return (videos[i:i + VIT_VIDEOS] for i in range(0, videos.shape[0], VIT_VIDEOS))
    return videos


@torch.no_grad()
def evaluation(model, videos, questions, question_ids, video_of_question, *, answer_list=None, inference="rank", k_test=64,
               video_representation="concat_frame", videos_per_block=None, timings=None, details=None, map_with=None):
    """train_vqa_video.py:66-104 for world size 1.  ``model``: a BLIP_Video_VQA on the GPU; ``videos``: f32 [V,N,3,S,S]
    (normalised) or an iterable of such batches — uint8 [b,N,S,S,3] batches take the fused preprocessing —, every video the same
    N; ``questions``: list[str] (already ``pre_question``-ed), ``question_ids`` their ids, ``video_of_question`` int [Q] the
    index of each question's video in ``videos``.  ``answer_list`` (inference='rank'): list[str], ``k_test`` of them scored in
    stage 2.  ``video_representation='single_frame'``: frame int(N/2) alone (:83-86).
    ``map_with`` (inference='generate'; a vidil_amd.sentence SentenceEncoder, with ``answer_list``): the generated answers are
    mapped onto ``answer_list`` by ``map_answers`` — the result the reference's eval_video_qa_result.py scores.
    Returns [{"question_id": int, "answer": str}, ...] in the order of ``questions`` — the reference's result format.
    ``timings`` (dict, optional): receives the seconds spent in ``vit`` / ``kv`` / ``encoder`` / ``answer``
    (video.phase_timer: HIP events, each phase synchronised).
    ``details`` (dict, optional; diagnostic output, what the tests compare — not part of the reference's interface): receives, on
    the host, ``max_ids`` int64 [Q], ``topk_ids`` i32 [Q, k_test] and ``log_probs_sum``
    f32 [Q, k_test] (rank) or ``tokens`` i32 [Q, 10] (generate)."""
    if inference not in ("generate", "rank"):
        raise ValueError(f"unknown inference {inference!r} (generate | rank)")
    if video_representation not in ("concat_frame", "single_frame"):
        raise ValueError(f"unknown video_representation {video_representation!r} (concat_frame | single_frame)")
    questions, question_ids = list(questions), [int(q) for q in question_ids]
    voq = torch.as_tensor(video_of_question).cpu().long().view(-1)
    Q = len(questions)
    if Q == 0 or len(question_ids) != Q or voq.numel() != Q:
        raise ValueError(f"evaluation: {Q} questions, {len(question_ids)} question_ids and {voq.numel()} entries of video_of_question")
    if map_with is not None and (inference != "generate" or answer_list is None):
        raise ValueError("evaluation: map_with maps GENERATED answers onto answer_list (inference='generate' and answer_list)")
    if inference == "rank":
        if answer_list is None:
            raise ValueError("evaluation: inference='rank' needs answer_list")
        answer_list = list(answer_list)
        if k_test > len(answer_list):
            raise ValueError(f"evaluation: k_test={k_test} exceeds the number of answers ({len(answer_list)})")
    model._require_plain()
    dev = next(model.text_encoder.parameters()).device
    lap = phase_timer(timings)
    ids, lens = model.tokenize_questions(questions)                       # padding='longest': Tq = the call's longest question
    t0 = lap()
    tokens, n_frames = [], None
    for batch in _video_batches(videos):
        batch = torch.as_tensor(batch)
        if batch.dim() != 5:
            raise ValueError(f"evaluation: [b,N,3,S,S] (f32) or [b,N,S,S,3] (uint8) video batches expected, got {tuple(batch.shape)}")
        if n_frames is None:
            n_frames = batch.shape[1]
        elif batch.shape[1] != n_frames:
            raise ValueError(f"evaluation: every video needs the same number of frames ({n_frames}), got {batch.shape[1]}")
        if video_representation == "single_frame":
            batch = middle_frame(batch)                                   # (train_vqa_video.py:85-86)
        batch = batch.to(dev)
        tokens.append(model.video_tokens_u8(batch) if batch.dtype == torch.uint8 else model.video_tokens(batch))
    if not tokens:
        raise ValueError("evaluation: no videos")
    n_per = [t.shape[0] for t in tokens]
    tokens = tokens[0] if len(tokens) == 1 else torch.cat(tokens, 0)
    T = model.visual_encoder.patch_embed.num_patches + 1
    Te = T * (1 if video_representation == "single_frame" else n_frames)
    V = sum(n_per) // Te
    lap("vit", t0)
    _, states16 = model.question_states_grouped(tokens, V, ids, lens, voq, videos_per_block=videos_per_block, timings=timings,
                                                f32=False)
    Tq = ids.shape[1]
    t0 = lap()
    parts = []
    if inference == "rank":
        a_ids, a_lens = model.tokenize_answers(answer_list)               # (:78-79)
        for q0 in range(0, Q, RANK_QUESTIONS):
            q1 = min(Q, q0 + RANK_QUESTIONS)
            parts.append(model.rank_answer(states16[q0 * Tq:q1 * Tq], q1 - q0, lens[q0:q1], a_ids, a_lens, k_test))
        max_ids = torch.cat([p[0] for p in parts]).cpu()
        result = [{"question_id": qid, "answer": answer_list[int(a)]} for qid, a in zip(question_ids, max_ids.tolist())]
        if details is not None:
            details.update(max_ids=max_ids, topk_ids=torch.cat([p[1] for p in parts]).cpu(),
                           log_probs_sum=torch.cat([p[2] for p in parts]).cpu())
    else:
        for q0 in range(0, Q, RANK_QUESTIONS):
            q1 = min(Q, q0 + RANK_QUESTIONS)
            parts.append(model.generate_answer_ids(states16[q0 * Tq:q1 * Tq], q1 - q0)[0])
        out_tok = torch.cat(parts).cpu()
        result = [{"question_id": qid, "answer": model.tokenizer.decode(row, skip_special_tokens=True)}
                  for qid, row in zip(question_ids, out_tok.tolist())]
        if details is not None:
            details.update(tokens=out_tok)
        if map_with is not None:
            result = map_answers(result, answer_list, map_with)
    lap("answer", t0)
    return result
