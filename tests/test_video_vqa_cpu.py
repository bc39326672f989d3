"""Video question answering, the parts that need no GPU: the annotation helpers of vidil_amd/video_qa.py, the video-major
schedule, the refusals that come before any launch, the import shim, and the fixture of tests/video_vqa_cases.py itself — that
its seeds keep the composed oracle's own decisions safe at both gates and that its video tokens matter to the result."""
import json
import os

import numpy as np
import pytest
import torch

import video_vqa_cases as C
import vqa_cases as vc
from common import GOLDEN

F16_GATE, BF16_GATE = 1.25e-3, 1e-2        # test_models_gpu.PLAIN_F16_REL, test_vqa_gpu.PLAIN_BF16_REL


def test_pre_question_annotations_and_accuracy(tmp_path):
    from vidil_amd import video_qa as VQ

    assert VQ.pre_question('What is "the man" (left) doing?  ') == "what is the man left doing?"
    assert VQ.pre_question("A.B!C*D#E:F;G~H") == "abcdefgh"                       # removed, not blanked (data/utils.py:79-83)
    assert VQ.pre_question("who  is  it") == "who  is  it"                        # inner blanks stay (unlike pre_caption)
    long_q = " ".join(f"w{i}" for i in range(60))
    assert VQ.pre_question(long_q) == " ".join(f"w{i}" for i in range(50))
    assert VQ.pre_question(long_q, max_ques_words=3) == "w0 w1 w2"
    rows = [{"video_id": "video7010", "question": "What is a man doing?", "answer": "cook"},
            {"video_id": "video7010", "question": "Who is TALKING.", "answer": "man"},
            {"video_id": "video7011", "question": "what is shown", "answer": "car", "extra": 1}]
    path = tmp_path / "qa.jsonl"
    path.write_text("\n".join(json.dumps(r) for r in rows) + "\n")
    ann = VQ.load_qa_annotations(str(path))
    assert [a["question_id"] for a in ann] == [0, 1, 2]
    assert [a["video_id"] for a in ann] == ["video7010", "video7010", "video7011"]
    assert [a["question"] for a in ann] == ["what is a man doing?", "who is talking", "what is shown"]
    assert [a["answer"] for a in ann] == ["cook", "man", "car"]
    result = [{"question_id": 2, "answer": "car"}, {"question_id": 0, "answer": "cooking"}, {"question_id": 7, "answer": "x"}]
    assert VQ.accuracy(result, ann) == 0.5                                        # ids 0 and 2 are in both; 1 and 7 are not
    assert VQ.accuracy([{"question_id": i, "answer": a["answer"]} for i, a in enumerate(ann)], ann) == 1.0
    with pytest.raises(ValueError, match="share no question_id"):
        VQ.accuracy([{"question_id": 9, "answer": "x"}], ann)


def test_video_major_order_group_table_and_inverse():
    from vidil_amd.blip_vqa import video_major_order

    rng = np.random.default_rng(3)
    cases = [(C.VIDEO_OF_QUESTION, 3), ([1, 3, 1, 0, 1, 3, 1], 4), ([2, 2, 2], 5), ([0], 1), (list(range(6)), 6)]
    cases += [(rng.integers(0, 9, size=40).tolist(), 9)]
    for voq, V in cases:
        s = video_major_order(torch.tensor(voq), V)
        order, inverse, gs = C.video_major(voq, V)
        assert s["order"].dtype == torch.int64 and s["group_start"].dtype == torch.int32
        assert np.array_equal(s["order"].numpy(), order) and np.array_equal(s["inverse"].numpy(), inverse)
        assert np.array_equal(s["group_start"].numpy(), gs) and s["max_group"] == int(np.diff(gs).max())
        v = np.asarray(voq)
        assert (np.diff(v[order]) >= 0).all()                                     # video-major
        for j in range(V):                                                        # a group holds its video's questions, in caller order
            mine = order[gs[j]:gs[j + 1]]
            assert np.array_equal(mine, np.flatnonzero(v == j))
        assert np.array_equal(order[inverse], np.arange(len(voq)))                # sorted[inverse] is the caller's order
    s = video_major_order([1, 3, 1, 0, 1, 3, 1], 4)
    assert s["group_start"].tolist() == [0, 1, 5, 5, 7] and s["max_group"] == 4   # video 2: an empty group
    assert video_major_order(C.VIDEO_OF_QUESTION, 3)["group_start"].tolist() == [0, 1, 5, 7]
    for bad in ([0, 3], [-1, 0]):
        with pytest.raises(ValueError, match="video_of_question"):
            video_major_order(bad, 3)


@pytest.fixture(scope="module")
def cpu_model():
    from vidil_amd.blip_vqa import BLIP_Video_VQA
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    return BLIP_Video_VQA(image_size=32, vit="base", tokenizer=SyntheticBertTokenizer())


def test_shim_exports_and_state_dict_keys(cpu_model):
    from vidil_amd import blip_vqa as mod
    from models.blip_vqa import BLIP_VQA, BLIP_Video_VQA, blip_vqa, blip_vqa_video  # noqa: F401  (the reference's import path)

    assert BLIP_Video_VQA is mod.BLIP_Video_VQA and blip_vqa_video is mod.blip_vqa_video and issubclass(BLIP_Video_VQA, BLIP_VQA)
    with open(os.path.join(GOLDEN, "blip_vqa_keys.json")) as f:
        ref_keys = set(json.load(f))          # the reference's two classes have the same members (models/blip_vqa.py:185-193)
    mine = set(cpu_model.state_dict().keys())
    assert {k for k in mine if "pos_embed" not in k} == {k for k in ref_keys if "pos_embed" not in k}
    assert mine == ref_keys


def test_token_bound_is_16384_and_is_refused_before_any_launch(cpu_model):
    from vidil_amd.blip_vqa import MAX_VIDEO_TOKENS

    assert MAX_VIDEO_TOKENS == 16384
    cpu_model._require_video_tokens(16384)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model._require_video_tokens(16385)
    # image_size 32: 5 tokens per frame; 3,277 frames are 16,385 tokens — refused on a CPU tensor, so before any launch
    frames = torch.zeros(1, 1, 3, 32, 32).expand(1, 3277, 3, 32, 32)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model(frames, ["w200"], ["w300"], train=False, inference="rank", k_test=1)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model.video_tokens_u8(torch.zeros(1, 1, 32, 32, 3, dtype=torch.uint8).expand(1, 3277, 32, 32, 3))
    # 8 x 197 = 1,576 tokens pass the video bound where BLIP_VQA's image bound refuses them; BLIP_VQA's own message is unchanged
    with pytest.raises(ValueError, match="1576 image tokens"):
        cpu_model._require_image_tokens(1576)
    cpu_model._require_video_tokens(1576)
    with pytest.raises(ValueError, match="questions for 2 videos"):
        cpu_model(torch.zeros(2, 2, 3, 32, 32), ["w200"], ["w300"], train=False, inference="rank", k_test=1)


def test_evaluation_checks_its_arguments_before_any_launch(cpu_model):
    from vidil_amd import video_qa as VQ

    video = torch.zeros(2, 2, 3, 32, 32)
    kw = dict(answer_list=["w300", "w301"], k_test=2)
    with pytest.raises(ValueError, match="k_test=3"):
        VQ.evaluation(cpu_model, video, ["w200"], [0], [0], answer_list=["w300", "w301"], k_test=3)
    with pytest.raises(ValueError, match="2 questions, 2 question_ids and 1 entries"):
        VQ.evaluation(cpu_model, video, ["w200", "w201"], [0, 1], [0], **kw)
    with pytest.raises(ValueError, match="2 questions, 1 question_ids"):
        VQ.evaluation(cpu_model, video, ["w200", "w201"], [0], [0, 1], **kw)
    with pytest.raises(ValueError, match="inference"):
        VQ.evaluation(cpu_model, video, ["w200"], [0], [0], inference="sample", **kw)
    with pytest.raises(ValueError, match="video_representation"):
        VQ.evaluation(cpu_model, video, ["w200"], [0], [0], video_representation="mean_frame", **kw)
    with pytest.raises(ValueError, match="answer_list"):
        VQ.evaluation(cpu_model, video, ["w200"], [0], [0])


def test_parity_and_fp8_are_refused(cpu_model):
    from vidil_amd import packing

    cpu_model._require_plain()
    with pytest.raises(ValueError, match="parity"):
        packing.set_parity_mode(True, cpu_model)
    with pytest.raises(ValueError, match="fp8"):
        packing.set_compute_dtype("fp8", cpu_model)


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_seeds_keep_the_oracles_decisions_safe(case):
    """The near-tie rule of vqa_cases.excluded on this reference: no question is excluded at the f16 gate and at most one of
    the seven at the bf16 gate (SEEDS were searched on the CPU until this held)."""
    ref = C.reference(case)
    N, T = C.CASES[case]
    assert ref["question_states"].shape == (C.Q, 12, C.WIDTH) and C.tokens(case).shape == (C.B, N * T, C.WIDTH)
    assert C.question_ids(case)[1].sum(1).tolist() == C.QUESTION_TOKENS and max(C.QUESTION_TOKENS) == 12 and min(C.QUESTION_TOKENS) == 3
    assert np.bincount(C.VIDEO_OF_QUESTION).tolist() == [1, 4, 2]
    assert int(C.excluded(case, F16_GATE).sum()) == 0
    assert int(C.excluded(case, BF16_GATE).sum()) <= 1
    tok = C.tokens(case)
    assert torch.equal(tok.bfloat16().float(), tok) and torch.equal(tok.half().float(), tok)     # exact in both 16-bit types


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_the_oracle_tells_videos_and_tail_keys_apart(case):
    """What the GPU tests could not see, they could not check: on the oracle, a question answered from the NEXT video, or from
    its own video without the last 2 keys (case c: what lies past the last whole 32-key tile; case a: a quarter of the 8 keys
    past 768), moves its states by more than the widest gate (the wrong video: by more than four times that)."""
    ref = C.reference(case)
    sd_e, _ = vc.states()
    q_ids, q_mask = C.question_ids(case)
    qs = ref["question_states"]
    bound = BF16_GATE * max(1.0, qs.abs().max().item())
    with torch.no_grad():
        wrong = C.tokens(case)[(torch.tensor(C.VIDEO_OF_QUESTION) + 1) % C.B]
        short = C.tokens(case)[torch.tensor(C.VIDEO_OF_QUESTION)][:, :-2]
        d_wrong = (vc.stack(sd_e, "text_encoder.", q_ids, q_mask, wrong, None, False) - qs).abs().amax((1, 2))
        d_short = (vc.stack(sd_e, "text_encoder.", q_ids, q_mask, short, None, False) - qs).abs().amax((1, 2))
    assert d_wrong.min().item() > 4.0 * bound and d_short.min().item() > bound, (d_wrong.min().item(), d_short.min().item(), bound)
