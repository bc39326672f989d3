"""vidil_amd.sentence.SentenceEncoder on the GPU against the float64 restatement of tests/sentence_cases.py: embeddings, the
rankings the three consumers take from them, bit-identity across batches, the full-size model once, and the consumers end to end."""
import json

import pytest
import torch

import sentence_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
# Every embedding within FACTOR x E32 (L2) of the float64 one, E32 = the float32-vs-float64 L2 error of the restatement itself:
# 8 for operands carried to 2^-21 instead of 2^-24 (include/vidil_hip.h, arith = 1), times 4 of margin for summation order.
FACTOR = 32


def _encoder(cfg, sd):
    from vidil_amd.sentence import SentenceConfig, SentenceEncoder
    from vidil_amd.tokenizer import SyntheticSentenceTokenizer

    m = SentenceEncoder(SentenceConfig(**cfg), tokenizer=SyntheticSentenceTokenizer(vocab_size=cfg["vocab_size"]))
    return sc.load_into(m, sd).eval().to(DEV)


@pytest.fixture(scope="module")
def small():
    sd, sup, qry, es, eq = sc.small()
    m = _encoder(sc.SMALL, sd)
    return dict(sd=sd, sup=sup, qry=qry, es=es, eq=eq, model=m, gs=m.encode([sc.words(x) for x in sup]), gq=m.encode([sc.words(x) for x in qry]))


def _e32(sd, cfg, id_lists, e64):
    return (sc.embed(sd, cfg, id_lists, torch.float32).double() - e64).norm(dim=1).max().item()


def test_small_model_embeddings_vs_float64(small):
    e32 = max(_e32(small["sd"], sc.SMALL, small["sup"], small["es"]), _e32(small["sd"], sc.SMALL, small["qry"], small["eq"]))
    assert small["gs"].shape == (48, 128) and small["gs"].dtype == torch.float32 and small["gs"].is_cuda
    d = torch.cat([(small["gs"].cpu().double() - small["es"]).norm(dim=1), (small["gq"].cpu().double() - small["eq"]).norm(dim=1)])
    print(f"small model, 64 sentences: worst L2 distance to the float64 embedding {d.max().item():.2e} = {d.max().item() / e32:.1f} x E32 "
          f"(E32 {e32:.2e}; asserted <= {FACTOR} x E32)")
    assert d.max().item() <= FACTOR * e32


def test_rankings_equal_the_reference(small):
    from vidil_amd.prompts import select_from_support_set
    from vidil_amd.sentence import closest, cos_sim

    cos = cos_sim(small["gq"], small["gs"])
    assert cos.shape == (16, 48) and (cos.cpu().double() - small["eq"] @ small["es"].t()).abs().max().item() < 1e-5
    for n in (1, 5):
        want, _ = sc.ranking(small["eq"], small["es"], n)
        vals, idx = closest(small["gq"], small["gs"], n)
        assert idx.dtype == torch.int32 and idx.cpu().tolist() == want, n
        assert torch.equal(vals, torch.gather(cos, 1, idx.long()))
    # a tie: value descending, INDEX ASCENDING
    twice = torch.cat([small["gs"][:6], small["gs"][2:3], small["gs"][6:]])            # candidate 6 repeats candidate 2
    _, idx = closest(small["gs"][2:3], twice, 3)
    assert idx.cpu().tolist()[0][:2] == [2, 6]
    # the selection of the prompt generator: the same five, highest last
    examples = [f"Question: {sc.words(x)}\nAnswer: a{i}" for i, x in enumerate(small["sup"])]
    want5, _ = sc.ranking(small["eq"], small["es"], 5)
    queries = [f"Frame Captions: First, x.\nQuestion: {sc.words(x)}\nAnswer:" for x in small["qry"]]
    got = select_from_support_set(small["model"], small["gs"], examples, queries, N=5)
    assert got == [[examples[j] for j in reversed(row)] for row in want5]
    assert select_from_support_set(small["model"], small["gs"], examples, queries[3], N=5) == got[3]


def test_embedding_bits_do_not_depend_on_the_batch(small):
    m = small["model"]
    ids = sc.sentences([33, 40, 64, 47, 50, 64, 35, 61, 34, 59, 48, 33, 63, 52, 41, 36, 44, 57, 39, 62], 21)       # all pad to 64 tokens
    whole = m.encode_ids(ids, batch_size=32)
    for bs in (1, 3, 7):
        assert torch.equal(m.encode_ids(ids, batch_size=bs).view(torch.int32), whole.view(torch.int32)), bs
    other = sc.sentences([64, 64, 38], 22)
    mixed = m.encode_ids([other[0], ids[1], other[1], ids[4], other[2]], batch_size=32)
    assert torch.equal(mixed[[1, 3]].view(torch.int32), whole[[1, 4]].view(torch.int32))
    # input order is kept whatever the length sort does
    short = sc.sentences([3, 20, 5], 23)
    both = m.encode_ids([short[0], ids[2], short[1], short[2]], batch_size=2)
    assert torch.equal(both[1].view(torch.int32), whole[2].view(torch.int32))
    assert torch.equal(both[[0, 2, 3]].view(torch.int32), m.encode_ids(short, batch_size=32).view(torch.int32))      # (all pad to 32)


def test_full_size_model_once():
    sd = sc.make_state(sc.FULL, 2)
    ids = sc.sentences(sc.FULL_LENS, 31, vocab=30527)
    e64 = sc.embed(sd, sc.FULL, ids)
    e32 = _e32(sd, sc.FULL, ids, e64)
    m = _encoder(sc.FULL, sd)
    got = m.encode([sc.words(x) for x in ids], batch_size=2)
    d = (got.cpu().double() - e64).norm(dim=1)
    print(f"full-size model, sentences of {sc.FULL_LENS} tokens: L2 distances to float64 {[f'{x:.2e}' for x in d.tolist()]} = "
          f"{d.max().item() / e32:.1f} x E32 (E32 {e32:.2e}; asserted <= {FACTOR} x E32)")
    assert got.shape == (3, 768) and d.max().item() <= FACTOR * e32


def test_consumers_end_to_end(small):
    from vidil_amd.prompts import in_context_selection_prompt_lines
    from vidil_amd.video_qa import map_answers

    m, sup, qry = small["model"], small["sup"], small["qry"]
    answers = [sc.words(x) for x in sup]
    top1, _ = sc.ranking(small["eq"], small["es"], 1)
    result = [{"question_id": 100 + i, "answer": sc.words(x)} for i, x in enumerate(qry)]
    assert map_answers(result, answers, m) == [{"question_id": 100 + i, "answer": answers[row[0]]} for i, row in enumerate(top1)]
    # the prompt generator, qa task, compared by the question line
    frames = [{k: [f"{k[:3]}{(i + j) % 3}" for j in range(3)] for k in ("objects", "attributes", "scenes", "verbs")} for i in range(8)]
    vt = {f"v{i}": {"frame_tokens": frames, "caption": "c"} for i in range(4)}
    caps = {f"v{i}": [f"cap {i} {j}." for j in range(3)] for i in range(4)}
    qa = {f"v{i}": [dict(question=sc.words(qry[4 * i + j]), answer="a") for j in range(4)] for i in range(4)}
    examples = [f"Frame Captions: First, s.\nQuestion: {sc.words(x)}\nAnswer: a{i}" for i, x in enumerate(sup)]
    cfg = dict(topk=4, visual_token_aggregation_version="v2", prompt_temporal_template="temporal_natural", prompt_task="qa",
               add_objects=True, add_events=False, add_attributes=True, add_scenes=False, add_frame_captions=True, add_ASR=False,
               add_original_caption=False, add_answer=False, caption_all_video=True, request_body=dict(prompt="", max_tokens=8))
    lines, idx = in_context_selection_prompt_lines(vt, caps, {}, 3, "INSTRUCTION", examples, cfg, qa, None, comparing_target="question", model=m)
    want3, _ = sc.ranking(small["eq"], small["es"], 3)
    assert len(lines) == 16 and idx == {4 * i + j: (f"v{i}", j) for i in range(4) for j in range(4)}
    for n, line in enumerate(lines):
        prefix = "\n\n".join(["INSTRUCTION"] + [examples[j] for j in reversed(want3[n])]) + "\n\n"
        prompt = json.loads(line)["prompt"]
        assert prompt.startswith(prefix + "Objects: ") and prompt.endswith(f"Question: {sc.words(qry[n])}\nAnswer:"), n


@pytest.mark.parametrize("planes", [3, 2])
def test_layernorm_of_128_columns_vs_float64(planes):
    """The small model's width: vidil_layernorm's D = 128 form (half a wave holds the row), f32 rows and [hi | lo | hi] rows."""
    from vidil_amd import kernels as K

    g = torch.Generator().manual_seed(5)
    M = 37                                                              # not a multiple of the 4 rows of a workgroup
    x = (torch.randn(M, 128, generator=g) * 3 + 1).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(128, generator=g)).to(DEV), (0.1 * torch.randn(128, generator=g)).to(DEV)
    out32 = torch.zeros(M + 1, 128, device=DEV)
    out3 = torch.zeros(M + 1, 384, dtype=torch.float16, device=DEV)
    K.layernorm(x, gamma, beta, 1e-5, M=M, D=128, out16=out3, out32=out32, split3=True, planes=planes)
    ref = torch.nn.functional.layer_norm(x.double().cpu(), (128,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    assert (out32[:M].cpu().double() - ref).abs().max().item() < 2e-6 and not out32[M].any() and not out3[M].any()
    hi, lo = out3[:M, :128].float(), out3[:M, 128:256].float()
    assert torch.equal(hi, out32[:M].half().float()) and ((hi + lo).cpu().double() - ref).abs().max().item() < 5e-6
    assert torch.equal(out3[:M, 256:], out3[:M, :128]) if planes == 3 else not out3[:M, 256:].any()
