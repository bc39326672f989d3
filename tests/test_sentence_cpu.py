"""The sentence encoder's host side: the float64 restatement pinned to the installed ``transformers.MPNetModel``, what the fixture of
tests/sentence_cases.py can detect, the host bias-table builder, the tokenizers, the argument contract of the relative-position-bias
attention (checked by the library before any launch) and the three consumers on a stub encoder."""
import ctypes
import json
import os
import re

import pytest
import torch

import sentence_cases as sc
from common import GOLDEN

BIAS = "encoder.relative_attention_bias.weight"


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_equals_transformers_mpnet_in_float64():
    from transformers import MPNetConfig, MPNetModel

    sd, sup, qry, _, eq = sc.small()
    cfg = MPNetConfig(**sc.SMALL, layer_norm_eps=sc.EPS, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pad_token_id=sc.PAD)
    hf = MPNetModel(cfg, add_pooling_layer=False).double().eval()
    hf.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    for batch in (qry, sup[:24]):
        ids, mask = sc.pad(batch)
        with torch.no_grad():
            want = hf(input_ids=ids, attention_mask=mask).last_hidden_state
            got = sc.hidden_states(sd, sc.SMALL, ids, mask)
        d = ((want - got) * mask[:, :, None]).abs().max().item()
        print(f"restatement vs transformers.MPNetModel, float64, {len(batch)} sentences: max|d| {d:.1e}")
        assert d <= 1e-12
    # pooled and normalised, every sentence alone and unpadded (how the reference values of the GPU tests are computed)
    assert (sc.pool(want, mask) - sc.embed(sd, sc.SMALL, sup[:24])).abs().max().item() <= 1e-12
    for T in (1, 2, 8, 9, 91, 92, 384):
        with torch.no_grad():
            b = hf.encoder.compute_position_bias(torch.zeros(1, T, 1, dtype=torch.float64))[0]
        assert torch.equal(b, sc.position_bias(sd, T)), T


@pytest.mark.parametrize("T", [1, 2, 8, 9, 91, 92, 384])
def test_host_table_is_the_toeplitz_bias(T):
    from vidil_amd.sentence import relative_bias_table

    sd = sc.small()[0]
    table, rel_off = relative_bias_table(sd[BIAS], T)
    assert table.shape == (2, 2 * T - 1) and rel_off == T - 1 and table.dtype == torch.float32
    bias = sc.position_bias(sd, T, torch.float32)
    i = torch.arange(T)
    assert torch.equal(table[:, rel_off + i[None, :] - i[:, None]], bias)
    if T > 92:      # offsets of magnitude 91 and beyond share one bucket per sign
        assert (table[:, :rel_off - 90] == table[:, :1]).all() and (table[:, rel_off + 91:] == table[:, -1:]).all()
        assert not torch.equal(table[:, 0], table[:, -1])


def test_fixture_detects_the_bias_and_separates_the_ranks():
    sd, sup, qry, es, eq = sc.small()
    zero = dict(sd)
    zero[BIAS] = torch.zeros_like(sd[BIAS])
    moved = (sc.embed(zero, sc.SMALL, qry) - eq).norm(dim=1).min().item()
    swap = dict(sd)
    swap[BIAS] = torch.cat([sd[BIAS][16:], sd[BIAS][:16]])
    moved_swap = (sc.embed(swap, sc.SMALL, qry) - eq).norm(dim=1).min().item()
    print(f"smallest L2 move of a query embedding: bias zeroed {moved:.2e}, sign halves swapped {moved_swap:.2e}")
    assert moved > 1e-2 and moved_swap > 1e-2
    s32, q32 = sc.embed(sd, sc.SMALL, sup, torch.float32), sc.embed(sd, sc.SMALL, qry, torch.float32)
    ecos = ((q32 @ s32.t()).double() - eq @ es.t()).abs().max().item()
    G = 32 * ecos
    srt = (eq @ es.t()).sort(dim=1, descending=True).values
    gap12, gap56 = (srt[:, 0] - srt[:, 1]).min().item(), (srt[:, 4] - srt[:, 5]).min().item()
    print(f"Ecos32 {ecos:.2e}, G = 32 x Ecos32 {G:.2e}; smallest top-1/top-2 gap {gap12:.2e}, smallest 5th/6th gap {gap56:.2e}")
    assert gap12 > G and gap56 > G        # the rank assertions of tests/test_sentence_gpu.py leave out no query


# ------------------------------------------------------------------------------------------------ tokenizers
def test_synthetic_sentence_tokenizer():
    from vidil_amd.tokenizer import SyntheticSentenceTokenizer

    tok = SyntheticSentenceTokenizer(vocab_size=200)
    assert (tok.bos_token_id, tok.pad_token_id, tok.eos_token_id, tok.unk_token_id) == (0, 1, 2, 3)
    assert tok("w5 W17 w199 w200 w3 zebra")["input_ids"] == [0, 5, 17, 199, 3, 3, 3, 2]
    ids = tok([" ".join(f"w{4 + i}" for i in range(20)), "w9"], truncation=True, max_length=8)["input_ids"]
    assert ids == [[0, 4, 5, 6, 7, 8, 9, 2], [0, 9, 2]]               # truncation keeps </s>
    assert tok.decode(ids[0], skip_special_tokens=True) == "w4 w5 w6 w7 w8 w9"
    x = sc.sentences([3, 9], 5)
    assert tok([sc.words(s) for s in x])["input_ids"] == x


def test_sentence_tokenizer_from_a_vocabulary_file(tmp_path, monkeypatch):
    from vidil_amd.tokenizer import init_sentence_tokenizer

    words = ["<s>", "<pad>", "</s>", "<unk>", "the", "cat", "sat", "on", "mat", "##s", "a", "dog", "run", "##ning", ".", ",", "what", "is",
             "?", "<mask>"]
    path = tmp_path / "vocab.txt"
    path.write_text("".join(w + "\n" for w in words), encoding="utf-8")
    tok = init_sentence_tokenizer(str(path))
    assert (tok.cls_token_id, tok.pad_token_id, tok.sep_token_id, tok.unk_token_id) == (0, 1, 2, 3)
    assert tok("The cats sat on a MAT, running zebra?")["input_ids"] == [0, 4, 5, 9, 6, 7, 10, 8, 15, 12, 13, 3, 18, 2]
    assert tok(["the cat", "the cat sat on the mat ."], truncation=True, max_length=5)["input_ids"] == [[0, 4, 5, 2], [0, 4, 5, 6, 2]]
    monkeypatch.setenv("VIDIL_MPNET_VOCAB", str(path))
    assert init_sentence_tokenizer()("a dog")["input_ids"] == [0, 10, 11, 2]
    with pytest.raises(FileNotFoundError):
        init_sentence_tokenizer(str(tmp_path / "missing.txt"))
    bert = tmp_path / "bert.txt"
    bert.write_text("[PAD]\n[UNK]\nthe\n", encoding="utf-8")
    with pytest.raises(RuntimeError, match="not an MPNet vocabulary"):
        init_sentence_tokenizer(str(bert))


def test_sentence_tokenizer_without_a_source_raises(tmp_path, monkeypatch):
    from vidil_amd.tokenizer import init_sentence_tokenizer

    monkeypatch.delenv("VIDIL_MPNET_VOCAB", raising=False)
    monkeypatch.setenv("HF_HOME", str(tmp_path))                        # an empty local cache
    monkeypatch.setenv("HF_HUB_CACHE", str(tmp_path / "hub"))
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    with pytest.raises(RuntimeError, match="never downloaded"):
        init_sentence_tokenizer()


def test_no_loader_without_local_files_only():
    """Neither the tokenizer module nor the encoder calls a ``from_pretrained`` that could open a connection."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "vidil_amd", "tokenizer.py")).read()
    body = src[src.index("def init_sentence_tokenizer"):]
    calls = re.findall(r"from_pretrained\(([^)]*)\)", body)
    assert calls and all("local_files_only=True" in c for c in calls), calls
    enc = open(os.path.join(root, "vidil_amd", "sentence.py")).read()
    assert "from_pretrained" not in enc and "snapshot_download" not in enc and "hf_hub_download" not in enc


def test_pretrained_with_the_stand_in_tokenizer_is_refused(tmp_path):
    from vidil_amd.sentence import sentence_encoder
    from vidil_amd.tokenizer import SyntheticSentenceTokenizer

    with pytest.raises(RuntimeError, match="real MPNet tokenizer"):
        sentence_encoder(pretrained=str(tmp_path), tokenizer=SyntheticSentenceTokenizer())


def test_checkpoint_names_load_and_strays_raise(tmp_path):
    from vidil_amd.sentence import SentenceConfig, SentenceEncoder, sentence_encoder
    from vidil_amd.tokenizer import SyntheticSentenceTokenizer

    sd = sc.small()[0]
    tok = SyntheticSentenceTokenizer(vocab_size=200, allow_pretrained=True)
    d = tmp_path / "model"
    d.mkdir()
    stored = {"0.auto_model." + k: v for k, v in sd.items()}
    stored["0.auto_model.pooler.dense.weight"] = torch.zeros(4, 4)
    stored["0.auto_model.embeddings.position_ids"] = torch.arange(514)[None]
    torch.save(stored, d / "pytorch_model.bin")
    (d / "config.json").write_text(json.dumps({"layer_norm_eps": 1e-7}))
    m = sentence_encoder(pretrained=str(d), tokenizer=tok, **sc.SMALL)
    assert m.config.layer_norm_eps == 1e-7 and m.embeddings.LayerNorm.eps == 1e-7
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items()) and set(m.state_dict()) == set(sd)
    torch.save({"mpnet." + k: v for k, v in sd.items()}, d / "pytorch_model.bin")
    SentenceEncoder(SentenceConfig(**sc.SMALL)).load_pretrained(str(d))
    torch.save({k: v for k, v in sd.items() if k != BIAS}, d / "pytorch_model.bin")
    with pytest.raises(RuntimeError, match="missing keys.*relative_attention_bias"):
        SentenceEncoder(SentenceConfig(**sc.SMALL)).load_pretrained(str(d))
    torch.save(dict(sd, stray=torch.zeros(1)), d / "pytorch_model.bin")
    with pytest.raises(RuntimeError, match="unexpected keys.*stray"):
        SentenceEncoder(SentenceConfig(**sc.SMALL)).load_pretrained(str(d))
    assert m.encode([]).shape == (0, 128)                                # (nothing to encode: no launch)
    full = SentenceConfig()
    assert (full.vocab_size, full.max_position_embeddings, full.pad_token_id, full.layer_norm_eps, full.max_seq_length,
            full.relative_attention_num_buckets) == (30527, 514, 1, 1e-5, 384, 32)


# ------------------------------------------------------------------------------------------------ the kernel's argument contract
def test_relbias_arguments_are_refused_before_any_launch():
    """vidil_attention_f32 with arith = 2 validates on the host; the fields behind kv16 are read for that value of arith only."""
    from vidil_amd import _lib

    lib = _lib.load()
    table = (ctypes.c_float * 64)()

    def args(**kw):
        a = _lib.AttnF32Args()
        a.q = a.k = a.v = a.out = 16
        a.ldq = a.ldk = a.ldv = 384
        a.ldo, a.Bq, a.H, a.Nq, a.Nk, a.kv_rows, a.kv_group, a.scale = 128, 2, 2, 8, 12, 12, 1, 0.125
        a.arith, a.rel_bias, a.rel_bias_ld, a.rel_off = 2, ctypes.addressof(table), 32, 7
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(text, **kw):
        assert lib.vidil_attention_f32(ctypes.byref(args(**kw)), None) == -1
        assert text in lib.vidil_last_error(), lib.vidil_last_error()

    refused(b"rel_bias is NULL or not 4-byte aligned", rel_bias=None)
    refused(b"rel_bias is NULL or not 4-byte aligned", rel_bias=ctypes.addressof(table) + 2)
    refused(b"rel_off=6 < Nq - 1 = 7", rel_off=6)
    refused(b"rel_off=21 + Nk=12 > rel_bias_ld=32", rel_off=21)
    refused(b"kv16 must be 0", kv16=1)
    refused(b"anc must be NULL", anc=16, anc_ld=12, arena_rows=2, Nq=1)
    refused(b"2: split-operand + relative-position bias", arith=3)
    assert _lib.ABI_VERSION == 13 and [f[0] for f in _lib.AttnF32Args._fields_][-5:] == ["arith", "kv16", "rel_bias", "rel_bias_ld", "rel_off"]


# ------------------------------------------------------------------------------------------------ the consumers, on a stub encoder
@pytest.fixture
def host_closest(monkeypatch):
    """The consumers select through vidil_amd.sentence.closest (HIP kernels); here its contract restated on the host."""
    import vidil_amd.sentence as S

    monkeypatch.setattr(S, "closest", sc.host_closest)


EXAMPLE = ("Objects: First, a. Then, b.\nFrame Captions: First, a dog runs. Then, a man talks.\nSubtitle: hello there\n"
           "Video Caption: a dog and a man")
QA_EXAMPLE = "Objects: First, a.\nFrame Captions: First, cap one.\nQuestion:  what is shown? \nAnswer: a dog"


def test_comparing_text_extractions():
    from vidil_amd.prompts import comparing_text

    assert comparing_text(QA_EXAMPLE, "question") == "what is shown?"
    assert comparing_text(EXAMPLE, "caption") == "First, a dog runs. Then, a man talks."
    assert comparing_text(EXAMPLE, "caption_asr") == "First, a dog runs. Then, a man talks.\nSubtitle: hello there"
    assert comparing_text(EXAMPLE, "anything else") == EXAMPLE
    with pytest.raises(IndexError):
        comparing_text(EXAMPLE, "question")


def test_select_from_support_set_order_and_ties(host_closest):
    from vidil_amd.prompts import select_from_support_set

    examples = [f"Question: s{i}?\nAnswer: x" for i in range(5)]
    e = lambda *v: torch.tensor(v, dtype=torch.float32)
    # cosines with the query (1, 0): s0 0.6, s1 1.0, s2 0.8, s3 0.8 (a tie with s2), s4 0.0
    vec = {"s0?": e(0.6, 0.8), "s1?": e(1, 0), "s2?": e(0.8, 0.6), "s3?": e(0.8, 0.6), "s4?": e(0, 1), "q?": e(2, 0), "r?": e(0, 3)}
    enc = sc.StubEncoder(vec)
    support = enc.encode([f"s{i}?" for i in range(5)])
    q = "Frame Captions: x\nQuestion: q?\nAnswer:"
    pick = lambda n, query=q: select_from_support_set(enc, support, examples, query, N=n)
    assert pick(1) == [examples[1]]
    assert pick(3) == [examples[3], examples[2], examples[1]]                   # highest LAST; of the tie, index 2 is the closer
    assert pick(2) == [examples[2], examples[1]]
    assert pick(9) == [examples[4], examples[0], examples[3], examples[2], examples[1]]      # N > support set: all of it
    enc.calls.clear()
    both = select_from_support_set(enc, support, examples, [q, "Question: r?\n"], N=2)
    assert both == [[examples[2], examples[1]], [examples[0], examples[4]]]
    assert enc.calls == [["q?", "r?"]]                                          # one batch, the question lines alone


def test_map_answers(host_closest):
    from vidil_amd.video_qa import accuracy, map_answers

    e = lambda *v: torch.tensor(v, dtype=torch.float32)
    vec = {"dog": e(1, 0, 0), "cat": e(0, 1, 0), "car": e(0, 0, 1), "kitten": e(0, 1, 0), "a big dog": e(0.9, 0.1, 0.1), "a kitten": e(0.1, 0.8, 0.3),
           "vehicle": e(0.2, 0.1, 0.9)}
    enc = sc.StubEncoder(vec)
    result = [{"question_id": 7, "answer": "a big dog"}, {"question_id": 3, "answer": "a kitten"}, {"question_id": 5, "answer": "vehicle"}]
    mapped = map_answers(result, ["dog", "cat", "car", "kitten"], enc)
    assert mapped == [{"question_id": 7, "answer": "dog"}, {"question_id": 3, "answer": "cat"}, {"question_id": 5, "answer": "car"}]   # cat == kitten: the first
    assert enc.calls == [["dog", "cat", "car", "kitten"], ["a big dog", "a kitten", "vehicle"]]
    assert accuracy(mapped, [{"question_id": 7, "answer": "dog"}, {"question_id": 3, "answer": "kitten"}]) == 0.5
    assert map_answers([], ["dog"], enc) == []


def test_in_context_selection_equals_the_reference_generator(host_closest):
    """tests/golden/in_context_prompts_golden.json: written by the reference's own save_prompt_lines_with_in_context_selection with
    the stub encoder of sentence_cases (tests/golden/make_in_context_golden.py)."""
    import copy

    from vidil_amd.prompts import in_context_selection_prompt_lines

    runs = json.load(open(os.path.join(GOLDEN, "in_context_prompts_golden.json")))["runs"]
    assert len(runs) == 6
    for r in runs:
        enc = sc.StubEncoder()
        lines, idx = in_context_selection_prompt_lines(copy.deepcopy(r["visual_tokens"]), r["filtered"], r["unfiltered"], r["N"],
                                                       "INSTRUCTION LINE", list(r["examples"]), copy.deepcopy(r["config"]), r["qa"], r["asr"],
                                                       comparing_target=r["comparing_target"], model=enc)
        assert lines == r["lines"], (r["config"]["prompt_task"], r["comparing_target"])
        assert {str(k): (list(v) if isinstance(v, tuple) else v) for k, v in idx.items()} == r["idx"]
        assert len(enc.calls) == 2 and len(enc.calls[0]) == len(r["examples"]) and len(enc.calls[1]) == len(lines)   # support once, queries once
