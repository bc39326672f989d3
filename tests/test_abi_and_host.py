"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every symbol
include/vidil_hip.h declares (no compute calls), the ctypes mirror agrees with the header,
argument validation fails loudly, and the host-side mirror of the reference interface."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

HEADER = os.path.join(ROOT, "include", "vidil_hip.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vidil_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_exactly_the_declared_symbols():
    from vidil_amd import _lib

    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vidil_hip.h but not exported"
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert lib.vidil_num_entry_points() == len(names) == 28
    assert lib.vidil_abi_version() == 13 == _lib.ABI_VERSION


def test_gemm_args_struct_matches_header_field_order():
    from vidil_amd._lib import GemmArgs

    src = open(HEADER).read()
    body = src[src.index("typedef struct vidil_gemm_args"):src.index("} vidil_gemm_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0])
    assert fields == [f[0] for f in GemmArgs._fields_]


def test_attn_f32_args_struct_matches_header_field_order():
    from vidil_amd._lib import AttnF32Args

    src = open(HEADER).read()
    end = src.index("} vidil_attn_f32_args;")
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())[0])
    assert fields == [f[0] for f in AttnF32Args._fields_]
    # types: 64-bit strides / pointers, 32-bit everything else (spot checks of the layout)
    assert AttnF32Args.ldq.size == 8 and AttnF32Args.q_off.size == 4 and AttnF32Args.scale.size == 4 and AttnF32Args.anc.size == 8


def test_argument_validation_without_a_gpu():
    """Bad shapes are rejected before any launch, with a message (error convention of the ABI)."""
    from vidil_amd import _lib

    lib = _lib.load()
    g = _lib.GemmArgs()
    assert lib.vidil_gemm(ctypes.byref(g), None) == -1
    assert b"null operand" in lib.vidil_last_error()
    g.A, g.W, g.M, g.N, g.K = 16, 16, 8, 8, 100
    assert lib.vidil_gemm(ctypes.byref(g), None) == -1
    assert b"multiple of 64" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 4, 800, 4, 800, 800, 1, 0, 0, 768, 0, 0, 0, None) == -3
    assert b"not supported" in lib.vidil_last_error()
    # fragment-tiled K/V: key capacity a multiple of 32, at most 32 query rows per unit
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 3, 12, 1, 197, 1, 200, 0, 3, 0, 0, 768, 1, 0, 0, None) == -1
    assert b"multiple of 32" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 40, 12, 1, 197, 1, 224, 0, 40, 0, 0, 768, 1, 0, 0, None) == -1
    assert b"at most 32 query rows" in lib.vidil_last_error()
    # the edges of the staged / direct kernels' contract (tests/test_attention_forms_gpu.py covers what is inside it): 769 keys
    # with at most 32 rows per unit on plain K / V; row-major V (NP == 0) with at most 32 rows; a V^T stride that is no multiple
    # of 16; group_start together with kv_index; fp8 rows at ldo % 16 != 0; split3 rows at ldo % 24 != 0
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 4, 769, 4, 769, 784, 1, 0, 0, 768, 0, 0, 0, None) == -3
    assert b"Nk=769 > 768 not supported" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 4, 64, 4, 64, 0, 1, 0, 0, 768, 0, 0, 0, None) == -1
    assert b"row-major V (NP == 0) needs more than 32 query rows" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 40, 64, 40, 64, 72, 1, 0, 0, 768, 0, 0, 0, None) == -1
    assert b"NP=72 must be a multiple of 16" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, 16, 16, 1, 1, 1, 12, 40, 64, 40, 64, 64, 1, 0, 0, 768, 0, 0, 0, None) == -1
    assert b"group_start and kv_index are mutually exclusive" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 1, 40, 64, 40, 64, 64, 1, 0, 0, 72, 0, 0, 2, None) == -1
    assert b"out_dtype" in lib.vidil_last_error()
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 1, 40, 64, 40, 64, 64, 1, 0, 0, 200, 0, 0, 0x100, None) == -1
    assert b"split3 output needs ldo=200" in lib.vidil_last_error()
    assert lib.vidil_scan_topk_ws_bytes(128, 42784, 5) > 0
    # the parity mode's f32 attention: 16-byte aligned rows / head offsets, one query row per batch in the arena form
    a = _lib.AttnF32Args()
    assert lib.vidil_attention_f32(ctypes.byref(a), None) == -1 and b"null pointer" in lib.vidil_last_error()
    a.q = a.k = a.v = a.out = 16
    a.ldq = a.ldk = a.ldv = 770
    a.ldo, a.Bq, a.H, a.Nq, a.Nk, a.kv_rows, a.kv_group = 768, 2, 12, 4, 4, 4, 1
    assert lib.vidil_attention_f32(ctypes.byref(a), None) == -1 and b"16-byte aligned" in lib.vidil_last_error()
    a.ldq = a.ldk = a.ldv = 2304
    a.anc, a.anc_ld, a.arena_rows = 16, 20, 6
    assert lib.vidil_attention_f32(ctypes.byref(a), None) == -1 and b"one query row per batch" in lib.vidil_last_error()
    # unknown operand type codes are argument errors; the kernel-name query follows the dispatch without launching
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 4, 64, 4, 64, 64, 1, 0, 0, 768, 0, 7, 7, None) == -1
    assert b"unknown dtype" in lib.vidil_last_error()
    g = _lib.GemmArgs()
    g.A, g.W, g.out, g.M, g.N, g.K, g.ldo, g.epi, g.dtype = 16, 16, 16, 201728, 768, 768, 768, 1, 1
    buf = ctypes.create_string_buffer(128)
    assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0 and buf.value == b"gemm256_kernel<__bf16, __bf16, 1, 0, false, false, false>"
    # ... the dispatch between the library's GEMM kernels (round 3; all of them produce the same bits — tests/test_gemm4w_gpu.py):
    # the plain f32 epilogue stays on the 8-wave kernel (above); 16-bit outputs of a big grid go to the 4-wave kernel;
    # a mid-size grid (10,752 decode rows x 768 columns: 126 tiles of 256^2, 252 of 128 x 256) to its 128-row-tile form;
    # a small problem to the small-tile kernel
    import os
    if not any(k in os.environ for k in ("VIDIL_GEMM4W", "VIDIL_GEMM4W128", "VIDIL_GEMM256")):
        g.K = 3072            # ... unless the reduction is long (round 4: the towers' last fc2, the parity mode's K-tripled GEMMs)
        assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0 and buf.value == b"gemm4w_kernel<__bf16, __bf16, 1, 0, false, false, false, 4, false>"
        g.K = 768
        g.epi = 0
        assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0 and buf.value == b"gemm4w_kernel<__bf16, __bf16, 0, 0, false, false, false, 4, false>"
        g.M, g.epi = 10752, 1
        assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0 and buf.value == b"gemm4w_kernel<__bf16, __bf16, 1, 0, false, false, false, 2, false>"
        g.epi = 1
    g.M, g.dtype = 3072, 0
    assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0 and buf.value.startswith(b"gemm_kernel<_Float16, ")
    g.dtype = 5
    assert lib.vidil_gemm(ctypes.byref(g), None) == -1 and b"unknown dtype" in lib.vidil_last_error()
    # fp8 operands: K a multiple of 128, a 16-bit companion type, the 256x256 kernel whatever M is
    g.dtype, g.dtype16, g.K = 2, 0, 192
    assert lib.vidil_gemm(ctypes.byref(g), None) == -1 and b"multiple of 128" in lib.vidil_last_error()
    g.K, g.M = 768, 100
    assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == -1 and b"w_scale" in lib.vidil_last_error()
    g.w_scale = 16
    assert lib.vidil_gemm_kernel_name(ctypes.byref(g), buf, 128) == 0 and buf.value == b"gemm256_kernel<fp8, _Float16, 1, 0, false, false, false>"
    # the refusals of the epilogue features (ln_fold, out16, out16_split3, ln_stats_out, rln, fp8, split_k): each from a struct that
    # is valid but for the one field named (tests/test_gemm_stat_forms_gpu.py covers what is inside the contract)
    def gemm_refused(needle, base, **fields):
        plain = dict(A=16, W=16, out=16, M=300, N=128, K=256, ldo=128, epi=0, dtype=0)
        a, ok = _lib.GemmArgs(), _lib.GemmArgs()
        for k, v in {**plain, **base, **fields}.items():
            setattr(a, k, v)
        for k, v in {**plain, **base}.items():
            setattr(ok, k, v)
        assert lib.vidil_gemm_kernel_name(ctypes.byref(ok), buf, 128) == 0, (needle, lib.vidil_last_error())
        assert lib.vidil_gemm(ctypes.byref(a), None) == -1 and needle in lib.vidil_last_error(), (needle, lib.vidil_last_error())

    fold = dict(ln_fold=1, ln_colsum=16, ln_stats=16, ln_eps=1e-5)
    gemm_refused(b"A rows must be dense", fold, lda=264)
    gemm_refused(b"LayerNorm widths up to 1024", fold, K=1088)
    gemm_refused(b"only EPI_F16 / EPI_HEADS / EPI_ARENA consume", fold, epi=1)
    gemm_refused(b"gemm/split_k", dict(K=192, **fold), split_k=1)
    prod = dict(epi=1, out16=16, ldo16=128)
    gemm_refused(b"only the f32 residual epilogue writes the 16-bit copy", prod, epi=0)
    split3 = dict(epi=1, out16=16, ldo16=384, out16_split3=1)
    gemm_refused(b"three planes", split3, ldo16=388)
    gemm_refused(b"gemm/out16_split3: the plain f32 epilogue", split3, ln_stats_out=16)
    stats = dict(prod, ln_stats_out=16)
    gemm_refused(b"gemm/ln_stats_out", stats, N=136, ldo=136, ldo16=136)
    gemm_refused(b"gemm/ln_stats_out", stats, act=1)
    rln = dict(stats, resid=16, rln_gamma=16, rln_beta=16, ln_stats=16, ln_eps=1e-5)
    gemm_refused(b"gemm/rln: the residual LayerNorm needs", rln, ln_stats_out=None)
    gemm_refused(b"dense residual rows", rln, ldo=136)
    gemm_refused(b"dense residual rows", rln, N=1088, ldo=1088, ldo16=1088)
    fp8 = dict(dtype=2, dtype16=0, w_scale=16, epi=1)
    gemm_refused(b"is not built for fp8 operands", fp8, epi=0)
    gemm_refused(b"w_scale", fp8, w_scale=None)
    gemm_refused(b"multiple of 128", fp8, K=192)
    gemm_refused(b"EPI_F8 needs fp8 operands", dict(), epi=5)
    # out_dtype of the attention: fp8 only from the staged kernel
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 4, 64, 4, 64, 64, 1, 0, 0, 768, 0, 0, 2, None) == -1
    assert b"out_dtype" in lib.vidil_last_error()
    # VIDIL_DT_SPLIT3 outputs ([hi | lo | hi] planes): ldo must hold three planes of >= H*64 columns
    assert lib.vidil_attention(16, 16, 16, 16, None, None, None, 0, 0, 1, 12, 4, 64, 4, 64, 64, 1, 0, 0, 768, 0, 0, 0x100, None) == -1
    assert b"split3" in lib.vidil_last_error()
    assert lib.vidil_beam_attention(16, 16, 16, 16, 16, 4, 12, 3, 4, 8, 768, 0, 0x100, None) == -1
    assert b"split3" in lib.vidil_last_error()
    assert lib.vidil_beam_attention(16, 16, 16, 16, 16, 4, 12, 3, 4, 8, 768, 0, 1, None) == -1
    assert b"out_dtype" in lib.vidil_last_error()


def test_product_path_refuses_cpu_tensors():
    from vidil_amd import kernels as K
    from vidil_amd.vit import VisionTransformer

    with pytest.raises(K.VidilHipError):
        K.gemm(torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8, 64, dtype=torch.float16))
    v = VisionTransformer(img_size=32, patch_size=16, embed_dim=256, depth=1, num_heads=4)
    with pytest.raises(K.VidilHipError):
        v(torch.zeros(1, 3, 32, 32))


def test_state_dict_names_match_reference_checkpoints():
    """the key names BLIP .pth files carry."""
    from vidil_amd.blip import BLIP_Decoder
    from vidil_amd.blip_itm import BLIP_ITM
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    tok = SyntheticBertTokenizer()
    cap = BLIP_Decoder(image_size=224, vit="base", tokenizer=tok)
    keys = set(cap.state_dict().keys())
    for k in ["visual_encoder.blocks.0.attn.qkv.weight", "visual_encoder.pos_embed", "visual_encoder.cls_token",
              "visual_encoder.patch_embed.proj.weight", "text_decoder.bert.encoder.layer.0.crossattention.self.key.weight",
              "text_decoder.cls.predictions.decoder.weight", "text_decoder.cls.predictions.bias",
              "text_decoder.bert.embeddings.word_embeddings.weight", "text_decoder.bert.encoder.layer.11.output.LayerNorm.bias"]:
        assert k in keys, k
    assert tuple(cap.state_dict()["visual_encoder.blocks.0.attn.qkv.weight"].shape) == (2304, 768)
    assert tuple(cap.state_dict()["text_decoder.cls.predictions.decoder.weight"].shape) == (30524, 768)
    assert len([k for k in cap.visual_encoder.state_dict()]) == 150
    assert cap.prompt_length == 4 and cap.prompt_ids(2, "cpu").tolist() == [[30522, 1037, 3861, 1997]] * 2
    itm = BLIP_ITM(image_size=224, vit="base", tokenizer=tok)
    ik = set(itm.state_dict().keys())
    for k in ["itm_head.weight", "text_encoder.encoder.layer.3.crossattention.output.dense.weight", "vision_proj.weight"]:
        assert k in ik, k
    # the reference's BertLMHeadModel(configs/med_config.json) key names (tests/golden/make_fullsize_golden.py)
    with open(os.path.join(ROOT, "tests", "golden", "med_decoder_keys.json")) as f:
        ref_keys = set("text_decoder." + k for k in json.load(f))
    mine = set(k for k in keys if k.startswith("text_decoder."))
    assert ref_keys == mine, ref_keys ^ mine


def test_load_checkpoint_semantics(tmp_path):
    """models/blip.py:332-354: checkpoint['model'], pos-embed interpolation from a 384 checkpoint, strict=False."""
    from vidil_amd.blip import BLIP_Decoder, blip_decoder
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    with pytest.raises(RuntimeError):        # a checkpoint + the stand-in vocabulary is refused unless asked for
        blip_decoder(pretrained=os.path.join(tmp_path, "x.pth"), image_size=64, vit="base", tokenizer=SyntheticBertTokenizer())
    tok = SyntheticBertTokenizer(allow_pretrained=True)
    src = BLIP_Decoder(image_size=64, vit="base", tokenizer=tok)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    big = torch.randn(1, 1 + 36, 768)          # a checkpoint trained at 96x96 (6x6 grid)
    sd["visual_encoder.pos_embed"] = big
    sd["unexpected.key"] = torch.zeros(1)
    path = os.path.join(tmp_path, "ckpt.pth")
    torch.save({"model": sd}, path)
    m = blip_decoder(pretrained=path, image_size=64, vit="base", tokenizer=tok)
    assert tuple(m.visual_encoder.pos_embed.shape) == (1, 17, 768)
    from oracle import vit_ref

    assert torch.allclose(m.visual_encoder.pos_embed, vit_ref.interpolate_pos_embed(big, 16), atol=1e-6)
    assert torch.equal(m.text_decoder.bert.embeddings.word_embeddings.weight, sd["text_decoder.bert.embeddings.word_embeddings.weight"])


def test_synthetic_tokenizer_round_trip_and_itm_padding():
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    tok = SyntheticBertTokenizer()
    assert tok("a picture of ").input_ids == [101, 1037, 3861, 1997, 102]
    ids = [30522, 1037, 3861, 1997, 2000, 17, 29999, 102, 0, 0]
    text = tok.decode(ids, skip_special_tokens=True)
    assert text == "a picture of w2000 w17 w29999" and text[len("a picture of "):] == "w2000 w17 w29999"
    enc = tok(["w2000 w17", "w5"], padding="max_length", truncation=True, max_length=35, return_tensors="pt")
    assert enc.input_ids.shape == (2, 35) and enc.input_ids[0, :4].tolist() == [101, 2000, 17, 102]
    assert enc.attention_mask.sum(1).tolist() == [4, 3]
    long = tok(" ".join(f"w{i}" for i in range(1000, 1100)), truncation=True, max_length=35)
    assert len(long.input_ids) == 35 and long.input_ids[-1] == 102


def test_capfilt_host_logic():
    from vidil_amd import capfilt

    assert capfilt.dedup(["a", "b", "a", "c", "b"]) == ["a", "b", "c"]
    assert capfilt.keep_caption([0.1, 0.41, 0.2], 0.4, "max_filter") is True
    assert capfilt.keep_caption([0.1, 0.40, 0.2], 0.4, "max_filter") is False       # strict '>'
    assert capfilt.keep_caption([0.3, 0.6], 0.4, "avg_filter") is True
    items = [dict(video_id="v0", text=["x"], unfiltered_text=["x", "y"]), dict(video_id="v1", text=[], unfiltered_text=["z"]),
             dict(video_id="v2", text=["q"])]
    f, u = capfilt.collect_outputs(items)
    assert f == {"v0": ["x"]} and u == {"v0": ["x", "y"], "v1": ["z"]}              # v1 filtered out, v2 never processed


def test_balanced_shards_cover_everything_in_order():
    from vidil_amd import dist as vdist

    for n, w in [(16, 8), (10, 4), (3, 8), (0, 2), (2990, 8)]:
        bounds = [vdist.shard_bounds(n, w, r) for r in range(w)]
        assert bounds[0][0] == 0 and bounds[-1][1] == n
        assert all(bounds[i][1] == bounds[i + 1][0] for i in range(w - 1))
        sizes = [e - s for s, e in bounds]
        assert max(sizes) - min(sizes) <= 1
    assert [e - s for s, e in (vdist.shard_bounds(16, 8, r) for r in range(8))] == [2] * 8


def test_init_tokenizer_never_falls_back_silently(monkeypatch, tmp_path):
    from vidil_amd import tokenizer as T

    monkeypatch.setenv("VIDIL_TOKENIZER", "synthetic")
    assert isinstance(T.init_tokenizer(), T.SyntheticBertTokenizer)
    monkeypatch.delenv("VIDIL_TOKENIZER")
    monkeypatch.setenv("VIDIL_BERT_VOCAB", str(tmp_path / "missing_vocab.txt"))
    with pytest.raises(FileNotFoundError):
        T.init_tokenizer()
    monkeypatch.delenv("VIDIL_BERT_VOCAB")
    monkeypatch.setenv("HF_HUB_OFFLINE", "1")
    try:
        tok = T.init_tokenizer()              # a box with the vocabulary cached gets the real tokenizer
        assert not getattr(tok, "is_synthetic", False)
    except RuntimeError as e:                 # no vocabulary anywhere: loud, and names the explicit opt-in
        assert "VIDIL_TOKENIZER=synthetic" in str(e)
    # a real vocab file works and carries the two added special tokens at the reference's ids
    vocab = tmp_path / "vocab.txt"
    words = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + ["a", "picture", "of", "dog"]
    vocab.write_text("\n".join(words) + "\n")
    tok = T.init_tokenizer(str(vocab))
    assert tok.bos_token_id == len(words) and tok.enc_token_id == len(words) + 1 and tok.sep_token_id == 102


def test_capfilt_config_is_validated_up_front():
    from vidil_amd.capfilt import validate_config

    good = dict(caption=True, filter=True, filter_generated_only=True, keep_original_caption=False, threshold=0.4)
    validate_config(good)
    for k in ("caption", "filter", "threshold", "filter_generated_only", "keep_original_caption"):
        bad = dict(good); bad.pop(k)
        with pytest.raises(KeyError):
            validate_config(bad)
    with pytest.raises(ValueError):    # would keep every original caption unfiltered
        validate_config(dict(caption=False, filter=True, filter_generated_only=True, threshold=0.4))
    validate_config(dict(caption=False, filter=True, filter_generated_only=False, threshold=0.4))


def test_split_sentences_requires_spacy_or_an_explicit_opt_in(monkeypatch):
    from vidil_amd import capfilt

    capfilt.split_sentences.__dict__.pop("_nlp", None)
    try:
        import spacy  # noqa: F401
        spacy.load("en_core_web_sm")
        have = True
    except Exception:
        have = False
    if not have:
        monkeypatch.delenv("VIDIL_SENTENCE_SPLIT", raising=False)
        with pytest.raises(RuntimeError):
            capfilt.split_sentences(["One sentence here. Another one there."])
        monkeypatch.setenv("VIDIL_SENTENCE_SPLIT", "naive")
        with pytest.warns(UserWarning):
            out = capfilt.split_sentences(["One sentence here. Another one there."])
        assert out == ["One sentence here", "Another one there."]
        capfilt.split_sentences.__dict__.pop("_nlp", None)
    assert capfilt.split_sentences(["a\nb"], do_sentence_tokenization=False) == ["a. b"]
    assert capfilt.split_sentences([]) == []


def test_clip_model_from_pretrained_reads_the_hf_directory_layout(tmp_path):
    """run_visual_tokenization.py:347-348 `CLIPModel.from_pretrained(name)`: a directory written by the installed
    transformers' save_pretrained (config.json + model.safetensors) loads key for key."""
    transformers = pytest.importorskip("transformers")
    from vidil_amd.clip import CLIPModel

    hc = transformers.CLIPConfig(
        text_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=300,
                         max_position_embeddings=16, eos_token_id=299, bos_token_id=298),
        vision_config=dict(hidden_size=192, intermediate_size=384, num_hidden_layers=2, num_attention_heads=3, image_size=64,
                           patch_size=16),
        projection_dim=96)
    torch.manual_seed(3)
    hf = transformers.CLIPModel(hc).eval()
    hf.save_pretrained(str(tmp_path))
    m = CLIPModel.from_pretrained(str(tmp_path))
    assert m.config.projection_dim == 96 and m.config.vision_config.patch_size == 16 and m.config.text_config.vocab_size == 300
    assert m.config.text_config.eos_token_id == 299
    ref = {k: v for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    own = m.state_dict()
    assert set(ref) == set(own)
    assert all(torch.equal(own[k], ref[k]) for k in ref)
    # state_dict= form, and a checkpoint that lacks a tensor is an error, not a silent random init
    m2 = CLIPModel.from_pretrained(str(tmp_path), state_dict=ref)
    assert torch.equal(m2.state_dict()["visual_projection.weight"], ref["visual_projection.weight"])
    bad = dict(ref); bad.pop("logit_scale")
    with pytest.raises(RuntimeError):
        CLIPModel.from_pretrained(str(tmp_path), state_dict=bad)


def test_clip_processor_text_side_and_no_cpu_fallback_for_images():
    from vidil_amd.clip import CLIPProcessor
    from vidil_amd.tokenizer import Encoding

    def fake_bpe(texts, return_tensors="pt", padding=True, truncation=True, **_):
        L = max(len(t.split()) for t in texts) + 2
        ids = torch.full((len(texts), L), 49407, dtype=torch.long)
        mask = torch.zeros((len(texts), L), dtype=torch.long)
        for i, t in enumerate(texts):
            n = len(t.split())
            ids[i, 0] = 49406
            ids[i, 1:1 + n] = torch.tensor([1000 + len(w) for w in t.split()])
            mask[i, :n + 2] = 1
        return Encoding(input_ids=ids, attention_mask=mask)

    proc = CLIPProcessor(tokenizer=fake_bpe)
    enc = proc(text=["A photo of dog", "A photo of a big cat"], return_tensors="pt", padding=True, truncation=True)
    assert tuple(enc["input_ids"].shape) == (2, 8) and "pixel_values" not in enc
    assert enc.to("cpu")["attention_mask"].sum().item() == 6 + 8
    if not torch.cuda.is_available():
        with pytest.raises(Exception):
            proc(images=[np.zeros((10, 12, 3), np.uint8)], return_tensors="pt")


def test_bench_gflop_model_reproduces_baseline_md_section_4():
    """bench.py derives the algorithmic GFLOP/frame from the geometry (so ViT-L/16, 384^2 and CLIP-L/14 get their own
    figures); at the headline geometry it must reproduce BASELINE.md §4 / SURVEY.md §8d."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    g = b.gflop_per_frame("base", 224, "b32")
    for key, want in dict(vit_caption=35.13, decode=20.05, itm_kv=5.58, itm_per_caption=7.24, clip=8.82, scan=0.044).items():
        assert abs(g[key] - want) <= 0.005 * want + 0.002, (key, g[key], want)
    total8 = 2 * g["vit_caption"] + g["decode"] + g["itm_kv"] + 8 * g["itm_per_caption"] + g["clip"] + g["scan"]
    assert abs(total8 - 162.6) < 0.5
    assert abs(b.gflop_per_frame("large", 224, "b32")["vit_caption"] - 123.11) < 0.1       # config 4
    assert abs(b.gflop_per_frame("base", 384, "l14")["vit_caption"] - 110.97) < 0.1
    assert abs(b.gflop_per_frame("base", 384, "l14")["clip"] - 162.03) < 0.2


def test_itm_short_circuit_host_logic_equals_the_exhaustive_schedule_on_stand_in_models(monkeypatch):
    """Host logic of CapFiltEngine's two filter schedules with stand-in models (no GPU): a deterministic pseudo-random
    probability per (frame, caption text), so the kept lists must be identical for every threshold while the short
    circuit scores fewer pairs; covers captions shared by several frames, original captions (no home frame) and
    videos whose captions all fail on their own frame."""
    import zlib

    import numpy as np
    import torch

    from vidil_amd import capfilt
    from vidil_amd.capfilt import CapFiltEngine as _Engine

    class _Done:
        def synchronize(self):
            pass

    class CapFiltEngine(_Engine):                # the two places the engine touches the device itself
        def _to_host(self, key, t):
            return t.clone(), _Done()

    monkeypatch.setattr(capfilt, "blip_frames", lambda frames, size: frames)
    Nv, F = 5, 4
    frame_caps = [f"cap {(v * 7 + f * 3) % 5} of {v}" for v in range(Nv) for f in range(F)]      # repeats inside a video

    class _Vis:
        def forward_u8(self, flat, mean, std):
            return None, torch.arange(flat.shape[0], dtype=torch.float32).view(-1, 1)             # "features" = frame id

    class _Cap(torch.nn.Module):
        visual_encoder = _Vis()

        def generate_ids(self, y16, n, **kw):
            return torch.arange(n).view(-1, 1), None

        def decode_captions(self, tok):
            return [frame_caps[int(i)] for i in tok.view(-1).tolist()]

    class _Flt(torch.nn.Module):
        visual_encoder = _Vis()
        calls = []

        def tokenize(self, caps):
            self.texts = list(caps)
            ids = torch.zeros(len(caps), 35, dtype=torch.int32)
            ids[:, 1] = torch.arange(len(caps), dtype=torch.int32)          # "token" 1 names the caption
            lens = torch.tensor([5 + zlib.crc32(c.encode()) % 30 for c in caps], dtype=torch.int32)   # 5..34: all buckets
            return ids, lens

        def project_image_kv(self, y16, n, min_rows):
            return "cross"

        def itm_pairs(self, y16, n_images, ids, lens, image_index=None, group_start=None, max_group=0, pair_text=None, cross=None):
            if group_start is not None:
                gs = group_start.numpy()
                image_index = np.repeat(np.arange(n_images), np.diff(gs))
                assert np.diff(gs).max() == max_group
            img = np.asarray(image_index).astype(np.int64)
            assert int(lens.max()) <= max(e for e in (8, 12, 16, 20, 24, 28, 35) if e >= int(lens.max()))
            txt = ids[:, 1].numpy()[pair_text.numpy()]                      # rows of ids are a subset of the captions
            assert len(img) == len(txt)
            self.calls.append(len(txt))
            u = np.array([zlib.crc32(f"{i}|{self.texts[t]}".encode()) / 2 ** 32 for i, t in zip(img, txt)], dtype=np.float64)
            u = np.clip(u, 1e-6, 1 - 1e-6)
            logit = np.log(u / (1 - u))
            return torch.from_numpy(np.stack([np.zeros_like(logit), logit], axis=1).astype(np.float32))

    frames = torch.zeros(Nv, F, 8, 8, 3, dtype=torch.uint8)
    some_split = False
    for thr, min_pairs in [(t, m) for t in (0.0, 0.2, 0.5, 0.8, 0.97, 1.0) for m in (1, 2048)]:
        CapFiltEngine.MIN_BUCKET_PAIRS = min_pairs          # 1: every length bucket is its own call; 2048: one call
        for keep in (False, True):
            out = {}
            for short in (False, True):
                cfg = dict(caption=True, filter=True, filter_generated_only=not keep, keep_original_caption=keep, threshold=thr,
                           filter_mode="max_filter", generation_mode="beam", image_size=8, vit="base",
                           do_sentence_tokenization=False, itm_short_circuit=short)
                flt = _Flt()
                flt.calls = []
                eng = CapFiltEngine(cfg, "cpu", captioner=_Cap(), filterer=flt)
                items = [dict(video_id=f"v{v}", text=["an original caption", f"another {v}"] if keep else []) for v in range(Nv)]
                eng.process(items, frames)
                out[short] = (items, eng.last_stats["itm_pairs"], list(flt.calls))
            assert out[True][0] == out[False][0], (thr, keep)
            assert out[True][1] == sum(out[True][2]) and out[False][1] == sum(out[False][2])
            assert out[True][1] <= out[False][1]
            assert (len(out[False][2]) > 1) == (min_pairs == 1)          # length buckets really were separate calls
            kept = sum(len(i["text"]) for i in out[True][0])
            some_split |= 0 < kept < sum(len(i["unfiltered_text"]) for i in out[True][0])
            if thr == 0.0 and not keep:       # everything passes on its own frame: one pair per distinct caption
                assert out[True][1] == sum(len(i["unfiltered_text"]) for i in out[True][0])
    assert some_split
    # avg_filter has no short circuit: the flag is ignored
    cfg = dict(caption=True, filter=True, filter_generated_only=True, keep_original_caption=False, threshold=0.5,
               filter_mode="avg_filter", generation_mode="beam", image_size=8, vit="base", do_sentence_tokenization=False,
               itm_short_circuit=True)
    flt = _Flt()
    flt.calls = []
    eng = CapFiltEngine(cfg, "cpu", captioner=_Cap(), filterer=flt)
    items = [dict(video_id=f"v{v}", text=[]) for v in range(Nv)]
    eng.process(items, frames)
    assert eng.last_stats["itm_pairs"] == sum(len(i["unfiltered_text"]) for i in items) * F


def test_the_drivers_build_hook_passes():
    """__graft_entry__.build() is what the driver runs every round: make (a no-op on an up-to-date tree), the oracle's C
    part, and its own checks of the loaded library — an ABI bump that forgets the hook must fail here, not there."""
    import __graft_entry__ as g

    g.build()


def test_length_buckets_merge_a_small_tail_only_when_the_padding_it_adds_is_cheap():
    """ADVICE r3 (capfilt._length_buckets): a handful of long captions behind a large bucket of short ones used to be merged
    into it unconditionally — padding every pair of the large bucket to the long captions' length (+50 % rows on real
    caption length distributions).  The merge is now decided by the rows it adds."""
    import numpy as np

    from vidil_amd.capfilt import CapFiltEngine

    eng = CapFiltEngine.__new__(CapFiltEngine)           # (host logic only: no models, no device)
    F = 8
    # 3,000 captions of 9-12 tokens (one bucket of 24,000 pairs) + 5 captions of 30 tokens (40 pairs)
    lens = np.r_[np.random.default_rng(0).integers(9, 13, 3000), np.full(5, 30)].astype(np.int64)
    idx = np.arange(len(lens))
    b = eng._length_buckets(idx, lens, F)
    assert [len(x) for x in b] == [3000, 5], [len(x) for x in b]          # merging would add 3000 * 8 * 18 = 432,000 rows
    assert np.array_equal(np.sort(np.concatenate(b)), idx)
    # the same tail behind a bucket that already runs to 28 tokens: 300 captions * 8 * 2 = 4,800 rows -> merged
    lens2 = np.r_[np.full(300, 28), np.full(5, 30)].astype(np.int64)
    b2 = eng._length_buckets(np.arange(305), lens2, F)
    assert [len(x) for x in b2] == [305]
    # equal lengths (the synthetic benchmark): one bucket, as before
    assert [len(x) for x in eng._length_buckets(np.arange(100), np.full(100, 20, dtype=np.int64), F)] == [100]
