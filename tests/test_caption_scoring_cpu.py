"""Teacher-forced caption scoring, the parts that need no GPU: argument validation of the teacher-forced form of
vidil_logsoftmax_topk_penalty (num_beams == 0), the target construction against a literal restatement of
models/blip.py:109-114, and the composed oracle against the reference's own BertLMHeadModel(labels=...)."""
import ctypes

import pytest
import torch

import caption_scoring_cases as cs
from vidil_amd.med import teacher_forced_targets


def test_teacher_forced_form_rejects_bad_arguments_before_any_launch():
    """Follows test_argument_validation_without_a_gpu: VIDIL_EINVAL and a message, no launch."""
    from vidil_amd import _lib

    lib = _lib.load()

    def call(logits=16, B=4, V=512, seqs=16, ld_seqs=1, out_scores=16, out_index=16):
        return lib.vidil_logsoftmax_topk_penalty(logits, None, B, 0, 0, V, -1, seqs, 0, ld_seqs, ctypes.c_float(1.0), out_scores,
                                                 out_index, None)

    assert call(seqs=None) == -1 and b"null labels" in lib.vidil_last_error()
    assert call(out_scores=None) == -1 and b"null pointer" in lib.vidil_last_error()
    assert call(logits=None) == -1 and b"null pointer" in lib.vidil_last_error()
    assert call(out_index=None) == -1 and b"null pointer" in lib.vidil_last_error()
    assert call(V=0) == -1 and b"bad shape" in lib.vidil_last_error()
    assert call(V=-3) == -1 and b"bad shape" in lib.vidil_last_error()
    assert call(B=0) == -1 and b"bad shape" in lib.vidil_last_error()
    assert call(ld_seqs=0) == -1 and b"ld_seqs" in lib.vidil_last_error()
    # the search forms are as they were: five beams are still unsupported, and the ABI did not move
    assert lib.vidil_logsoftmax_topk_penalty(16, 16, 4, 5, 5, 512, -1, 16, 4, 8, ctypes.c_float(1.0), 16, 16, None) == -3
    assert lib.vidil_num_entry_points() == 28 and lib.vidil_abi_version() == 13


def test_targets_equal_the_reference_construction_with_the_synthetic_tokenizer():
    """Prompt mask, pad mask, shift, truncation at 40 and the [DEC] swap, on the seven captions of the GPU tests."""
    from vidil_amd.blip import BLIP_Decoder

    tok = cs.SmallTokenizer()
    caps = cs.captions()
    ids_ref, mask_ref, targets_ref = cs.reference_targets(tok, caps, cs.PROMPT_LENGTH)
    ids, lens = BLIP_Decoder.tokenize_captions(type("M", (), {"tokenizer": tok})(), caps)
    assert ids.dtype == torch.int32 and torch.equal(ids.long(), ids_ref) and torch.equal(lens.long(), mask_ref.sum(1))
    assert lens.tolist() == [min(n, 40) for n in cs.TOKEN_COUNTS] and ids.shape[1] == 40
    assert bool((ids[:, 0] == tok.bos_token_id).all()) and int(ids[5, 39]) == tok.sep_token_id       # truncated: ends on [SEP]
    got = teacher_forced_targets(ids, lens, cs.PROMPT_LENGTH)
    assert torch.equal(got[:, :-1], targets_ref[:, 1:]) and bool((got[:, -1] == -100).all())
    assert (got >= 0).sum(1).tolist() == [min(n, 40) - cs.PROMPT_LENGTH for n in cs.TOKEN_COUNTS]    # one target for caption 0


def test_targets_on_hand_written_ids():
    pad, bos = 0, 510
    ids = torch.tensor([[bos, 7, 8, 9, 41, 42, 102, pad, pad],
                        [bos, 7, 8, 9, 102, pad, pad, pad, pad],
                        [bos, 7, 8, pad, pad, pad, pad, pad, pad],      # cut inside the prompt: nothing to score
                        [bos, 7, 8, 9, 51, 52, 53, 54, 102]])
    lens = torch.tensor([7, 5, 3, 9])
    # literal: targets = ids with pad -> -100, the first 4 positions -> -100; logits at t against targets at t + 1
    targets = ids.masked_fill(ids == pad, -100)
    targets[:, :4] = -100
    got = teacher_forced_targets(ids, lens, 4)
    assert torch.equal(got[:, :-1], targets[:, 1:])
    assert got.tolist() == [[-100, -100, -100, 41, 42, 102, -100, -100, -100],
                            [-100, -100, -100, 102, -100, -100, -100, -100, -100],
                            [-100] * 9,
                            [-100, -100, -100, 51, 52, 53, 54, 102, -100]]


def test_composed_oracle_equals_the_reference_lm_head_model_with_labels():
    """Live: the reference's BertLMHeadModel(..., labels=..., reduction='none') on the small geometry against
    med_ref.bert_model + med_ref.lm_head + cross_entropy as the GPU tests compose them."""
    from oracle import ref_shim

    if not ref_shim.available():
        pytest.skip("reference tree not present")
    pytest.importorskip("transformers")
    _, med_mod = ref_shim.load()
    cfg = ref_shim.med_config(encoder_width=256)
    cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size = 256, 4, 512
    cfg.num_hidden_layers, cfg.vocab_size, cfg.max_position_embeddings = 2, 512, 64
    dec = med_mod.BertLMHeadModel(cfg).eval()
    sd, enc = cs.small_state()
    msg = dec.load_state_dict({k[len("text_decoder."):]: v for k, v in sd.items() if k.startswith("text_decoder.")}, strict=False)
    assert not msg.unexpected_keys and all("position_ids" in k for k in msg.missing_keys), msg
    ref = cs.reference()
    e = enc[torch.tensor(cs.IMAGE_INDEX)]
    with torch.no_grad():
        out = dec(ref["ids"], attention_mask=ref["mask"], encoder_hidden_states=e,
                  encoder_attention_mask=torch.ones(e.shape[:2], dtype=torch.long), labels=ref["labels"], return_dict=True,
                  reduction="none")
        mean = dec(ref["ids"], attention_mask=ref["mask"], encoder_hidden_states=e,
                   encoder_attention_mask=torch.ones(e.shape[:2], dtype=torch.long), labels=ref["labels"], return_dict=True).loss
    assert (out.logits - ref["logits"]).abs().max().item() < 2e-4
    assert torch.allclose(out.loss, ref["none"], rtol=1e-5, atol=1e-4)
    assert torch.allclose(mean, ref["mean"], rtol=1e-5, atol=1e-5)
