"""Video captioning, the parts that need no GPU: the import shim and the checkpoint keys, the refusals that come before any
launch, the bookkeeping of vidil_amd/video_captioning.py's ``evaluation``, and the fixture of tests/video_captioning_cases.py
itself — what a dropped key or a swapped video does to the oracle's logits, against the gates the GPU tests apply."""
import types

import numpy as np
import pytest
import torch

import video_captioning_cases as C

F16_GATE, BF16_GATE = 1.25e-3, 1e-2        # test_models_gpu.PLAIN_F16_REL, test_caption_scoring_gpu.PLAIN_BF16_REL
SCALE = {"a": 1.45, "b": 1.54, "c": 1.72}                     # max |logit| over every decoder call of the oracle's search
LOSE_LAST_TWO = {"a": 9.4e-2, "b": 1.5e-1, "c": 8.8e-2}       # max |d prompt-pass logits| without a video's last two keys
LOSE_PAST_768 = {"a": 5.3e-1, "c": 2.6e-1}                    # ... without the keys past 768
WRONG_VIDEO = 5.2e-1                                          # ... captioning from another video: at least


@pytest.fixture(scope="module")
def cpu_model():
    from vidil_amd.blip import BLIP_Video_Decoder
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    return BLIP_Video_Decoder(image_size=32, vit="base", tokenizer=SyntheticBertTokenizer())


def test_shim_exports_defaults_and_state_dict_keys(cpu_model):
    from vidil_amd import blip as mod
    from vidil_amd.tokenizer import SyntheticBertTokenizer
    from models.blip import BLIP_Decoder, BLIP_Video_Decoder, blip_decoder, blip_decoder_video  # noqa: F401  (the reference's path)

    assert BLIP_Video_Decoder is mod.BLIP_Video_Decoder and blip_decoder_video is mod.blip_decoder_video
    assert issubclass(BLIP_Video_Decoder, BLIP_Decoder)
    assert cpu_model.prompt == "a video of " and cpu_model.prompt_length == len(cpu_model.tokenizer("a video of ").input_ids) - 1
    image_model = BLIP_Decoder(image_size=32, vit="base", tokenizer=SyntheticBertTokenizer())
    assert list(cpu_model.state_dict().keys()) == list(image_model.state_dict().keys())       # a BLIP_Decoder checkpoint loads
    assert {k: tuple(v.shape) for k, v in cpu_model.state_dict().items()} == {k: tuple(v.shape) for k, v in image_model.state_dict().items()}
    m = blip_decoder_video(image_size=32, vit="base", tokenizer=SyntheticBertTokenizer(), prompt="a clip of ")
    assert isinstance(m, BLIP_Video_Decoder) and m.prompt == "a clip of "


def test_token_bound_is_16384_and_is_refused_before_any_launch(cpu_model):
    from vidil_amd.blip import MAX_VIDEO_TOKENS

    assert MAX_VIDEO_TOKENS == 16384
    cpu_model._require_video_tokens(16384)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model._require_video_tokens(16385)
    # image_size 32: 5 tokens per frame; 3,277 frames are 16,385 tokens — refused on a CPU tensor, so before any launch
    frames = torch.zeros(1, 1, 3, 32, 32).expand(1, 3277, 3, 32, 32)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model.generate(frames)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model(frames, ["a video of w200"])
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model.generate(torch.zeros(1, 1, 32, 32, 3, dtype=torch.uint8).expand(1, 3277, 32, 32, 3))
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model.generate_ids(torch.zeros(16385, 768, dtype=torch.float16), 1)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        cpu_model.sample_ids(torch.zeros(16385, 768, dtype=torch.float16), 1)
    with pytest.raises(ValueError, match=r"f32 \[B,N,3,S,S\] expected"):
        cpu_model.generate(torch.zeros(2, 3, 32, 32))


def test_parity_and_fp8_are_refused(cpu_model):
    from vidil_amd import packing

    cpu_model._require_plain()
    with pytest.raises(ValueError, match="parity"):
        packing.set_parity_mode(True, cpu_model)
    with pytest.raises(ValueError, match="fp8"):
        packing.set_compute_dtype("fp8", cpu_model)
    packing.set_parity_mode(True, cpu_model.text_decoder)
    try:
        with pytest.raises(ValueError, match="parity"):
            cpu_model.generate(torch.zeros(1, 2, 3, 32, 32))
        with pytest.raises(ValueError, match="parity"):
            cpu_model.generate_ids(torch.zeros(10, 768, dtype=torch.float16), 1)
    finally:
        packing.set_parity_mode(False, cpu_model.text_decoder)
    cpu_model._require_plain()


def test_videos_per_block_follows_the_retrieval_evaluations_budget(cpu_model):
    from vidil_amd.video_retrieval import KV_BLOCK_BYTES

    cfg = cpu_model.text_decoder.config
    per_video = cfg.num_hidden_layers * 2 * 1576 * cfg.hidden_size * 2
    assert cpu_model.videos_per_block(1576) == KV_BLOCK_BYTES // per_video >= 1
    assert cpu_model.videos_per_block(10 ** 9) == 1


# ---------------------------------------------------------------------------------------------- evaluation's bookkeeping
class _StubModel:
    """Records what ``evaluation`` hands to the model: a frame's first pixel is its number."""

    def __init__(self):
        self.text_decoder = torch.nn.Linear(1, 1)
        self.visual_encoder = types.SimpleNamespace(forward_both=self._frames, forward_u8=self._frames_u8)
        self.log = []

    def _require_plain(self):
        pass

    def _frames(self, x):                       # f32 [b,3,S,S] -> one token per frame whose value is the frame's number
        assert x.dim() == 4 and x.shape[1] == 3
        t = x[:, 0, 0, 0].view(-1, 1).clone()
        return t.view(-1, 1, 1), t

    def _frames_u8(self, x, mean, std):
        assert x.dim() == 4 and x.shape[-1] == 3 and x.dtype == torch.uint8
        t = x[:, 0, 0, 0].float().view(-1, 1)
        return t.view(-1, 1, 1), t

    def video_tokens(self, v):
        assert v.dim() == 5 and v.shape[2] == 3
        return v[:, :, 0, 0, 0].reshape(-1, 1).clone()

    def video_tokens_u8(self, v):
        assert v.dim() == 5 and v.shape[-1] == 3 and v.dtype == torch.uint8
        return v[:, :, 0, 0, 0].float().reshape(-1, 1)

    def generate(self, tok3, sample=False, videos_per_block=None, details=None, **kw):
        self.log.append(("generate", tok3.clone(), sample, videos_per_block, kw))
        details["tokens"] = tok3[:, :, 0].to(torch.int32)
        return [" ".join(str(int(x)) for x in row) for row in tok3[:, :, 0]]

    def decode_captions(self, out_tok):
        return [" ".join(str(int(x)) for x in row) for row in out_tok]


def _numbered(V, N, first=0):
    v = torch.zeros(V, N, 3, 4, 4)
    v[:, :, 0, 0, 0] = first + torch.arange(V * N, dtype=torch.float32).view(V, N)
    return v


def test_evaluation_bookkeeping_ids_order_and_the_single_frame_pick(monkeypatch):
    from vidil_amd import video_captioning as VC

    cfg = dict(video_representation="concat_frame", num_beams=3, max_length=30, min_length=5)
    m = _StubModel()
    batches = [(_numbered(2, 5), ["video9", "video3"]), (_numbered(1, 5, first=10).numpy(), ("video7",))]
    det = {}
    res = VC.evaluation(m, batches, cfg, videos_per_block=2, details=det)
    assert res == [{"video_id": "video9", "caption": "0 1 2 3 4"}, {"video_id": "video3", "caption": "5 6 7 8 9"},
                   {"video_id": "video7", "caption": "10 11 12 13 14"}]                  # arrival order, every frame, ids kept
    assert [c[0] for c in m.log] == ["generate", "generate"] and all(c[2] is False and c[3] == 2 for c in m.log)
    assert all(c[4] == dict(num_beams=3, max_length=30, min_length=5) for c in m.log)
    assert det["tokens"].tolist() == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14]]
    # uint8 batches take the fused preprocessing entry
    u8 = torch.zeros(2, 5, 4, 4, 3, dtype=torch.uint8)
    u8[:, :, 0, 0, 0] = torch.arange(10, dtype=torch.uint8).view(2, 5)
    assert [r["caption"] for r in VC.evaluation(m, [(u8, [1, 2])], cfg)] == ["0 1 2 3 4", "5 6 7 8 9"]
    # single_frame: frame int(N / 2) alone, through BLIP_Decoder's search
    seen = []

    def fake_generate_ids(self, enc16, B, **kw):
        seen.append((self, enc16.clone(), B, kw))
        return enc16.view(B, -1).to(torch.int32), None

    monkeypatch.setattr(VC.BLIP_Decoder, "generate_ids", fake_generate_ids)
    cfg1 = dict(cfg, video_representation="single_frame", num_beams=2, max_length=20, min_length=4)
    m.log.clear()
    res = VC.evaluation(m, [(_numbered(2, 5), ["x", "y"]), (_numbered(3, 4, first=100), [4, 5, 6])], cfg1)
    assert not m.log
    assert res == [{"video_id": "x", "caption": "2"}, {"video_id": "y", "caption": "7"},            # frame int(5 / 2) = 2
                   {"video_id": 4, "caption": "102"}, {"video_id": 5, "caption": "106"}, {"video_id": 6, "caption": "110"}]   # int(4 / 2) = 2
    assert [(s[0] is m, s[2], s[3]) for s in seen] == [(True, 2, dict(num_beams=2, max_length=20, min_length=4)),
                                                       (True, 3, dict(num_beams=2, max_length=20, min_length=4))]
    assert [r["caption"] for r in VC.evaluation(m, [(u8, [1, 2])], cfg1)] == ["2", "7"]
    with pytest.raises(ValueError, match="video_representation"):
        VC.evaluation(m, batches, dict(cfg, video_representation="mean_frame"))
    with pytest.raises(ValueError, match="2 ids"):
        VC.evaluation(m, [(_numbered(3, 5), ["a", "b"])], cfg)


# ---------------------------------------------------------------------------------------------- the fixture
def test_prompt_ids_are_the_small_tokenizers():
    import caption_scoring_cases as cs

    tok = cs.SmallTokenizer()
    ids = tok([cs.PROMPT], return_tensors="pt").input_ids
    ids[:, 0] = tok.bos_token_id
    assert ids[0, :-1].tolist() == C.PROMPT_IDS == [510, 7, 8, 9] and C.SEP == 102 and C.PAD == 0
    assert {c: n * t for c, (n, t) in C.CASES.items()} == {"a": 776, "b": 68, "c": 1154}


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_a_dropped_key_or_a_swapped_video_cannot_pass_the_gates(case):
    """The oracle's search (3 beams, max_length 30, min_length 5) and what its prompt-pass logits (every position of the four
    prompt tokens) lose with a video's last two keys, with the keys past 768, and with another video in its place: each at
    least five times the widest gate (bf16: 1e-2 x logit scale), so neither can pass the GPU tests.  The oracle's own candidate
    gaps are far below any gate: equality of token ids with the ORACLE's search decides nothing on these weights and is not
    asserted anywhere — printed: how many videos it would cover."""
    import caption_scoring_cases as cs

    ref = C.reference(case)
    assert len(ref["calls"]) == C.MAX_LENGTH - len(C.PROMPT_IDS) and ref["calls"][0][0].shape == (C.B * C.NUM_BEAMS, 4)
    assert ref["calls"][0][1] is None and all(bi is not None and bi.shape == (9,) for _, bi in ref["calls"][1:])
    assert ref["scale"] == pytest.approx(SCALE[case], abs=6e-3)
    widest = BF16_GATE * ref["scale"]
    assert F16_GATE * ref["scale"] == pytest.approx(2e-3, abs=3e-4) and widest == pytest.approx(1.6e-2, abs=1.6e-3)
    sd, _ = cs.small_state()

    def prompt_pass(enc):
        ids = torch.tensor([C.PROMPT_IDS] * enc.shape[0])
        return cs.oracle_logits(sd, enc, ids, torch.ones_like(ids), torch.arange(enc.shape[0]))

    tok = C.tokens(case)
    base = prompt_pass(tok)
    assert torch.equal(base[:, -1], C.prompt_logits(tok))
    last2 = (prompt_pass(tok[:, :-2]) - base).abs().max().item()
    assert last2 == pytest.approx(LOSE_LAST_TWO[case], rel=2e-2) and last2 >= 5.0 * widest
    if case in LOSE_PAST_768:
        past = (prompt_pass(tok[:, :768]) - base).abs().max().item()
        assert past == pytest.approx(LOSE_PAST_768[case], rel=2e-2) and past >= 5.0 * widest
    wrong = min((prompt_pass(tok[perm]) - base).abs().amax((1, 2)).min().item() for perm in ([1, 2, 0], [2, 0, 1]))
    assert wrong >= WRONG_VIDEO - 5e-3 and wrong >= 5.0 * widest
    gaps = ref["gen_gap"]
    assert 3e-6 <= gaps.min() and gaps.max() <= 5e-4                                   # (4e-6 .. 4e-4 over the three cases)
    for name, gate in (("f16", F16_GATE), ("bf16", BF16_GATE)):
        margin = gate * ref["scale"] * 2.0 * len(ref["calls"])
        print(f"\ncase {case} {name}: {int((gaps > margin).sum())} of {C.B} videos have every candidate gap above {margin:.3e} "
              f"(gaps {' '.join(f'{g:.1e}' for g in gaps)}): id equality with the oracle's search would cover that many")
        assert int((gaps > margin).sum()) == 0


def test_loss_reference_scores_every_caption_against_its_video():
    import caption_scoring_cases as cs

    for case in sorted(C.CASES):
        ref = C.loss_reference(case)
        assert ref["counts"].tolist() == [min(n, 40) - cs.PROMPT_LENGTH for n in cs.TOKEN_COUNTS]
        assert bool(torch.isfinite(ref["none"]).all()) and 5.0 < ref["mean"].item() < 8.0
    # another video gives another loss, by far more than the bound the GPU test allows (2 n g per caption)
    a = C.loss_reference("a")
    sd, _ = cs.small_state()
    swapped = cs.oracle_loss(cs.oracle_logits(sd, C.tokens("a"), a["ids"], a["mask"], [(v + 1) % 3 for v in C.VIDEO_INDEX]), a["labels"], "none")
    g = BF16_GATE * max(1.0, a["logits"].abs().max().item())
    assert bool(((swapped - a["none"]).abs()[a["counts"] > 0] > 2.0 * a["counts"][a["counts"] > 0].float() * g).any())
