"""Video captioning on the GPU (vidil_amd/blip.py: BLIP_Video_Decoder; vidil_amd/video_captioning.py) against the oracle composed
in tests/video_captioning_cases.py, in f16 and bf16: three videos of 776 / 68 / 1,154 keys, 3 beams, max_length 30, min_length 5.
The gates are tests/test_video_vqa_gpu.py's (PLAIN_F16_REL = 1.25e-3 and 1e-2 x logit scale): a softmax average does not get less
accurate with more keys.  The ViT is a token table, as there."""
import json
import types

import numpy as np
import pytest
import torch

import caption_scoring_cases as cs
import video_captioning_cases as C
from common import load_into
from test_models_gpu import PLAIN_F16_REL, _small_med_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
PLAIN_BF16_REL = 1e-2
SIZE = 32                          # the stub ViT reads a frame's first pixel only
CASE_NAMES = sorted(C.CASES)
NB = C.NUM_BEAMS
KW = dict(num_beams=NB, max_length=C.MAX_LENGTH, min_length=C.MIN_LENGTH)


class _FramesViT(torch.nn.Module):
    """Stands in for the ViT: a frame's first pixel holds its row in the token table [frames, T, C]; counts its calls."""

    def __init__(self, table16):
        super().__init__()
        self.table16, self.calls = table16, 0
        self.patch_embed = types.SimpleNamespace(num_patches=table16.shape[1] - 1)

    def forward_both(self, x):
        self.calls += 1
        e = self.table16[x[:, 0, 0, 0].round().long()].contiguous()
        return e.float(), e.reshape(-1, e.shape[-1])

    def forward_u8(self, x, mean, std):
        self.calls += 1
        e = self.table16[x[:, 0, 0, 0].long()].contiguous()
        return e.float(), e.reshape(-1, e.shape[-1])


def _videos(V, N, first=0):
    v = torch.zeros(V, N, 3, SIZE, SIZE)
    v[:, :, 0, 0, 0] = first + torch.arange(V * N, dtype=torch.float32).view(V, N)
    return v


@pytest.fixture(scope="module")
def small_med_json(tmp_path_factory):
    c = _small_med_cfg()
    path = tmp_path_factory.mktemp("cfg") / "med_small.json"
    path.write_text(json.dumps({k: getattr(c, k) for k in ("hidden_size", "num_attention_heads", "intermediate_size",
                                                           "num_hidden_layers", "vocab_size", "max_position_embeddings")}))
    return str(path)


_MODELS = {}


def _model(med_json, case, dtype):
    """A BLIP_Video_Decoder of the small geometry (the decoder of med_decoder_small.npz, prompt ids 510 7 8 9) whose ViT hands out
    the case's token table.  One per (case, dtype), shared: (model, videos f32 [3, N, 3, S, S] on the device, tokens 16-bit)."""
    from vidil_amd.blip import BLIP_Video_Decoder
    from vidil_amd.med import BertLMHeadModel
    from vidil_amd.packing import set_compute_dtype

    if (case, dtype) not in _MODELS:
        N, T = C.CASES[case]
        sd, _ = cs.small_state()
        m = BLIP_Video_Decoder(med_config=med_json, image_size=SIZE, vit="base", tokenizer=cs.SmallTokenizer(), prompt=cs.PROMPT)
        assert m.prompt_length == cs.PROMPT_LENGTH
        m.text_decoder = load_into(BertLMHeadModel(_small_med_cfg()), sd, "text_decoder.").to(DEV)
        tdt = torch.float16 if dtype == "f16" else torch.bfloat16
        m.visual_encoder = _FramesViT(C.tokens(case).view(-1, T, C.WIDTH).to(DEV).to(tdt).contiguous())
        set_compute_dtype(dtype, m)
        video = _videos(C.B, N).to(DEV)
        tok16 = m.video_tokens(video)
        assert tuple(tok16.shape) == (C.B * N * T, C.WIDTH)
        assert torch.equal(tok16.float().cpu().view(C.B, -1, C.WIDTH), C.tokens(case))          # a video's N*T rows are contiguous
        _MODELS[(case, dtype)] = (m, video, tok16)
    return _MODELS[(case, dtype)]


def _gate(dtype):
    return PLAIN_F16_REL if dtype == "f16" else PLAIN_BF16_REL


def _run(sess, ids_, beam_idx, nb=NB):
    """One decoder call of a beam search on a DecoderSession: the shared prompt pass (beam_idx None), else a step."""
    if beam_idx is None:
        lg = sess.prefill(torch.from_numpy(ids_[::nb].copy()).to(torch.int32).reshape(-1).to(DEV), ids_.shape[1], shared=True)
        return lg.cpu().repeat_interleave(nb, 0)
    return sess.step(torch.from_numpy(ids_[:, -1].copy()).to(torch.int32).to(DEV),
                     torch.from_numpy(beam_idx).to(torch.int32).to(DEV), ids_.shape[1] - 1).cpu()


def _spy_attention(monkeypatch):
    """Records (Nk, kv_tiled, rows per unit) of every K.attention launch."""
    from vidil_amd import kernels as K

    seen, attention = [], K.attention

    def shim(*a, **kw):
        rows = kw["Nq"] * (kw.get("max_group", 0) if kw.get("group_start") is not None else 1 if kw.get("kv_index") is not None
                           else kw.get("kv_group", 1))
        seen.append((kw["Nk"], kw.get("kv_tiled", False), rows))
        return attention(*a, **kw)

    monkeypatch.setattr(K, "attention", shim)
    return seen


@pytest.mark.parametrize("fused", ["1", "0"], ids=["ln_folded", "ln_launched"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_every_decoder_call_of_the_oracles_search_within_the_gate(small_med_json, monkeypatch, case, dtype, fused):
    """The shared prompt pass (4 rows per video) and each of the 25 steps (3 rows per video) on the oracle's tokens and beam_idx,
    through a DecoderSession(tiled_cross=True) over the video's 776 / 68 / 1,154 keys — with the decoder's LayerNorms folded
    into its GEMMs and ($VIDIL_DECODE_FUSE_LN=0) as separate launches.  Before the key-split attention form, cases a and c raised
    "needs more than 32 query rows per unit (got 4)" on the first call.  The cross-attention launches over more than 768 keys
    carry kv_tiled = 2; case b's are the image captioner's (kv_tiled = True)."""
    from vidil_amd.blip import DecoderSession

    m, _, tok16 = _model(small_med_json, case, dtype)
    ref, gate = C.reference(case), _gate(dtype)
    monkeypatch.setenv("VIDIL_DECODE_FUSE_LN", fused)
    seen = _spy_attention(monkeypatch)
    sess = DecoderSession(m.text_decoder, tok16, C.B, NB, C.MAX_LENGTH, tiled_cross=True)
    assert sess.fused_ln == (fused == "1")
    worst = []
    for s, (ids_, beam_idx) in enumerate(ref["calls"]):
        lg = _run(sess, ids_, beam_idx)
        live = torch.from_numpy(ids_[:, -1] != C.PAD)
        assert bool(live.any())
        worst.append((lg - torch.from_numpy(ref["logits"][s]))[live].abs().max().item())
    print(f"\nvideo captioning {case} {dtype} fused_ln={fused}: max |d logits| per decoder call along the oracle's beam path "
          f"{' '.join(f'{w:.2e}' for w in worst)} (gate {gate * ref['scale']:.3e})")
    assert max(worst) <= gate * ref["scale"], worst
    Te = C.CASES[case][0] * C.CASES[case][1]
    cross = [x for x in seen if x[0] == Te]
    L = m.text_decoder.config.num_hidden_layers
    assert len(cross) == L * len(ref["calls"])
    assert all(x[1] == (2 if Te > 768 else True) for x in cross) and {x[2] for x in cross} == {4, 3}
    assert all(x[1] in (False, True) for x in seen if x[0] != Te)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_generate_equals_the_reference_search_on_the_devices_logits(small_med_json, case, dtype):
    """generate(video [3, N, 3, S, S]): the tokens of oracle/beam_ref.py's search driven by the device's own logits (a
    DecoderSession stepped by the restated BeamSearchScorer); the captions are their decoding; the uint8 entry gives the same."""
    from oracle import beam_ref
    from vidil_amd.blip import DecoderSession

    m, video, tok16 = _model(small_med_json, case, dtype)
    det = {}
    captions = m.generate(video, **KW, details=det)
    toks = det["tokens"].numpy()
    assert toks.shape == (C.B, C.MAX_LENGTH) and (toks[:, :4] == np.asarray(C.PROMPT_IDS)).all()
    sess = DecoderSession(m.text_decoder, tok16, C.B, NB, C.MAX_LENGTH, tiled_cross=True)
    seqs_dev, _ = beam_ref.beam_search(lambda i, b: _run(sess, i, b).numpy(), np.asarray([C.PROMPT_IDS] * C.B, dtype=np.int64), num_beams=NB,
                                       max_length=C.MAX_LENGTH, min_length=C.MIN_LENGTH, eos_token_id=C.SEP, pad_token_id=C.PAD)
    for b in range(C.B):
        assert np.array_equal(toks[b][:len(seqs_dev[b])], seqs_dev[b]), (b, toks[b], seqs_dev[b])
    assert isinstance(captions, list) and len(captions) == C.B and all(isinstance(c, str) for c in captions)
    assert captions == m.decode_captions(det["tokens"])
    N = C.CASES[case][0]
    u8 = torch.zeros(C.B, N, SIZE, SIZE, 3, dtype=torch.uint8)
    u8[:, :, 0, 0, 0] = torch.arange(C.B * N, dtype=torch.uint8).view(C.B, N)
    det8 = {}
    assert m.generate(u8.to(DEV), **KW, details=det8) == captions and torch.equal(det8["tokens"], det["tokens"])
    ref = C.reference(case)
    margin = _gate(dtype) * ref["scale"] * 2.0 * len(ref["calls"])
    print(f"\ngenerate {case} {dtype}: {int((ref['gen_gap'] > margin).sum())} of {C.B} videos have every candidate gap of the ORACLE's "
          f"search above {margin:.3e}; equality with its ids is not asserted (tests/test_video_captioning_cpu.py)")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_up_to_768_keys_nothing_new_is_dispatched(small_med_json, monkeypatch, dtype):
    """Case b (68 keys per video): the search of BLIP_Video_Decoder is BLIP_Decoder's over the same token rows — the same
    launches (no kv_tiled = 2 anywhere), the same logits bit for bit at every step, the same tokens."""
    from vidil_amd.blip import BLIP_Decoder, DecodeTrace

    m, video, tok16 = _model(small_med_json, "b", dtype)
    seen = _spy_attention(monkeypatch)
    t_video, t_image = DecodeTrace(), DecodeTrace()
    a = m.generate_ids(tok16, C.B, trace=t_video, **KW)[0].clone()
    n_video = len(seen)
    b = BLIP_Decoder.generate_ids(m, tok16, C.B, trace=t_image, **KW)[0].clone()
    assert torch.equal(a, b) and len(t_video.logits) == len(t_image.logits) == C.MAX_LENGTH - 4
    assert all(torch.equal(x, y) for x, y in zip(t_video.logits, t_image.logits))
    assert seen[:n_video] == seen[n_video:] and all(x[1] in (False, True) for x in seen) and any(x[1] is True for x in seen)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_forward_and_caption_nll_vs_composed_oracle(small_med_json, case, dtype):
    """The teacher-forced loss over videos (models/blip.py:196-219): seven captions about the three videos (video_index 0 2 2 1 0
    2 1), every launch with more than 32 query rows per video (the long-key attention form past 768 keys).  The bound of
    tests/test_caption_scoring_gpu.py: a caption with n targets within 2 n g of the oracle, the mean within 2 g."""
    m, video, tok16 = _model(small_med_json, case, dtype)
    ref = C.loss_reference(case)
    g = _gate(dtype) * max(1.0, ref["logits"].abs().max().item())
    caps = cs.captions()
    nll, cnt = m.caption_nll(video, caps, C.VIDEO_INDEX, reduction="none")
    assert nll.dtype == torch.float32 and cnt.dtype == torch.int32 and nll.is_cuda
    assert cnt.cpu().tolist() == ref["counts"].tolist()
    d = (nll.cpu() - ref["none"]).abs()
    bound = 2.0 * ref["counts"].float() * g
    mean = m.caption_nll(tok16.view(C.B, -1, C.WIDTH), caps, C.VIDEO_INDEX, reduction="mean")
    r_mean = abs(mean.item() - ref["mean"].item()) / (2.0 * g)
    pick = [1, 3, 6]                                            # forward: caption i describes video i
    sd, _ = cs.small_state()
    ids3, mask3, lab3 = cs.reference_targets(cs.SmallTokenizer(), [caps[i] for i in pick], cs.PROMPT_LENGTH)
    ref_fwd = cs.oracle_loss(cs.oracle_logits(sd, C.tokens(case), ids3, mask3, [0, 1, 2]), lab3, "mean")
    loss = m(video, [caps[i] for i in pick])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and bool(torch.isfinite(loss))
    r_fwd = abs(loss.item() - ref_fwd.item()) / (2.0 * g)
    print(f"\nvideo caption_nll {case} {dtype}: worst |d sum| / (2 n g) = {(d / bound).max().item():.3f}, |d mean| / (2 g) = {r_mean:.4f}, "
          f"forward {r_fwd:.4f} (g = {g:.3e})")
    assert bool((d <= bound).all()), (d, bound)
    assert r_mean <= 1.0 and r_fwd <= 1.0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_sampling_equals_the_reference_loop_on_the_devices_logits(small_med_json, dtype):
    """generate(sample=True) on case a: oracle/sample_ref.py's loop fed the device's own logits (one row per video over 776
    keys), the relation tests/test_sample_gpu.py asserts — with repetition penalty 1.1 although the call says 1.0
    (models/blip.py:249)."""
    from oracle import sample_ref as S
    from vidil_amd.blip import DecoderSession

    m, video, tok16 = _model(small_med_json, "a", dtype)
    seed, max_length, min_length = 20261019, 20, 5
    det = {}
    caps = m.generate(video, sample=True, top_p=0.9, max_length=max_length, min_length=min_length, repetition_penalty=1.0, seed=seed,
                      details=det)
    toks = det["tokens"].numpy()
    assert toks.shape == (C.B, max_length) and (toks[:, :4] == np.asarray(C.PROMPT_IDS)).all() and len(caps) == C.B
    sess = DecoderSession(m.text_decoder, tok16, C.B, 1, max_length, tiled_cross=True)
    ident = torch.arange(C.B, dtype=torch.int32, device=DEV)

    def step_fn(ids):
        if ids.shape[1] == 4:
            lg = sess.prefill(torch.from_numpy(ids).to(torch.int32).reshape(-1).to(DEV), 4, shared=True)
        else:
            lg = sess.step(torch.from_numpy(ids[:, -1].copy()).to(torch.int32).to(DEV), ident, ids.shape[1] - 1)
        return lg.cpu().numpy()

    trace = []
    ref = S.sample_search(step_fn, np.asarray([C.PROMPT_IDS] * C.B, dtype=np.int64), max_length=max_length, min_length=min_length,
                          eos_token_id=C.SEP, pad_token_id=C.PAD, seed=seed, rep_penalty=1.1, trace=trace)
    tight = {t["row"] for t in trace if t["margin"] < 2e-6}
    for b in range(C.B):
        if b not in tight:
            assert np.array_equal(toks[b], ref[b]), (b, toks[b], ref[b])
    assert len(tight) <= 1
    # one video per block draws what it draws in the batch (the call's seed, the video's index as its Philox row)
    det1 = {}
    m.generate(video, sample=True, top_p=0.9, max_length=max_length, min_length=min_length, seed=seed, videos_per_block=1, details=det1)
    assert torch.equal(det1["tokens"], det["tokens"])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["a", "c"])
def test_a_videos_search_does_not_depend_on_batch_block_or_graphs(small_med_json, case, dtype):
    """Bit for bit: (1) video 1 searched alone against the same video in the batch of three — every step's logits; (2)
    evaluation with one video per block against all videos in one block; (3) eager steps (the first search of a shape) against
    captured and replayed step graphs (the second and third)."""
    from vidil_amd import video_captioning as VC
    from vidil_amd.blip import DecodeTrace

    m, video, tok16 = _model(small_med_json, case, dtype)
    Te = tok16.shape[0] // C.B
    t3, t1 = DecodeTrace(), DecodeTrace()
    all3 = m.generate_ids(tok16, C.B, trace=t3, **KW)[0].clone()
    one = m.generate_ids(tok16[Te:2 * Te], 1, trace=t1, **KW)[0].clone()
    assert torch.equal(one[0], all3[1]) and len(t3.logits) == len(t1.logits) == C.MAX_LENGTH - 4
    assert torch.equal(t1.logits[0][0], t3.logits[0][1])                                    # the shared prompt pass: one row per video
    for s in range(1, len(t1.logits)):
        assert torch.equal(t1.logits[s], t3.logits[s][NB:2 * NB]), s
    cfg = dict(video_representation="concat_frame", **KW)
    ids = ["video7", "video8", "video9"]
    d1, d3 = {}, {}
    r1 = VC.evaluation(m, [(video.cpu(), ids)], cfg, videos_per_block=1, details=d1)
    r3 = VC.evaluation(m, [(video.cpu(), ids)], cfg, videos_per_block=C.B, details=d3)
    assert r1 == r3 and [x["video_id"] for x in r1] == ids and all(isinstance(x["caption"], str) for x in r1)
    assert torch.equal(d1["tokens"], d3["tokens"]) and torch.equal(d1["tokens"], all3.cpu())
    split = VC.evaluation(m, [(video[:1].cpu(), ids[:1]), (video[1:].cpu(), ids[1:])], cfg)
    assert split == r3
    # eager, then captured + replayed, then replayed: a fresh model state so that the first call of the shape is this one
    m.__dict__.pop("_decode_state", None)
    runs = [m.generate_ids(tok16, C.B, **KW)[0].clone() for _ in range(3)]
    st = next(iter(m.__dict__["_decode_state"].values()))
    assert st["calls"] == 3 and st["graphs_ok"] and len(st["graphs"]) >= 1            # (the second search captured, the third replayed)
    assert torch.equal(runs[0], all3) and torch.equal(runs[1], all3) and torch.equal(runs[2], all3)


@pytest.mark.parametrize("dtype", ["f16"])
def test_single_frame_is_the_image_captioner_on_the_middle_frame(small_med_json, dtype):
    from vidil_amd import video_captioning as VC
    from vidil_amd.blip import BLIP_Decoder

    m, video, tok16 = _model(small_med_json, "a", dtype)
    N, T = C.CASES["a"]
    cfg = dict(video_representation="single_frame", **KW)
    det = {}
    res = VC.evaluation(m, [(video.cpu(), [0, 1, 2])], cfg, details=det)
    mid = tok16.view(C.B, N, T, C.WIDTH)[:, int(N / 2)].reshape(-1, C.WIDTH).contiguous()
    want = BLIP_Decoder.generate_ids(m, mid, C.B, **KW)[0].cpu()
    assert torch.equal(det["tokens"], want) and [x["caption"] for x in res] == m.decode_captions(want)
    assert BLIP_Decoder.generate(m, video[:, int(N / 2)], **KW) == [x["caption"] for x in res]


def test_refusals(small_med_json):
    from vidil_amd import kernels as K
    from vidil_amd import video_captioning as VC
    from vidil_amd.blip import DecoderSession
    from vidil_amd.packing import set_compute_dtype, set_parity_mode

    m, video, tok16 = _model(small_med_json, "a", "f16")
    cfg = dict(video_representation="concat_frame", **KW)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        m.generate_ids(torch.zeros(16385, C.WIDTH, dtype=torch.float16, device=DEV), 1, **KW)
    with pytest.raises(ValueError, match="16385 tokens per video"):
        m.caption_nll(torch.zeros(1, 16385, C.WIDTH, dtype=torch.float16, device=DEV), [cs.PROMPT + "w200"])
    with pytest.raises(ValueError, match="videos_per_block=0"):
        m.generate(video, videos_per_block=0, **KW)
    with pytest.raises(ValueError, match="parity"):
        set_parity_mode(True, m)
    with pytest.raises(ValueError, match="fp8"):
        set_compute_dtype("fp8", m)
    set_parity_mode(True, m.text_decoder)
    try:
        with pytest.raises(ValueError, match="parity"):
            m.generate(video, **KW)
        with pytest.raises(ValueError, match="parity"):
            m(video, [cs.PROMPT + "w200"] * 3)
        with pytest.raises(ValueError, match="parity"):
            VC.evaluation(m, [(video.cpu(), [0, 1, 2])], cfg)
    finally:
        set_parity_mode(False, m.text_decoder)
    # more than 32 rows per video on fragment tiles over more than 768 keys: refused by name, with the way out
    sess = DecoderSession(m.text_decoder, tok16, C.B, 33, C.MAX_LENGTH, tiled_cross=True)
    sess.prefill(torch.tensor(C.PROMPT_IDS * C.B, dtype=torch.int32, device=DEV), 4, shared=True)
    with pytest.raises(K.VidilHipError, match="tiled_cross=False"):
        sess.step(torch.full((C.B * 33,), 7, dtype=torch.int32, device=DEV), torch.arange(C.B * 33, dtype=torch.int32, device=DEV), 4)
    torch.cuda.synchronize()
