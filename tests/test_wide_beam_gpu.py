"""Beam searches of 5..16 beams on the GPU: `lsm_topk_wide_kernel` against fp64 on every case of tests/wide_beam_cases.py, its
refusals, the device loop (BeamBuffers -> logsoftmax_topk -> beam_update -> beam_finalize; `beam_update_wide_kernel`) against
oracle/beam_ref.py, the generators at 5 and 8 beams against that oracle driven by the device's own logits, the captured step
graphs, and the early refusal of 17 beams.  Before the wide kernels every launch below with more than 4 beams returned
VIDIL_EUNSUP "num_beams=5 not supported (1..4)"."""
import json
import os

import numpy as np
import pytest
import torch

import branch_cases as bc
import video_captioning_cases as C
import vqa_cases as vc
import wide_beam_cases as W
from test_caption_scoring_gpu import _captioner
from test_caption_scoring_gpu import small_med_json  # noqa: F401  (fixture)
from test_video_captioning_gpu import _model as _video_model
from test_video_captioning_gpu import _run

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _k():
    from vidil_amd import kernels
    return kernels


# ================================================================================================ 1. selection vs fp64
def _launch(k, c, dev_logits):
    kw = {}
    if c.get("hist") is not None:
        kw = dict(seqs=c["hist"].to(DEV), cur_len=c["cur_len"], penalty=c["penalty"])
    B = c["logits"].shape[0] // c["nbl"]
    s, i = k.logsoftmax_topk(dev_logits, c["beam_scores"].to(DEV), B, c["nb"], c["ban"], beams_in_logits=c["nbl"], **kw)
    return s.cpu().numpy().astype(np.float64), i.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("V,nb,nbl", W.selection_shapes())
def test_wide_selection_vs_fp64(V, nb, nbl):
    """Ten launches per shape (plain / banned, penalties 0.6 and 1.3 with 64 and 1 history tokens), B = 5.  Indices equal the
    reference's best 2 nb (f32 log-softmax + beam score; score descending, flat index ascending) exactly; scores are within 4x the
    error of torch's own f32 chain against fp64 on the same case, the bound the narrow kernel is held to.

    MI355X: torch f32 vs fp64 per case 7.0e-07 .. 3.4e-06; the kernel's worst |error| over a shape's launches in units of its
    case's yardstick: 0.22 .. 0.58 on the 24 shapes of the four kinds, 0.80 on the minimal one (V = 40)."""
    k = _k()
    worst, yards, dev = 0.0, [], None
    for key in W.selection_keys([(V, nb, nbl)]):
        c = bc.beam_case(*key)
        if dev is None:
            dev = c["logits"].to(DEV)
        s, i = _launch(k, c, dev)
        assert np.array_equal(i, c["order"][:, :2 * nb]), (key, i, c["order"])
        err = np.abs(s - np.take_along_axis(c["full64"], i, 1)).max()
        worst = max(worst, err / c["yardstick"])
        yards.append(c["yardstick"])
        assert err <= 4.0 * c["yardstick"], (key, err, c["yardstick"])
    print(f"\nwide logsoftmax_topk V={V} nb={nb} nbl={nbl} ({W.kind_of(V)}): torch f32 vs fp64 per case {min(yards):.3e} .. "
          f"{max(yards):.3e}; kernel worst |error| / that = {worst:.2f} (allowed 4)")


@pytest.mark.parametrize("name,nb,nbl", W.TIED)
def test_wide_selection_on_tied_rows(name, nb, nbl):
    """Rows of three logit levels and constant rows: the strict form of the kernel (more than half a wave's buffer within the
    margin of its K-th best).  Equal logits have equal scores, so the expected indices are exact: lower index first."""
    k = _k()
    c = W.tied_case(name, nb, nbl)
    s, i = _launch(k, c, c["logits"].to(DEV))
    assert np.array_equal(i, c["order"]), (i, c["order"])
    want = np.take_along_axis(c["full64"], i, 1)
    err = np.abs(s - want).max()
    # torch's f32 chain is no yardstick here: on a constant row of 2,044 logits it happens to be exact to 2e-8.  The bound is the
    # number format's: `(x - max) - lse + beam_score` is three f32 roundings and one logf, each at most one unit in the last
    # place of the largest magnitude involved (|score| and lse, both below 16 here) — four such units.
    ulp = 2.0 ** (np.floor(np.log2(np.abs(want).max())) - 23)
    print(f"\nwide logsoftmax_topk tied rows {name} nb={nb} nbl={nbl}: worst |error| {err:.3e} = {err / ulp:.2f} f32 ulp of the score "
          f"(allowed 4; torch f32 vs fp64 on the case: {c['yardstick']:.3e})")
    assert np.abs(want).max() < 16 and err <= 4.0 * ulp
    assert (np.diff(s, axis=1) <= 0).all()


# ========================================================================================================= 2. refusals
def test_wide_selection_refusals_write_nothing():
    k = _k()
    B, V = 2, 100
    logits = torch.zeros(B * 17, V, device=DEV)
    for nb, nbl, v, what in ((17, 17, V, "not supported"), (17, 1, V, "not supported"), (16, 1, 31, "fewer than 2"), (5, 5, 1, "fewer than 2")):
        s = torch.full((B, 2 * nb), 7.5, device=DEV)
        i = torch.full((B, 2 * nb), -3, dtype=torch.int32, device=DEV)
        bs = torch.zeros(B * nb, device=DEV)
        hist = torch.zeros(B * nb, 8, dtype=torch.int32, device=DEV)
        for kw in ({}, dict(seqs=hist, cur_len=4, penalty=1.3)):
            with pytest.raises(k.VidilHipError, match=what):
                k.logsoftmax_topk(logits.view(-1)[:B * nbl * v].view(B * nbl, v), bs, B, nb, -1, out_scores=s, out_index=i,
                                  beams_in_logits=nbl, **kw)
        torch.cuda.synchronize()
        assert bool((s == 7.5).all()) and bool((i == -3).all())
    with pytest.raises(k.VidilHipError, match="1..16"):
        bufs17 = k.BeamBuffers(B, 17, 8, DEV)
        k.beam_update(bufs17, torch.zeros(B, 34, device=DEV), torch.zeros(B, 34, dtype=torch.int32, device=DEV), V, 4, 2, 0)


# ================================================================================================ 3. the device loop
@pytest.mark.parametrize("penalty", [1.0, W.SEARCH_PENALTY], ids=["plain", "penalty"])
@pytest.mark.parametrize("nb", W.NBS)
@pytest.mark.parametrize("name", sorted(W.SEARCH))
def test_wide_device_loop_matches_the_oracle(name, nb, penalty):
    """BeamBuffers -> logsoftmax_topk -> beam_update -> beam_finalize on the table language models of wide_beam_cases: token ids
    equal oracle/beam_ref.py's exactly, scores to rel 1e-5.  The small case fills the hypothesis sets, displaces entries and fires
    `done` before the length limit at every width (asserted from the oracle's run by tests/test_wide_beam_cpu.py)."""
    k = _k()
    c = W.SEARCH[name]
    ref = W.search_reference(name, nb, penalty)
    fn = W.table_logits_fn(name, nb)
    B, V, P = c["B"], c["V"], len(c["prompt"])
    bufs = k.BeamBuffers(B, nb, c["max_length"], DEV)
    bufs.reset(torch.from_numpy(W.search_prompt(name)).to(torch.int32).to(DEV))
    cur_len = P
    while True:
        ids = bufs.seqs[:, :cur_len].cpu().numpy().astype(np.int64)
        cs_, ci = k.logsoftmax_topk(torch.from_numpy(fn(ids)).to(DEV), bufs.beam_scores, B, nb, c["eos"] if cur_len < c["min_length"] else -1,
                                    seqs=bufs.seqs if penalty != 1.0 else None, cur_len=cur_len, penalty=penalty)
        k.beam_update(bufs, cs_, ci, V, cur_len, c["eos"], c["pad"])
        cur_len += 1
        if cur_len >= c["max_length"] or int(bufs.n_done.item()) == B:
            break
    assert cur_len - P == ref["steps"]                         # the loop stops where the oracle's does
    tok, ln, score = k.beam_finalize(bufs, cur_len, c["eos"], c["pad"])
    tok, ln = tok.cpu().numpy(), ln.cpu().numpy()
    for b in range(B):
        n = len(ref["seqs"][b])
        assert tok[b][:n].tolist() == ref["seqs"][b].tolist(), (b, tok[b], ref["seqs"][b])
        assert np.all(tok[b][n:] == c["pad"])
        assert score[b].item() == pytest.approx(ref["scores"][b], rel=1e-5)


# ======================================================================================================= 4. the models
def _oracle_on_device_logits(text_decoder, enc, B, nb, prompt, max_length, min_length, eos, pad, penalty=1.0):
    """oracle/beam_ref.py's search stepping a fresh DecoderSession: the tokens a correct search finds on the device's own logits."""
    from oracle import beam_ref
    from vidil_amd.blip import DecoderSession

    sess = DecoderSession(text_decoder, enc, B, nb, max_length, tiled_cross=True)
    seqs, _ = beam_ref.beam_search(lambda i, b: _run(sess, i, b, nb).numpy(), np.asarray(prompt, dtype=np.int64), num_beams=nb,
                                   max_length=max_length, min_length=min_length, eos_token_id=eos, pad_token_id=pad,
                                   repetition_penalty=penalty)
    return seqs


def _vqa_med_json(small_med_json):  # noqa: F811
    """The small configuration with its encoder_width key, which BLIP_VQA's answer decoder needs (tests/test_vqa_gpu.py's own
    fixture writes the same file)."""
    from test_models_gpu import _small_med_cfg

    cfg = _small_med_cfg()
    path = os.path.join(os.path.dirname(small_med_json), "med_small_vqa.json")
    with open(path, "w") as f:
        json.dump({k_: getattr(cfg, k_) for k_ in ("hidden_size", "num_attention_heads", "intermediate_size", "num_hidden_layers",
                                                    "vocab_size", "max_position_embeddings", "encoder_width")}, f)
    return path


def _same_tokens(toks, seqs):
    for b, s in enumerate(seqs):
        assert np.array_equal(toks[b][:len(s)], s), (b, toks[b], s)


@pytest.mark.parametrize("nb", [5, 8])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_blip_decoder_generate_at_5_and_8_beams(small_med_json, dtype, nb):  # noqa: F811
    cap, enc16 = _captioner(small_med_json, dtype)
    B, max_length, min_length = 3, 20, 5
    kw = dict(num_beams=nb, max_length=max_length, min_length=min_length)
    flat = enc16.reshape(-1, enc16.shape[-1])
    toks = cap.generate_ids(flat, B, **kw)[0].cpu().numpy()
    prompt = cap.prompt_ids(B, "cpu").long().numpy()
    tk = cap.tokenizer
    _same_tokens(toks, _oracle_on_device_logits(cap.text_decoder, flat, B, nb, prompt, max_length, min_length, tk.sep_token_id, tk.pad_token_id))
    captions = cap.generate(torch.zeros(B, 3, 32, 32, device=DEV), **kw)
    assert captions == cap.decode_captions(torch.from_numpy(toks))
    # the repetition penalty of generate(..., repetition_penalty=1.3) at the same width
    toks_p = cap.generate_ids(flat, B, repetition_penalty=1.3, **kw)[0].cpu().numpy()
    _same_tokens(toks_p, _oracle_on_device_logits(cap.text_decoder, flat, B, nb, prompt, max_length, min_length, tk.sep_token_id,
                                                  tk.pad_token_id, penalty=1.3))


@pytest.mark.parametrize("nb", [5, 8])
def test_video_decoder_generate_past_768_keys_at_5_and_8_beams(small_med_json, nb):  # noqa: F811
    """Case a: 776 keys per video, so the decode steps' cross-attention is the key-split form with nb rows per unit."""
    from vidil_amd import video_captioning as VC

    m, video, tok16 = _video_model(small_med_json, "a", "f16")
    assert tok16.shape[0] // C.B > 768
    kw = dict(num_beams=nb, max_length=C.MAX_LENGTH, min_length=C.MIN_LENGTH)
    det = {}
    captions = m.generate(video, details=det, **kw)
    toks = det["tokens"].numpy()
    _same_tokens(toks, _oracle_on_device_logits(m.text_decoder, tok16, C.B, nb, [C.PROMPT_IDS] * C.B, C.MAX_LENGTH, C.MIN_LENGTH, C.SEP, C.PAD))
    assert captions == m.decode_captions(det["tokens"])
    d2 = {}
    res = VC.evaluation(m, [(video.cpu(), [0, 1, 2])], dict(video_representation="concat_frame", **kw), details=d2)
    assert torch.equal(d2["tokens"], det["tokens"]) and [r["caption"] for r in res] == captions


@pytest.mark.parametrize("nb", [5, 8])
def test_vqa_generate_at_5_and_8_beams(small_med_json, monkeypatch, nb):  # noqa: F811
    """BLIP_VQA's beam count is the constant of the reference (models/blip_vqa.py:92), VQA_NUM_BEAMS; set to 5 and 8 here."""
    from test_vqa_gpu import _model as _vqa_model
    from test_vqa_gpu import _states
    from vidil_amd import blip_vqa

    m = _vqa_model(_vqa_med_json(small_med_json))
    g = vc.golden()
    img, y16, ids, lens, h32, h16 = _states(m, g)
    monkeypatch.setattr(blip_vqa, "VQA_NUM_BEAMS", nb)
    Q = 4
    toks = m.generate_answer_ids(h16, Q)[0].cpu().numpy()
    _same_tokens(toks, _oracle_on_device_logits(m.text_decoder, h16, Q, nb, np.full((Q, 1), vc.DEC), vc.MAX_LENGTH, vc.MIN_LENGTH, vc.SEP, vc.PAD))
    answers = m(img, vc.questions(g), train=False, inference="generate")
    assert answers == [m.tokenizer.decode(r, skip_special_tokens=True) for r in toks.tolist()]


def test_parity_mode_decoder_generate_at_5_beams():
    """The parity precision mode (error-compensated operands; decode cross-attention in the kv16 form, 5 rows per image)."""
    from vidil_amd.blip import BLIP_Decoder
    from vidil_amd.packing import set_compute_dtype, set_parity_mode
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    torch.manual_seed(0)
    cap = BLIP_Decoder(image_size=32, vit="base", tokenizer=SyntheticBertTokenizer()).eval().to(DEV)
    set_compute_dtype("f16", cap)
    set_parity_mode(True, cap)
    B, nb, max_length, min_length = 2, 5, 8, 5
    _, y3 = cap.visual_encoder.forward_both(torch.randn(B, 3, 32, 32, device=DEV))
    toks = cap.generate_ids(y3, B, num_beams=nb, max_length=max_length, min_length=min_length)[0].cpu().numpy()
    tk = cap.tokenizer
    _same_tokens(toks, _oracle_on_device_logits(cap.text_decoder, y3, B, nb, cap.prompt_ids(B, "cpu").long().numpy(), max_length, min_length,
                                                tk.sep_token_id, tk.pad_token_id))


# ========================================================================================== 5. graphs, streams, compaction
@pytest.mark.parametrize("nb", [5, 16])
def test_wide_step_graphs_streams_and_compaction_give_the_eager_tokens(small_med_json, monkeypatch, nb):  # noqa: F811
    """The same shape generated four times (eager, captured, replayed, replayed) equals a VIDIL_DECODE_GRAPHS=0 run; so do the
    search split over two streams and the one that lets finished images leave the batch."""
    cap, enc16 = _captioner(small_med_json, "f16")
    flat = torch.cat([enc16, enc16]).reshape(-1, enc16.shape[-1]).contiguous()        # six images
    B = 6
    kw = dict(num_beams=nb, max_length=20, min_length=5)
    cap.__dict__.pop("_decode_state", None)
    monkeypatch.setenv("VIDIL_DECODE_GRAPHS", "0")
    want = cap.generate_ids(flat, B, **kw)[0].cpu()
    monkeypatch.delenv("VIDIL_DECODE_GRAPHS")
    cap.__dict__.pop("_decode_state", None)
    for call in range(4):
        assert torch.equal(cap.generate_ids(flat, B, **kw)[0].cpu(), want), call
    st = next(iter(cap._decode_state.values()))
    assert st["graphs_ok"] and len(st["graphs"]) >= 1 and st["calls"] == 4
    cap.__dict__.pop("_decode_state", None)
    for call in range(3):
        assert torch.equal(cap.generate_ids(flat, B, streams=2, **kw)[0].cpu(), want), call
    cap.__dict__.pop("_decode_state", None)
    for call in range(3):
        assert torch.equal(cap.generate_ids(flat, B, compact_min=1, check_done_every=1, **kw)[0].cpu(), want), call
    cap.__dict__.pop("_decode_state", None)


# =================================================================================================== 6. early refusal
def test_17_beams_are_refused_before_anything_is_launched(small_med_json, monkeypatch):  # noqa: F811
    from vidil_amd import kernels as K
    from vidil_amd import video_captioning as VC

    launches = []
    gemm = K.gemm
    monkeypatch.setattr(K, "gemm", lambda *a, **kw: (launches.append(1), gemm(*a, **kw))[1])
    cap, enc16 = _captioner(small_med_json, "f16")
    img = torch.zeros(3, 3, 32, 32, device=DEV)
    for call in (lambda: cap.generate(img, num_beams=17, max_length=20, min_length=5),
                 lambda: cap.generate_ids(enc16.reshape(-1, enc16.shape[-1]), 3, num_beams=17, max_length=20, min_length=5),
                 lambda: cap.generate(img, num_beams=0)):
        with pytest.raises(K.VidilHipError, match=r"num_beams=(17|0).*16"):
            call()
    assert cap.visual_encoder.calls == 0 and not launches
    m, video, tok16 = _video_model(small_med_json, "b", "f16")
    vit_calls = m.visual_encoder.calls
    with pytest.raises(K.VidilHipError, match=r"num_beams=17.*16"):
        m.generate(video, num_beams=17, max_length=20, min_length=5)
    with pytest.raises(K.VidilHipError, match=r"num_beams=17.*16"):
        VC.evaluation(m, [(video.cpu(), [0, 1, 2])], dict(video_representation="concat_frame", num_beams=17, max_length=20, min_length=5))
    assert m.visual_encoder.calls == vit_calls and not launches
    cap.generate(img, num_beams=5, max_length=8, min_length=5)
    assert launches and cap.visual_encoder.calls == 1             # (the spy sees a search that runs)
