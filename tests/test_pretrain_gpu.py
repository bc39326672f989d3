"""The forward of BLIP_Pretrain / BLIP_Pretrain_Video on the GPU against the golden recorded from the reference's own forward
(tests/golden/make_pretrain_golden.py), two consecutive calls per case, the reference's draws replayed through ``negatives=``;
and the single-frame filter (vidil_amd/pretrain.py) against the existing per-sentence ITM calls."""
import math

import pytest
import torch

import nlvr_cases as nc
import pretrain_cases as pc
from test_models_gpu import PLAIN_F16_REL

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [c.name for c in pc.CASES]
U = 2.0 ** -24                                   # unit roundoff of f32

_runs = {}


def _params(m, momentum):
    return {n: p.detach().clone() for n, p in m.named_parameters() if ("_m." in n) == momentum}


def replay(c):
    """Both calls of a case with the golden's draws, run once and shared (read-only): per call the losses, ``details`` and the
    state before / after."""
    if c.name in _runs:
        return _runs[c.name]
    g = pc.golden()
    m = pc.small_model(c).to(DEV)
    calls = []
    for call in range(pc.CALLS):
        k = f"{c.name}/{call}/"
        x, caps = pc.pixels(c, call).to(DEV), pc.captions(c, call)
        before = dict(image_queue=m.image_queue.clone(), text_queue=m.text_queue.clone(), ptr=int(m.queue_ptr),
                      online=_params(m, False), mom=_params(m, True))
        details = {}
        neg = (torch.from_numpy(g[k + "neg_image_of_text"]), torch.from_numpy(g[k + "neg_text_of_image"]))
        if c.video:                                            # positional
            ita, itm, lm = m(x, caps, c.alpha[call], negatives=neg, details=details)
        else:                                                  # alpha by keyword, as pretrain_video.py:110 passes it
            ita, itm, lm = m(x, caps, alpha=c.alpha[call], negatives=neg, details=details)
        torch.cuda.synchronize()
        calls.append(dict(ita=ita, itm=itm, lm=lm, details={n: v.clone() for n, v in details.items()}, before=before,
                          after=dict(image_queue=m.image_queue.clone(), text_queue=m.text_queue.clone(), ptr=int(m.queue_ptr),
                                     temp=float(m.temp.detach()), online=_params(m, False), mom=_params(m, True))))
    _runs[c.name] = (m, calls)
    return _runs[c.name]


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_the_new_arithmetic_alone_from_the_models_own_features_logits_and_logprobs(c):
    """What the model reports goes through the fp64 restatements; the towers' error does not enter.

    loss_ita: the bound derived in tests/test_retrieval_loss_gpu.py for the same kernel and the same torch tail —
    eps * (2 + 2 alpha / t) + 32 u * (1 / t + log(B + Q)) with eps = (D + 2) u / t.  loss_itm: torch's f32 cross-entropy of the
    reported logits, 16 u * max(1, max|logit|).  loss_lm: the f64 quotient of the reported per-caption sums and counts, rounded
    to f32 once (2 u relative); and from the reported per-target log-probabilities (kernels.token_logprobs) — the f32 products and
    the per-caption roundings of -(0.9 lp + 0.1 mean lp) move it by a few u of the largest token loss: 16 u * max(1, max|lp|),
    far inside the caption-scoring bound 2 g of tests/test_caption_scoring_gpu.py, which is asserted as that file builds it."""
    g = pc.golden()
    m, calls = replay(c)
    n_targets = sum(pc.lens(c)) - c.B
    for call, r in enumerate(calls):
        d = {n: v.cpu() for n, v in r["details"].items()}
        temp, alpha = float(d["temp"]), c.alpha[call]
        ita = pc.loss_ita64(d["image_feat"], d["text_feat"], d["image_feat_m"], d["text_feat_m"], r["before"]["image_queue"].cpu(),
                            r["before"]["text_queue"].cpu(), temp, alpha)
        eps = (pc.EMBED + 2) * U / temp
        tol = eps * (2 + 2 * alpha / temp) + 32 * U * (1 / temp + math.log(c.B + c.queue_size))
        print(f"{c.name} call {call}: loss_ita {float(r['ita']):.7f} restated {ita:.7f} |d| {abs(float(r['ita']) - ita):.2e} tol {tol:.2e}")
        for name in ("ita", "itm", "lm"):
            assert r[name].dtype == torch.float32 and r[name].dim() == 0 and r[name].is_cuda, name
        assert abs(float(r["ita"]) - ita) <= tol
        assert abs(float(r["ita"]) - float((d["loss_i2t"] + d["loss_t2i"]) / 2)) <= 2 * U * abs(ita)
        itm = pc.loss_itm64(d["itm_logits"])
        assert d["itm_logits"].shape == (3 * c.B, 2)
        assert abs(float(r["itm"]) - itm) <= 16 * U * max(1.0, float(d["itm_logits"].abs().max()))
        # the two blocks are the student rows against the batch's MOMENTUM features over the clamped temperature
        for name, a, b in (("sim_i2t", "image_feat", "text_feat_m"), ("sim_t2i", "text_feat", "image_feat_m")):
            assert (d[name].double() - d[a].double() @ d[b].double().T / temp).abs().max() <= eps, name
        # LM
        assert d["lm_loss_sum"].shape == d["lm_count"].shape == (c.B,)
        assert d["lm_count"].tolist() == [n - 1 for n in pc.lens(c)] and d["lm_lp_label"].numel() == n_targets
        quotient = float(d["lm_loss_sum"].double().sum() / d["lm_count"].sum())
        assert abs(float(r["lm"]) - quotient) <= 2 * U * quotient
        lm = pc.loss_lm64(d["lm_lp_label"], d["lm_lp_mean"])
        scale = max(1.0, float(d["lm_lp_label"].abs().max()), float(d["lm_lp_mean"].abs().max()))
        gate = PLAIN_F16_REL * max(1.0, float(g[f"{c.name}/{call}/lm_logit_scale"]))
        print(f"{c.name} call {call}: loss_lm {float(r['lm']):.7f} restated {lm:.7f} |d| {abs(float(r['lm']) - lm):.2e} "
              f"tol {16 * U * scale:.2e} (caption-scoring bound {2 * gate:.2e})")
        assert abs(float(r["lm"]) - lm) <= 16 * U * scale <= 2 * gate


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_the_three_losses_end_to_end_against_the_reference(c):
    """Features within the project's hidden-state tolerance.  |loss_ita - golden| <= 4 delta / temp + 1e-5, delta the largest
    deviation of the reported similarity blocks (x temp) from the golden's — lse and the target term are each 1-Lipschitz in the
    sup-norm of the logits, times 2 because the momentum targets move too.  |loss_itm - golden| <= 2 * PRED_REL * max(1,
    max|logit|): the project's two-logit bound through a 2-Lipschitz cross-entropy.  |loss_lm - golden| <= 2 g, g = the plain
    f16 logit gate x the reference's logit scale: the mean bound of tests/test_caption_scoring_gpu.py.
    Measured on an MI355X over the six calls: delta 8.2e-5 .. 1.6e-4; loss_ita off by 2.7e-5 .. 4.2e-4 (bounds 6.6e-4 .. 9.3e-3),
    loss_itm by 6.2e-6 .. 4.4e-5 (4.0e-3), loss_lm by 2.4e-6 .. 3.8e-5 (3.1e-3 .. 3.5e-3)."""
    g = pc.golden()
    m, calls = replay(c)
    for call, r in enumerate(calls):
        k = f"{c.name}/{call}/"
        d = {n: v.cpu() for n, v in r["details"].items()}
        temp = float(g[k + "temp"])
        for name in ("image_feat", "text_feat", "image_feat_m", "text_feat_m"):
            assert (d[name] - torch.from_numpy(g[k + name])).abs().max() <= nc.HIDDEN_TOL, name
        delta = max(float((d[n] - torch.from_numpy(g[k + n])).abs().max()) for n in ("sim_i2t", "sim_t2i")) * temp
        e = {n: abs(float(r[n]) - float(g[k + "loss_" + n])) for n in ("ita", "itm", "lm")}
        b_ita = 4 * delta / temp + 1e-5
        b_itm = 2 * pc.PRED_REL * max(1.0, float(d["itm_logits"].abs().max()))
        b_lm = 2 * PLAIN_F16_REL * max(1.0, float(g[k + "lm_logit_scale"]))
        print(f"{c.name} call {call}: delta {delta:.2e}; loss_ita off by {e['ita']:.2e} (bound {b_ita:.2e}); loss_itm off by "
              f"{e['itm']:.2e} (bound {b_itm:.2e}); loss_lm off by {e['lm']:.2e} (bound {b_lm:.2e})")
        assert e["ita"] <= b_ita and e["itm"] <= b_itm and e["lm"] <= b_lm


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_the_state_after_each_call(c):
    g = pc.golden()
    m, calls = replay(c)
    ptr = 0
    for call, r in enumerate(calls):
        k = f"{c.name}/{call}/"
        a, b, d = r["after"], r["before"], r["details"]
        assert b["ptr"] == ptr
        cols = slice(ptr, ptr + c.B)
        assert torch.equal(a["image_queue"][:, cols], d["image_feat_m"].T) and torch.equal(a["text_queue"][:, cols], d["text_feat_m"].T)
        rest = torch.ones(c.queue_size, dtype=torch.bool)
        rest[cols] = False
        assert torch.equal(a["image_queue"][:, rest], b["image_queue"][:, rest])
        assert torch.equal(a["text_queue"][:, rest], b["text_queue"][:, rest])
        ptr = (ptr + c.B) % c.queue_size
        assert a["ptr"] == ptr == int(g[k + "queue_ptr"][0])
        assert a["temp"] == pytest.approx(float(g[k + "temp"]), abs=1e-7) and 0.001 <= a["temp"] <= 0.5
        # EMA: every momentum parameter = old * 0.995 + online * 0.005 to f32 rounding; two of them against the golden's
        assert len(a["mom"]) == len(b["mom"]) > 0
        for n, p in a["mom"].items():
            want = b["mom"][n].double() * pc.MOMENTUM + b["online"][n.replace("_m.", ".")].double() * (1 - pc.MOMENTUM)
            assert (p.double() - want).abs().max() <= 6 * U * max(1.0, float(want.abs().max())), n
        for n in ("vision_proj_m.weight", "text_proj_m.bias"):
            assert (a["mom"][n].cpu() - torch.from_numpy(g[k + n])).abs().max() <= 4 * U
        # the online parameters are unchanged (temp apart: it is clamped) and tied tensors are still one object
        for n, p in a["online"].items():
            assert n == "temp" or torch.equal(p, b["online"][n]), n
    assert c.name != "image" or ptr == 0                       # the image case's queue wrapped
    # the towers re-packed after the second EMA: other momentum features for other weights
    assert not torch.equal(calls[0]["details"]["text_feat_m"], calls[1]["details"]["text_feat_m"])
    assert not torch.equal(calls[0]["details"]["image_feat_m"], calls[1]["details"]["image_feat_m"])
    for i in range(pc.TEXT_LAYERS):
        e, dl = m.text_encoder.encoder.layer[i], m.text_decoder.bert.encoder.layer[i]
        assert e.crossattention.self.value.weight is dl.crossattention.self.value.weight and e.output.dense.bias is dl.output.dense.bias
        assert e.attention.self.value.weight is not dl.attention.self.value.weight
    assert m.text_encoder.embeddings.word_embeddings.weight is m.text_decoder.bert.embeddings.word_embeddings.weight


def test_the_second_calls_momentum_features_come_from_repacked_towers():
    """The same pixels and captions twice: the online features repeat bit for bit, the momentum features move with the EMA."""
    c = pc.case("video")
    m = pc.small_model(c).to(DEV)
    x, caps = pc.pixels(c, 0).to(DEV), pc.captions(c, 0)
    d0, d1 = {}, {}
    m(x, caps, 0.4, seed=1, details=d0)
    m(x, caps, 0.4, seed=1, details=d1)
    assert torch.equal(d0["image_feat"], d1["image_feat"]) and torch.equal(d0["text_feat"], d1["text_feat"])
    assert not torch.equal(d0["image_feat_m"], d1["image_feat_m"]) and not torch.equal(d0["text_feat_m"], d1["text_feat_m"])


@pytest.mark.parametrize("c", pc.CASES, ids=IDS)
def test_own_draws_are_the_inverse_cdf_draws_of_the_reported_blocks(c):
    m = pc.small_model(c).to(DEV)
    x, caps = pc.pixels(c, 0).to(DEV), pc.captions(c, 0)
    own = torch.arange(c.B)
    seed = pc.DRAW_SEEDS[c.name]
    for call in range(2):                                      # (the second call has other momentum weights, hence other blocks)
        seen = []
        for again in range(2):
            before = {k: v.clone() for k, v in m.state_dict().items()}
            d = {}
            m(x, caps, 0.4, seed=seed, details=d)
            seen.append((d["neg_image_of_text"].cpu(), d["neg_text_of_image"].cpu()))
            excluded = 0
            for stream, name, sim in ((0, "neg_image_of_text", d["sim_t2i"]), (1, "neg_text_of_image", d["sim_i2t"])):
                want, close = pc.draws(sim, seed, stream)
                excluded += int(close.sum())
                assert torch.equal(d[name].cpu()[~close], want[~close]), (name, d[name], want)
                assert (d[name].cpu() != own).all()
            assert excluded <= 1
            if again == 0:                                     # the same call once more, from the same state
                m.load_state_dict(before)
        assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])


@pytest.fixture(scope="module")
def filterer():
    return pc.small_filterer().to(DEV)


@pytest.mark.parametrize("i", range(len(pc.SELECT_CASES)))
def test_select_frame_scores_the_pairs_of_the_per_sentence_calls(filterer, i):
    """Scores within 2 * PRED_REL * max(1, max|logit|) of the reference's schedule on the existing forward — one
    ``filterer(frames, [sentence] * N, 'itm')`` per sentence, pretrain_video.py:54-58 — and the same argmax."""
    from vidil_amd.pretrain import select_frame, select_frames, sentence_tokenization

    seed, text = pc.SELECT_CASES[i]
    frames = pc.select_pixels(seed).to(DEV)
    nlp = pc.NaiveNlp()
    sents = sentence_tokenization(text, nlp)
    logits = torch.cat([filterer(frames, [s] * pc.SELECT_FRAMES, "itm") for s in sents])
    want = torch.softmax(logits, 1)[:, 1].cpu()
    frame, sentence, scores = select_frame(filterer, frames, text, nlp)
    bound = 2 * pc.PRED_REL * max(1.0, float(logits.abs().max()))
    assert scores.shape == (len(sents), pc.SELECT_FRAMES) and len(sents) in (2, 3)
    print(f"select_frame case {i}: worst |d score| {float((scores.flatten() - want).abs().max()):.2e} (bound {bound:.2e})")
    assert (scores.flatten() - want).abs().max() <= bound
    best = int(want.argmax())
    assert (frame, sentence) == (best % pc.SELECT_FRAMES, sents[best // pc.SELECT_FRAMES])
    # the table discriminates: the scores spread (no saturated softmax), the top-2 margin is far above the bound's reach on a
    # probability, and the CPU oracle of the same pairs (first id [CLS], as the filter feeds it) names the same pair
    top = torch.sort(want, descending=True).values
    assert float(want.max() - want.min()) > 0.1 and float(top[0] - top[1]) >= 10 * pc.PRED_REL
    oracle = pc.select_oracle(pc.small_filterer(), pc.select_pixels(seed), sents)
    assert int(oracle.flatten().argmax()) == best and (scores - oracle).abs().max() <= bound
    # the batch form: the same numbers for this video, whatever stands beside it
    other_seed, other_text = pc.SELECT_CASES[1 - i]
    videos = torch.stack([pc.select_pixels(other_seed).to(DEV), frames])
    many = select_frames(filterer, videos, [other_text, text], nlp)
    assert len(many) == 2 and many[1][:2] == (frame, sentence) and torch.equal(many[1][2], scores)
    one_per_pass = select_frames(filterer, videos, [other_text, text], nlp, videos_per_pass=1)
    assert one_per_pass[1][:2] == (frame, sentence) and torch.equal(one_per_pass[0][2], many[0][2])


def test_refusals_come_by_name_before_any_launch_or_mutation(monkeypatch):
    from vidil_amd import kernels as K
    from vidil_amd.packing import set_compute_dtype, set_parity_mode

    c = pc.case("image")
    m = pc.small_model(c).to(DEV)
    v = pc.small_model(pc.case("video")).to(DEV)
    x, caps = pc.pixels(c, 0).to(DEV), pc.captions(c, 0)
    launches = []
    monkeypatch.setattr(K, "gemm", lambda *a, **k: launches.append("gemm") or (_ for _ in ()).throw(AssertionError("launched")))
    state = {k: t.clone() for k, t in m.state_dict().items()}

    def refused(exc, text, model=m, **kw):
        args = dict(alpha=0.4)
        args.update(kw)
        with pytest.raises(exc, match=text):
            model(args.pop("x", x), args.pop("caps", caps), **args)
        assert not launches and float(m.temp.detach()) == pytest.approx(c.temp0) and int(m.queue_ptr) == 0

    refused(K.VidilHipError, "BLIP_Pretrain.forward: input is on cpu", x=x.cpu())
    refused(ValueError, r"f32 \[B,3,S,S\] expected", x=x[None])
    refused(ValueError, r"f32 \[B,N,3,S,S\] expected", model=v, x=x)
    # 964 frames x 17 tokens = 16,388 keys: past the 16,384 the attention kernels serve (the pixels are never read)
    refused(ValueError, "BLIP_Pretrain_Video: 16388 tokens per video", model=v, x=torch.empty(2, 964, 3, 64, 64, device=DEV))
    refused(ValueError, "queue_size=12 is not a multiple of the batch size 5", x=x[:5], caps=caps[:5])
    refused(ValueError, "6 images and 5 captions", caps=caps[:5])
    refused(ValueError, "a batch of one has no admissible negative", x=x[:1], caps=caps[:1])
    refused(ValueError, "neg_image_of_text must hold 6 indices", negatives=(torch.arange(5), torch.arange(6)))
    refused(ValueError, "neg_text_of_image must hold 6 indices", negatives=(torch.tensor([1, 0, 0, 0, 0, 0]), torch.tensor([1, 6, 0, 0, 0, 0])))
    refused(ValueError, r"neg_text_of_image\[2\] is the row's own index", negatives=(torch.tensor([1, 0, 0, 0, 0, 0]), torch.tensor([1, 2, 2, 0, 0, 0])))
    set_parity_mode(True, m)
    refused(ValueError, "parity precision mode is not built for the loss forward")
    set_parity_mode(False, m)
    set_compute_dtype("fp8", m)
    refused(ValueError, "fp8 is not built for the loss forward")
    set_compute_dtype("f16", m)
    big = pc.small_model(pc.Case("big", False, 513, 1, 64, 513, 0.07, (0.4,), (1,) * 513))
    with pytest.raises(ValueError, match="batch size 513 exceeds the 512 rows"):
        big.to(DEV)(torch.zeros(513, 3, 64, 64, device=DEV), ["w120"] * 513, 0.4)
    assert not launches
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    refused(NotImplementedError, "world size 2")
    assert all(torch.equal(t, m.state_dict()[k]) for k, t in state.items())
