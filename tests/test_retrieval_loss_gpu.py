"""The loss forward of BLIP_Retrieval / BLIP_Retrieval_Video on the GPU against the golden recorded from the reference's own
forward (tests/golden/make_retrieval_loss_golden.py), two consecutive calls per case, the reference's draws replayed through
``negatives=``."""
import math

import numpy as np
import pytest
import torch

import nlvr_cases as nc
import retrieval_loss_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDS = [c.name for c in rc.CASES]
U = 2.0 ** -24                                   # unit roundoff of f32

_runs = {}


def replay(c):
    """Both calls of a case with the golden's draws, run once and shared (read-only): per call the losses, ``details``, the
    similarities of the EXISTING forward(match_head='itc') before the call, and the state before / after."""
    if c.name in _runs:
        return _runs[c.name]
    from vidil_amd import kernels as K

    g = rc.golden()
    m = rc.small_model(c).to(DEV)
    calls = []
    for call in range(rc.CALLS):
        k = f"{c.name}/{call}/"
        x, caps = rc.pixels(c, call).to(DEV), rc.captions(c, call)
        before = dict(image_queue=m.image_queue.clone(), text_queue=m.text_queue.clone(), ptr=int(m.ptr_queue),
                      online={n: p.detach().clone() for n, p in m.named_parameters() if "_m." not in n},
                      mom={n: p.detach().clone() for n, p in m.named_parameters() if "_m." in n})
        if c.video:
            itc = K.scan_scores(m.video_features(x)[1], m.text_features(caps, DEV)[0])           # the existing features
        else:
            itc = m(x, caps, "itc")
        details = {}
        neg = (torch.from_numpy(g[k + "neg_image_of_text"]), torch.from_numpy(g[k + "neg_text_of_image"]))
        if c.video:                                            # the reference's positional order
            ita, itm = m(x, caps, c.alpha[call], torch.tensor(c.idx[call]), negatives=neg, details=details)
        else:                                                  # keywords, as the reference's training script passes them
            ita, itm = m(x, caps, alpha=c.alpha[call], idx=torch.tensor(c.idx[call]), negatives=neg, details=details)
        torch.cuda.synchronize()
        calls.append(dict(ita=ita, itm=itm, details={n: v.clone() for n, v in details.items()}, itc=itc, before=before,
                          after=dict(image_queue=m.image_queue.clone(), text_queue=m.text_queue.clone(),
                                     idx_queue=m.idx_queue.clone(), ptr=int(m.ptr_queue), temp=float(m.temp.detach()),
                                     mom={n: p.detach().clone() for n, p in m.named_parameters() if "_m." in n})))
    _runs[c.name] = (m, calls)
    return _runs[c.name]


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_the_new_arithmetic_alone_from_the_models_own_features_and_logits(c):
    """The features and ITM logits the model reports go through the fp64 restatement; the model's tower error does not enter.

    Bound of loss_ita.  The kernel's logits are f32 chains over D terms of q = f / t (one rounding) with unit-norm keys:
    |d logit| <= eps = (D + 2) u / t.  A row loss is lse(s) - alpha * sum_j softmax(m)_j s_j - (1 - alpha) s_diag.  lse is
    1-Lipschitz in the sup-norm of s: eps.  The middle term moves by at most eps with s (the weights sum to 1) and, with m, by
    eps * sum_k p_k |s_k - mean_p s| <= eps * (max s - min s) <= 2 eps / t.  The diagonal moves by eps.  In all
    eps * (2 + 2 alpha / t), plus the f32 roundings of exp / sum / log / the merges of the (max, sum, weighted sum) triples:
    32 u * (1 / t + log(B + Q)), a few roundings each of magnitudes bounded by the largest logit and the largest lse.
    loss_itm is torch's f32 cross-entropy of the reported logits: 16 u * max(1, max|logit|)."""
    m, calls = replay(c)
    for call, r in enumerate(calls):
        d = {n: v.cpu() for n, v in r["details"].items()}
        temp, alpha = float(d["temp"]), c.alpha[call]
        ita = rc.loss_ita64(d["image_feat"], d["text_feat"], d["image_feat_m"], d["text_feat_m"], r["before"]["image_queue"].cpu(),
                            r["before"]["text_queue"].cpu(), temp, alpha)
        eps = (rc.EMBED + 2) * U / temp
        tol = eps * (2 + 2 * alpha / temp) + 32 * U * (1 / temp + math.log(c.B + c.queue_size))
        print(f"{c.name} call {call}: loss_ita {float(r['ita']):.7f} restated {ita:.7f} |d| {abs(float(r['ita']) - ita):.2e} tol {tol:.2e}")
        assert r["ita"].dtype == torch.float32 and r["ita"].dim() == 0 and r["ita"].is_cuda
        assert abs(float(r["ita"]) - ita) <= tol
        itm = rc.loss_itm64(d["itm_logits"])
        assert d["itm_logits"].shape == (3 * c.B, 2) and r["itm"].dtype == torch.float32 and r["itm"].dim() == 0
        assert abs(float(r["itm"]) - itm) <= 16 * U * max(1.0, float(d["itm_logits"].abs().max()))
        # the in-batch similarities are the features' exact-f32 products over the clamped temperature
        sim = (d["image_feat"].double() @ d["text_feat"].double().T / temp)
        assert (d["sim_i2t"].double() - sim).abs().max() <= eps and torch.equal(d["sim_t2i"], d["sim_i2t"].T)


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_both_losses_end_to_end_against_the_references(c):
    """|loss_ita - golden| <= 4 delta / temp + 1e-5, delta the largest deviation of the EXISTING forward(match_head='itc')
    similarities (for the video class: the existing video / text features' products) from the golden's — lse and the target term
    are each 1-Lipschitz in the sup-norm of the logits, times 2 because the momentum targets move too.  |loss_itm - golden| <=
    2 * PRED_REL * max(1, max|logit|): the project's two-logit bound through a 2-Lipschitz cross-entropy."""
    g = rc.golden()
    m, calls = replay(c)
    for call, r in enumerate(calls):
        k = f"{c.name}/{call}/"
        temp = float(g[k + "temp"])
        delta = float((r["itc"].cpu() - torch.from_numpy(g[k + "sim"])).abs().max())
        e_ita, e_itm = abs(float(r["ita"]) - float(g[k + "loss_ita"])), abs(float(r["itm"]) - float(g[k + "loss_itm"]))
        b_itm = 2 * rc.PRED_REL * max(1.0, float(r["details"]["itm_logits"].abs().max()))
        print(f"{c.name} call {call}: delta {delta:.2e}; loss_ita off by {e_ita:.2e} (bound {4 * delta / temp + 1e-5:.2e}); "
              f"loss_itm off by {e_itm:.2e} (bound {b_itm:.2e})")
        assert e_ita <= 4 * delta / temp + 1e-5
        assert e_itm <= b_itm


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_the_state_after_each_call(c):
    g = rc.golden()
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
        assert a["idx_queue"].cpu().numpy().tolist() == g[k + "idx_queue"].tolist()
        ptr = (ptr + c.B) % c.queue_size
        assert a["ptr"] == ptr == int(g[k + "ptr_queue"][0])
        assert a["temp"] == pytest.approx(float(g[k + "temp"]), abs=1e-7) and 0.001 <= a["temp"] <= 0.5
        # the enqueued momentum features are the reference's within the project's hidden-state tolerance (16-bit towers)
        assert (a["image_queue"].cpu() - torch.from_numpy(g[k + "image_queue"])).abs().max() <= nc.HIDDEN_TOL
        # EMA: every momentum parameter = old * 0.995 + online * 0.005 to f32 rounding; two of them against the golden's
        for n, p in a["mom"].items():
            want = b["mom"][n].double() * rc.MOMENTUM + b["online"][n.replace("_m.", ".")].double() * (1 - rc.MOMENTUM)
            assert (p.double() - want).abs().max() <= 6 * U * max(1.0, float(want.abs().max())), n
        for n in ("vision_proj_m.weight", "text_proj_m.bias"):
            assert (a["mom"][n].cpu() - torch.from_numpy(g[k + n])).abs().max() <= 4 * U
    assert c.name != "image" or ptr == 0                       # the image case's queue wrapped


@pytest.mark.parametrize("c", rc.CASES, ids=IDS)
def test_own_draws_are_the_inverse_cdf_draws_of_the_reported_similarities(c):
    m = rc.small_model(c).to(DEV)
    x, caps = rc.pixels(c, 0).to(DEV), rc.captions(c, 0)
    idx = torch.tensor(c.idx[0])
    seen = []
    for _ in range(2):                                         # (the second call has other momentum weights; the draws depend
        d = {}                                                 # on the online features and the seed alone)
        if c.video:
            m(x, caps, 0.4, idx, seed=rc.DRAW_SEEDS[c.name], details=d)
        else:
            m(x, caps, alpha=0.4, idx=idx, seed=rc.DRAW_SEEDS[c.name], details=d)
        seen.append((d["neg_image_of_text"].cpu(), d["neg_text_of_image"].cpu()))
        excluded = 0
        for stream, name, sim in ((0, "neg_image_of_text", d["sim_t2i"]), (1, "neg_text_of_image", d["sim_i2t"])):
            want, close = rc.draws(sim, idx, rc.DRAW_SEEDS[c.name], stream)
            excluded += int(close.sum())
            assert torch.equal(d[name].cpu()[~close], want[~close]), (name, d[name], want)
            assert (idx[d[name].cpu()] != idx).all()
        assert excluded <= 1
    assert torch.equal(seen[0][0], seen[1][0]) and torch.equal(seen[0][1], seen[1][1])


def test_refusals_come_by_name_before_any_launch_or_mutation(monkeypatch):
    from vidil_amd.packing import set_compute_dtype, set_parity_mode

    c = rc.case("image")
    m = rc.small_model(c, momentum_state=False).to(DEV)
    x, caps, idx = rc.pixels(c, 0).to(DEV), rc.captions(c, 0), torch.tensor(c.idx[0])
    launches = []
    from vidil_amd import kernels as K
    monkeypatch.setattr(K, "gemm", lambda *a, **k: launches.append("gemm") or (_ for _ in ()).throw(AssertionError("launched")))

    def refused(exc, text, **kw):
        args = dict(alpha=0.4, idx=idx)
        args.update(kw)
        with pytest.raises(exc, match=text):
            m(args.pop("x", x), args.pop("caps", caps), **args)
        assert not launches and not m.has_momentum_state and float(m.temp.detach()) == pytest.approx(c.temp0)

    refused(ValueError, "queue_size=12 is not a multiple of the batch size 5", x=x[:5], caps=caps[:5], idx=idx[:5])
    refused(ValueError, "row 0 has no admissible negative", idx=torch.full((c.B,), 7))
    refused(ValueError, r"neg_text_of_image\[1\] names a sample of the same idx", negatives=(torch.tensor([1, 0, 0, 0, 0, 0]),
                                                                                              torch.tensor([1, 2, 0, 0, 0, 0])))
    set_parity_mode(True, m)
    refused(ValueError, "parity precision mode is not built for the loss forward")
    set_parity_mode(False, m)
    set_compute_dtype("fp8", m)
    refused(ValueError, "fp8 is not built for the loss forward")
    set_compute_dtype("f16", m)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    refused(NotImplementedError, "world size 2")
    monkeypatch.undo()
    # ... and a queue that is no multiple of the batch is refused by the enqueue itself as well
    m2 = rc.small_model(c)
    with pytest.raises(ValueError, match="queue_size=12 is not a multiple of the batch size 5"):
        m2._dequeue_and_enqueue(torch.zeros(5, rc.EMBED), torch.zeros(5, rc.EMBED), torch.arange(5))
