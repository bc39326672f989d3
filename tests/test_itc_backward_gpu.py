"""``losses.itc_loss(...).backward()`` on the GPU against torch autograd in fp64 on the literal formula of the reference
(tests/itc_backward_cases.py), and the models' ``forward(..., grads=)``: the three gradients are ``itc_loss``'s on the features
the call reports, and everything else the call returns or changes has the bits of the call without ``grads``."""
import types

import pytest
import torch

import itc_backward_cases as ic
import pretrain_cases as pc
import retrieval_loss_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR = 2.0 ** -22


def bits(t):
    return t.contiguous().view(torch.int32)


def stores(queues, D):
    """The two row-major key buffers [QUEUE_HEAD + Q, D]: whatever lies in front of the queue and is not a call's batch is NaN."""
    from vidil_amd.losses import QUEUE_HEAD

    out = []
    for q in queues:
        s = torch.full((QUEUE_HEAD + q.shape[0], D), float("nan"), dtype=torch.float32, device=DEV)
        s[QUEUE_HEAD:] = q.to(DEV)
        out.append(s)
    return out


@pytest.mark.parametrize("B,D,Q,alpha", ic.CASES, ids=[f"b{B}_d{D}_q{Q}_a{a:g}" for B, D, Q, a in ic.CASES])
def test_itc_loss_backward_stays_within_four_times_f32_autograd_of_the_literal_formula(B, D, Q, alpha):
    """Reference: fp64 autograd of the literal formula on the same f32 features.  Bound per gradient: 4 x the error of the same
    literal formula under f32 torch autograd on the CPU, measured here, floored at 2^-22 x max |reference|.

    What makes the bound reachable in f32 is the centred form of the backward (losses.py): the positive class is left out of the
    kernel's sums, as autograd forms p - target before it multiplies."""
    from vidil_amd import losses
    from vidil_amd.blip_retrieval import BLIP_Retrieval

    feats, queues = ic.features(B, D, Q)
    want = ic.literal_grads(feats, queues, ic.TEMP, alpha, torch.float64)
    plain = ic.literal_grads(feats, queues, ic.TEMP, alpha, torch.float32)
    fi, ft, fim, ftm = (t.to(DEV) for t in feats)
    fi.requires_grad_(True)
    ft.requires_grad_(True)
    temp = torch.tensor(ic.TEMP, dtype=torch.float32, device=DEV, requires_grad=True)
    image_store, text_store = stores(queues, D)
    loss = losses.itc_loss(fi, ft, fim, ftm, image_store, text_store, temp, alpha, Q)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    assert fim.grad is None and ftm.grad is None
    got = (loss.detach(), fi.grad, ft.grad, temp.grad)
    assert got[1].shape == (B, D) and got[2].shape == (B, D) and got[3].shape == ()
    for name, g, w, p in zip(("loss", "image_feat", "text_feat", "temp"), got, want, plain):
        err = (g.double().cpu() - w).abs().max().item()
        measured = (p.double() - w).abs().max().item()
        bound = max(4 * measured, FLOOR * w.abs().max().item())
        print(f"{name}: error {err:.3e}, f32 autograd {measured:.3e}, bound {bound:.3e}, max |reference| {w.abs().max().item():.3e}")
        if name != "loss":                              # (the forward has its own bound in tests/test_retrieval_loss_gpu.py)
            assert torch.isfinite(g).all() and err <= bound, (name, err, bound)

    # the forward value is _itc_direction's, bit for bit (no autograd: the path the models take without grads=)
    me = types.SimpleNamespace(queue_size=Q)
    with torch.no_grad():
        t = temp.detach()
        rows_i2t, _ = BLIP_Retrieval._itc_direction(me, fi.detach(), fim, ftm, text_store, alpha, t)
        rows_t2i, _ = BLIP_Retrieval._itc_direction(me, ft.detach(), ftm, fim, image_store, alpha, t)
        assert not rows_i2t.requires_grad
        assert torch.equal(bits((rows_i2t.mean() + rows_t2i.mean()) / 2), bits(loss.detach()))


def _state(m, pointer):
    return dict(image_queue=m.image_queue.clone(), text_queue=m.text_queue.clone(), ptr=int(getattr(m, pointer)),
                temp=m.temp.detach().clone(), mom={n: p.detach().clone() for n, p in m.named_parameters() if "_m." in n})


def _same(a, b, what):
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        raw = lambda t: t if t.dtype == torch.bool else t.reshape(-1).contiguous().view(torch.uint8)      # (NaN == NaN)
        assert torch.equal(raw(a), raw(b)), what
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}/{k}")
    else:
        assert a == b, what


MODELS = [("retrieval", "image"), ("retrieval", "video"), ("pretrain", "image"), ("pretrain", "video")]


@pytest.mark.parametrize("kind,name", MODELS, ids=[f"{k}_{n}" for k, n in MODELS])
def test_the_models_fill_grads_with_itc_losss_gradients_and_change_nothing_else(kind, name):
    from vidil_amd import losses

    cases = rc if kind == "retrieval" else pc
    c = cases.case(name)
    pointer = "ptr_queue" if kind == "retrieval" else "queue_ptr"
    x, caps = cases.pixels(c, 0).to(DEV), cases.captions(c, 0)
    kw = dict(alpha=0.4, seed=cases.DRAW_SEEDS[c.name])
    if kind == "retrieval":
        kw["idx"] = torch.tensor(c.idx[0])
    runs = []
    for with_grads in (False, True):
        m = cases.small_model(c).to(DEV)
        before = [m._key_store(n).clone() for n in ("image_queue", "text_queue")]
        details, grads = {}, {}
        out = m(x, caps, details=details, **(dict(kw, grads=grads) if with_grads else kw))
        torch.cuda.synchronize()
        assert all(p.grad is None for p in m.parameters())
        runs.append(dict(out=tuple(out), details=dict(details), state=_state(m, pointer), grads=grads, before=before,
                         queue_size=m.queue_size))
    plain, run = runs
    _same(plain["out"], run["out"], "losses")
    _same(plain["details"], run["details"], "details")
    _same(plain["state"], run["state"], "state")
    _same(plain["before"], run["before"], "key stores before the call")

    g, d = run["grads"], run["details"]
    assert set(g) == {"image_feat", "text_feat", "temp"} and not plain["grads"]
    assert g["image_feat"].shape == g["text_feat"].shape == d["image_feat"].shape and g["temp"].shape == ()
    assert all(t.dtype == torch.float32 and not t.requires_grad and torch.isfinite(t).all() for t in g.values())
    assert g["image_feat"].abs().max() > 0 and g["text_feat"].abs().max() > 0 and g["temp"].abs() > 0
    fi, ft = d["image_feat"].clone().requires_grad_(True), d["text_feat"].clone().requires_grad_(True)
    temp = d["temp"].clone().requires_grad_(True)
    image_store, text_store = run["before"]
    loss = losses.itc_loss(fi, ft, d["image_feat_m"], d["text_feat_m"], image_store, text_store, temp, 0.4, run["queue_size"])
    loss.backward()
    assert torch.equal(bits(loss.detach()), bits(run["out"][0]))
    for k, t in (("image_feat", fi), ("text_feat", ft), ("temp", temp)):
        assert torch.equal(bits(t.grad), bits(g[k])), k
