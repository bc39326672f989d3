"""``losses.linear_backward`` and the two head backwards on the GPU against fp64 of the same 16-bit operands.  The yardstick is
the project's own (tests/test_itc_backward_gpu.py): the error is at most 4 x the error of f32 torch on the CPU for the same
product, measured per case, with a floor of 2^-22 max|reference|."""
import pytest
import torch

from vidil_amd import losses as L

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
KIN = 768


def _within_yardstick(name, got, ref64, cpu32):
    err = (got.double().cpu() - ref64).abs().max().item()
    yard = (cpu32.double() - ref64).abs().max().item()
    floor = 2.0 ** -22 * ref64.abs().max().item()
    allowed = max(4.0 * yard, floor)
    print(f"{name}: error {err:.3e}, f32 CPU error {yard:.3e}, floor {floor:.3e}, error / allowed = {err / allowed if allowed else 0:.3f}")
    assert err <= allowed, (name, err, allowed)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("Nout", [2, 256])
@pytest.mark.parametrize("M", [1, 6, 33])
def test_linear_backward(M, Nout, dtype):
    g = torch.Generator().manual_seed(M * 1000 + Nout)
    dev = torch.device("cuda:0")
    x = torch.randn(M, KIN, generator=g).to(dtype)
    w = (torch.randn(Nout, KIN, generator=g) * 0.05).to(dtype)
    dy = torch.randn(M, Nout, generator=g) * 10.0 ** torch.empty(M, 1).uniform_(-7, -3, generator=g)
    dx, dw, db = L.linear_backward(dy.to(dev), x.to(dev), w.to(dev))
    torch.cuda.synchronize()
    assert dx.dtype == dw.dtype == db.dtype == torch.float32
    assert tuple(dx.shape) == (M, KIN) and tuple(dw.shape) == (Nout, KIN) and tuple(db.shape) == (Nout,)
    d64, x64, w64 = dy.double(), x.double(), w.double()
    _within_yardstick("dx", dx, d64 @ w64, dy @ w.float())
    _within_yardstick("dw", dw, d64.t() @ x64, dy.t() @ x.float())
    _within_yardstick("db", db, d64.sum(0), dy.sum(0))
    only_w = L.linear_backward(dy.to(dev), x.to(dev), w.to(dev), need_x=False, need_b=False)
    assert only_w[0] is None and only_w[2] is None and torch.equal(only_w[1], dw)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("frames", [1, 3])
def test_proj_head_backward_against_fp64_autograd(frames, dtype):
    """feat = normalize(mean_frames(cls · w^T + b)); upstream gradient of the size the ITC loss reports."""
    B, D = 6, 256
    g = torch.Generator().manual_seed(17 + frames)
    dev = torch.device("cuda:0")
    cls = torch.randn(B * frames, KIN, generator=g).to(dtype)
    w = (torch.randn(D, KIN, generator=g) * 0.03).to(dtype)
    b = torch.randn(D, generator=g) * 0.1
    up = torch.randn(B, D, generator=g) * 1e-3

    def chain(c, ww, bb, dt):
        p = c.to(dt) @ ww.to(dt).t() + bb.to(dt)
        return (torch.nn.functional.normalize(p.view(B, frames, D).mean(1), dim=-1) * up.to(dt)).sum()

    leaves64 = [t.double().requires_grad_(True) for t in (cls, w, b)]
    ref = torch.autograd.grad(chain(*leaves64, torch.float64), leaves64)
    leaves32 = [t.float().requires_grad_(True) for t in (cls, w, b)]
    cpu = torch.autograd.grad(chain(*leaves32, torch.float32), leaves32)
    got = L.proj_head_backward(up.to(dev), cls.to(dev), w.to(dev), b.to(dev))
    torch.cuda.synchronize()
    for name, a, r, c in zip(("dcls", "dw", "db"), got, ref, cpu):
        _within_yardstick(name, a, r, c)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_itm_head_backward_against_fp64_autograd(dtype):
    B = 6
    g = torch.Generator().manual_seed(5)
    dev = torch.device("cuda:0")
    cls = torch.randn(3 * B, KIN, generator=g).to(dtype)
    w = (torch.randn(2, KIN, generator=g) * 0.05).to(dtype)
    b = torch.randn(2, generator=g) * 0.1
    labels = torch.cat([torch.ones(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long)])
    logits = (cls.double() @ w.double().t() + b.double()).float()        # what the forward reported
    z64 = logits.double().requires_grad_(True)
    (dz,) = torch.autograd.grad(torch.nn.functional.cross_entropy(z64, labels), z64)
    dz32 = L.cross_entropy_backward(logits, labels)
    got = L.itm_head_backward(logits.to(dev), labels.to(dev), cls.to(dev), w.to(dev))
    torch.cuda.synchronize()
    _within_yardstick("dcls", got[0], dz @ w.double(), dz32 @ w.float())
    _within_yardstick("dw", got[1], dz.t() @ cls.double(), dz32.t() @ cls.float())
    _within_yardstick("db", got[2], dz.sum(0), dz32.sum(0))


# ------------------------------------------------------------------------------------------------ the models: head_grads=
from test_itc_backward_gpu import DEV, MODELS, _same, _state, bits   # noqa: E402  (the project's helpers, used as they are)

HEAD_KEYS = {"vision_proj.weight", "vision_proj.bias", "text_proj.weight", "text_proj.bias", "temp", "image_cls", "text_cls",
             "itm_head.weight", "itm_head.bias", "itm_cls"}
ALPHA = 0.4


def _run_model(kind, name):
    """Two calls on identical small models, without and with head_grads= (grads= and details= in both) -> (plain, run, model of
    the second call, inputs).  Computed once per class and shared by the tests below; nothing modifies it."""
    import itc_backward_cases  # noqa: F401
    import pretrain_cases as pc
    import retrieval_loss_cases as rc

    cases = rc if kind == "retrieval" else pc
    c = cases.case(name)
    pointer = "ptr_queue" if kind == "retrieval" else "queue_ptr"
    x, caps = cases.pixels(c, 0).to(DEV), cases.captions(c, 0)
    kw = dict(alpha=ALPHA, seed=cases.DRAW_SEEDS[c.name])
    if kind == "retrieval":
        kw["idx"] = torch.tensor(c.idx[0])
    runs = []
    for with_heads in (False, True):
        m = cases.small_model(c).to(DEV)
        before = [m._key_store(n).clone() for n in ("image_queue", "text_queue")]
        details, grads, heads = {}, {}, {}
        out = m(x, caps, details=details, grads=grads, **(dict(kw, head_grads=heads) if with_heads else kw))
        torch.cuda.synchronize()
        assert all(p.grad is None for p in m.parameters())
        runs.append(dict(out=tuple(out), details=dict(details), state=_state(m, pointer), grads=dict(grads), heads=heads,
                         before=before, queue_size=m.queue_size))
    return runs[0], runs[1], m, (x, caps)


_RUNS = {}


def _model_run(kind, name):
    if (kind, name) not in _RUNS:
        _RUNS[(kind, name)] = _run_model(kind, name)
    return _RUNS[(kind, name)]


def _operands(m, run, x, caps):
    """The 16-bit [CLS] rows and weights the call used, recomputed from the online towers (which a call does not change): the
    recomputed features and ITM logits must be the call's, bit for bit."""
    d = run["details"]
    B = d["image_feat"].shape[0]
    with torch.no_grad():
        p = m.packed()
        enc16, image_feat = m._visual_side(x, momentum=False)
        image_cls = m._image_cls_rows(enc16, x)
        ids, lens = m.tokenize(list(caps))
        t_eff = max(1, min(ids.shape[1], int(lens.max().item())))
        cap = {}
        text_feat = m.text_embeds(ids[:, :t_eff].to(DEV).contiguous(), lens.to(DEV).contiguous(), cap)
        logits, _ = m._itm_loss(enc16, B, ids, lens, d["neg_image_of_text"], d["neg_text_of_image"], cap)
        torch.cuda.synchronize()
    assert torch.equal(bits(image_feat), bits(d["image_feat"])) and torch.equal(bits(text_feat), bits(d["text_feat"]))
    assert torch.equal(bits(logits), bits(d["itm_logits"]))
    return dict(image_cls=image_cls.cpu(), text_cls=cap["text_cls"].cpu(), itm_cls=cap["itm_cls"].cpu(),
                vp_w=p["vp_w"].cpu(), vp_b=p["vp_b"].cpu(), tp_w=p["tp_w"].cpu(), tp_b=p["tp_b"].cpu(),
                itm_w=p["itm_w"].cpu(), itm_b=p["itm_b"].cpu())


def _feature(cls, w, b, B):
    """normalize(mean over a sample's frames of cls · w^T + b) in the dtype of the arguments."""
    proj = cls @ w.t() + b
    return torch.nn.functional.normalize(proj.view(B, -1, proj.shape[-1]).mean(1), dim=-1)


IDS = [f"{k}_{n}" for k, n in MODELS]


@pytest.mark.parametrize("kind,name", MODELS, ids=IDS)
def test_head_grads_changes_no_result_and_no_state(kind, name):
    plain, run, _, _ = _model_run(kind, name)
    _same(plain["out"], run["out"], "losses")
    _same(plain["details"], run["details"], "details")
    _same(plain["grads"], run["grads"], "grads")
    _same(plain["state"], run["state"], "state")
    _same(plain["before"], run["before"], "key stores before the call")
    assert set(run["grads"]) == {"image_feat", "text_feat", "temp"} and not plain["heads"]
    h = run["heads"]
    assert set(h) == HEAD_KEYS
    assert all(t.dtype == torch.float32 and not t.requires_grad and torch.isfinite(t).all() for t in h.values())
    assert all(t.abs().max() > 0 for t in h.values())
    assert torch.equal(bits(h["temp"]), bits(run["grads"]["temp"])) and h["temp"].shape == ()


@pytest.mark.parametrize("kind,name", MODELS, ids=IDS)
def test_head_grads_alone_and_shapes(kind, name):
    """head_grads= without grads=: the same head gradients; shapes are the parameters' and the [CLS] rows'."""
    import pretrain_cases as pc
    import retrieval_loss_cases as rc

    _, run, m_ref, (x, caps) = _model_run(kind, name)
    cases = rc if kind == "retrieval" else pc
    c = cases.case(name)
    kw = dict(alpha=ALPHA, seed=cases.DRAW_SEEDS[c.name])
    if kind == "retrieval":
        kw["idx"] = torch.tensor(c.idx[0])
    m = cases.small_model(c).to(DEV)
    heads = {}
    out = m(x, caps, head_grads=heads, **kw)
    torch.cuda.synchronize()
    _same(tuple(out), run["out"], "losses")
    _same(heads, run["heads"], "head_grads")
    B = run["details"]["image_feat"].shape[0]
    frames = x.shape[1] if x.dim() == 5 else 1
    for mod in ("vision_proj", "text_proj", "itm_head"):
        assert heads[f"{mod}.weight"].shape == getattr(m, mod).weight.shape
        assert heads[f"{mod}.bias"].shape == getattr(m, mod).bias.shape
    width = m.vision_proj.weight.shape[1]
    assert tuple(heads["image_cls"].shape) == (B * frames, width)
    assert tuple(heads["text_cls"].shape) == (B, m.text_proj.weight.shape[1])
    assert tuple(heads["itm_cls"].shape) == (3 * B, m.itm_head.weight.shape[1])
    if kind == "retrieval" and name == "image":         # (the one class whose forward also serves without the losses)
        with pytest.raises(TypeError, match="head_grads"):
            m(x, caps, head_grads={})


@pytest.mark.parametrize("kind,name", MODELS, ids=IDS)
def test_projection_head_grads_equal_the_fp64_backward_of_the_head_alone(kind, name):
    """Upstream: the grads["image_feat"] / ["text_feat"] the call reported; operands: the 16-bit [CLS] rows and weights it used."""
    _, run, m, (x, caps) = _model_run(kind, name)
    ops = _operands(m, run, x, caps)
    B = run["details"]["image_feat"].shape[0]
    h = run["heads"]
    for side, pre in (("image", "vp"), ("text", "tp")):
        up = run["grads"][f"{side}_feat"].cpu()
        res = {}
        for dt in (torch.float64, torch.float32):
            leaves = [ops[f"{side}_cls"].to(dt).requires_grad_(True), ops[f"{pre}_w"].to(dt).requires_grad_(True),
                      ops[f"{pre}_b"].to(dt).requires_grad_(True)]
            res[dt] = torch.autograd.grad((_feature(*leaves, B) * up.to(dt)).sum(), leaves)
        mod = "vision_proj" if side == "image" else "text_proj"
        for key, r64, r32 in zip((f"{side}_cls", f"{mod}.weight", f"{mod}.bias"), res[torch.float64], res[torch.float32]):
            _within_yardstick(f"{kind}_{name} {key}", h[key], r64, r32)


@pytest.mark.parametrize("kind,name", MODELS, ids=IDS)
def test_itm_head_grads_equal_fp64_autograd_of_the_cross_entropy_on_the_reported_logits(kind, name):
    _, run, m, (x, caps) = _model_run(kind, name)
    ops = _operands(m, run, x, caps)
    logits = run["details"]["itm_logits"].cpu()
    B = logits.shape[0] // 3
    labels = torch.cat([torch.ones(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long)])
    res = {}
    for dt in (torch.float64, torch.float32):
        z = logits.to(dt).requires_grad_(True)
        (dz,) = torch.autograd.grad(torch.nn.functional.cross_entropy(z, labels), z)
        res[dt] = (dz @ ops["itm_w"].to(dt), dz.t() @ ops["itm_cls"].to(dt), dz.sum(0))
    h = run["heads"]
    for key, r64, r32 in zip(("itm_cls", "itm_head.weight", "itm_head.bias"), res[torch.float64], res[torch.float32]):
        _within_yardstick(f"{kind}_{name} {key}", h[key], r64, r32)


@pytest.mark.parametrize("kind,name", MODELS, ids=IDS)
def test_head_grads_end_to_end_against_fp64_autograd_of_the_literal_chain(kind, name):
    """[CLS] rows -> projection -> (mean of frames) -> normalize -> the literal loss_ita of itc_backward_cases."""
    import itc_backward_cases as ic
    from vidil_amd.losses import QUEUE_HEAD

    _, run, m, (x, caps) = _model_run(kind, name)
    ops = _operands(m, run, x, caps)
    d = run["details"]
    B, Q = d["image_feat"].shape[0], run["queue_size"]
    queues = [s[QUEUE_HEAD:QUEUE_HEAD + Q].cpu() for s in run["before"]]
    res = {}
    for dt in (torch.float64, torch.float32):
        names = ("image_cls", "vp_w", "vp_b", "text_cls", "tp_w", "tp_b")
        leaves = [ops[n].to(dt).requires_grad_(True) for n in names]
        temp = d["temp"].cpu().to(dt).requires_grad_(True)
        loss = ic.literal_loss(_feature(*leaves[:3], B), _feature(*leaves[3:], B), d["image_feat_m"].cpu().to(dt),
                               d["text_feat_m"].cpu().to(dt), queues[0].to(dt), queues[1].to(dt), temp, ALPHA)
        res[dt] = torch.autograd.grad(loss, leaves + [temp])
    keys = ("image_cls", "vision_proj.weight", "vision_proj.bias", "text_cls", "text_proj.weight", "text_proj.bias", "temp")
    for key, r64, r32 in zip(keys, res[torch.float64], res[torch.float32]):
        _within_yardstick(f"{kind}_{name} end to end {key}", run["heads"][key], r64, r32)
