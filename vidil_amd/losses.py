"""The differentiable image-text contrastive (ITC) loss over batch + queue (models/blip_retrieval.py:108-141, the same
statements in models/blip_pretrain.py:123-138) on the two fused forms of the exact-f32 scan.

One direction, for row b, with s_j = a_b·K_j / t (student row), m_j = g_b·K_j / t (momentum row) and K the other modality's
momentum batch features followed by the queue (both under ``no_grad`` in the reference):

    L_b = lse(s) - alpha * sum_j softmax(m)_j s_j - (1 - alpha) * s_b

Gradient reaches the student rows a (through s) and the temperature t only:

    dL_b/ds_j = softmax(s)_j - alpha softmax(m)_j - (1 - alpha) [j == b]
    dL_b/da   = (1/t) [ sum_j (e^{s_j - lse s} - alpha e^{m_j - lse m}) K_j - (1 - alpha) K_b ]
              = (1/t) sum_{j != b} c_j (K_j - K_b),  c_j = e^{s_j - lse s} - alpha e^{m_j - lse m}     (sum_j dL_b/ds_j = 0)
    dL_b/dt   = -(1/t) [ sum_j e^{s_j - lse s} s_j - alpha * sum_j softmax(m)_j s_j - (1 - alpha) s_b ]
              = -(1/t) (a_b / t) · (t dL_b/da)              (s is linear in a / t; the form the backward evaluates)

The forward is ``kernels.scan_softmax_stats`` (no [B, B + queue] matrix); the backward is ONE ``kernels.scan_softmax_grad`` call
per direction with cv = 1, cw = alpha (each times 1 - the rounding error of its row's f32 log-sum-exp) and the row's positive b
as the hard class, which reads the keys once more and returns G = sum_{j != b} c_j K_j and C = sum_{j != b} c_j (no matrix
either); dL_b/dq = G - C K_b is the second form of dL/da above.  Then [B]- and [B, D]-sized torch ops apply 1/t, the temperature
and the upstream gradient.  The kernel's output T_b = sum_j e^{s_j - lse s} s_j gives dL/dt by the first form above; the
backward takes the second, which does not subtract three f32 numbers of the size of a score.

Which gradients exist: those of ``loss_ita`` with respect to the online features and the temperature (above), and the backward of
the heads on top of the two losses that have a forward: ``linear_backward`` (dX = dY · W and dW = dY^T · X on the backward forms
of the GEMM, ``kernels.gemm_grad_input`` / ``gemm_grad_weight``), ``proj_head_backward`` (vision_proj / text_proj under the
normalisation, from a gradient at the unit-norm feature to the head's parameters and its [CLS] input rows) and
``itm_head_backward`` (the two-class cross-entropy to itm_head's parameters and its [CLS] rows).  The four loss models report
them through ``forward(..., head_grads={})``; the text stack, the ViT and the LM loss have no backward.
"""
from __future__ import annotations

import torch

from . import kernels as K

QUEUE_HEAD = 512     # rows of a key buffer in front of the queue (a multiple of 32): a call's batch features live in rows [0, B)


def _two_sum_error(a, b, s):
    """e with a + b == s + e exactly, for s = fl(a + b) (Knuth's two-sum; f32 tensors)."""
    bb = s - a
    return (a - (s - bb)) + (b - bb)


class ItcDirection(torch.autograd.Function):
    """One direction of the soft-target contrastive loss -> (f32 [B] row losses, f32 [B,B] the student rows against the batch's
    momentum keys over temp — the block the diagonal is read from; not differentiable).  a, a_m: the student and the momentum
    rows [B, D] (unit norm); keys_m: the other modality's momentum batch features, written to rows [0, B) of ``store``, whose queue
    segment starts at QUEUE_HEAD.  Differentiable in ``a`` and ``temp``.  The backward reads ``store`` again (after putting
    ``keys_m`` back into its first rows): it must run before the queue rows change, as the reference's backward sees the
    similarity matrices of the queue as it was."""

    @staticmethod
    def forward(ctx, a, a_m, keys_m, store, alpha, temp, queue_size):
        B = a.shape[0]
        store[:B] = keys_m
        q, q_m = (a / temp).contiguous(), (a_m / temp).contiguous()
        st, _ = K.scan_softmax_stats(q, q_m, store, [0, QUEUE_HEAD], [B, queue_size])              # [B, 2, 5]
        m, mw = st[..., 0].amax(1, keepdim=True), st[..., 2].amax(1, keepdim=True)
        ev, ew = torch.exp(st[..., 0] - m), torch.exp(st[..., 2] - mw)
        log_sum = torch.log((st[..., 1] * ev).sum(1))
        lse = m[:, 0] + log_sum
        soft = (st[..., 4] * ew).sum(1) / (st[..., 3] * ew).sum(1)                              # sum_j softmax(m)_j s_j
        block = K.scan_scores(q, store[:B])
        diag = block.diagonal()
        ctx.alpha, ctx.queue_size, ctx.store = alpha, queue_size, store
        ctx.save_for_backward(q, q_m, keys_m, temp, m[:, 0], log_sum, lse, st)
        ctx.mark_non_differentiable(block)
        return lse - alpha * soft - (1.0 - alpha) * diag, block

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rows, _g_block):
        q, q_m, keys_m, temp, m, log_sum, lse, st = ctx.saved_tensors
        alpha, store = ctx.alpha, ctx.store
        B = q.shape[0]
        store[:B] = keys_m
        mw = st[..., 2].amax(1)
        log_sum_m = torch.log((st[..., 3] * torch.exp(st[..., 2] - mw[:, None])).sum(1))
        lse_m = mw + log_sum_m
        # The kernel takes exp(s - lse) with lse in f32, whose rounding (half an ulp of ~14 at temp 0.07) would scale a whole
        # softmax row.  lse = fl(max + log_sum); the rounding error of that one addition is itself an f32 number (two_sum), and
        # exp(-error) = 1 - error goes into the row's coefficient: the softmax is then as exact as log_sum, as in log_softmax.
        cv = 1.0 - _two_sum_error(m, log_sum, lse)
        cw = alpha * (1.0 - _two_sum_error(mw, log_sum_m, lse_m))
        # dL_b/dq_b = sum_j g_j K_j with g_j = p_j - alpha pm_j - (1 - alpha) [j == b] and sum_j g_j = 0, hence
        # = sum_{j != b} c_j (K_j - K_b): the kernel leaves class b out and returns G = sum_{j != b} c_j K_j and C = sum_{j != b} c_j.
        # Neither c_b K_b (of the size of K_b when the row is peaked on its positive) nor (1 - alpha) K_b is formed and cancelled,
        # and an error of a row's normalisation scales the small terms only — what autograd gets by forming p - target first.
        hard = torch.arange(B, dtype=torch.int32, device=q.device)
        G, _, C = K.scan_softmax_grad(q, q_m, store, [0, QUEUE_HEAD], [B, ctx.queue_size], lse, lse_m, cv, cw, hard=hard)
        d_q = G - C[:, None] * keys_m                                     # dL_b/dq_b, q = a / temp
        g_a = g_temp = None
        if ctx.needs_input_grad[0]:
            g_a = d_q * (g_rows / temp)[:, None]
        if ctx.needs_input_grad[5]:
            # dL_b/dt = -(1/t) sum_j dL_b/ds_j s_j, and s_j = q_b·K_j, so the sum is q_b · dL_b/dq_b: the same number as
            # T - alpha soft - (1 - alpha) s_b with the kernel's T, without the cancellation of three f32 numbers of the size of
            # a score (an ulp of ~10, over temp, is more than the whole error of f32 autograd on the literal formula).
            g_temp = -(((q * d_q).sum(1) * g_rows).sum() / temp)
        return g_a, None, None, None, None, g_temp, None


def itc_terms(image_feat, text_feat, image_feat_m, text_feat_m, image_store, text_store, temp, alpha, queue_size):
    """(loss_ita, loss_i2t, loss_t2i, sim_i2t, sim_t2i): both directions, their means, and the [B,B] blocks of the student rows
    against the batch's momentum features over temp."""
    rows_i2t, sim_i2t = ItcDirection.apply(image_feat, image_feat_m, text_feat_m, text_store, alpha, temp, queue_size)
    rows_t2i, sim_t2i = ItcDirection.apply(text_feat, text_feat_m, image_feat_m, image_store, alpha, temp, queue_size)
    loss_i2t, loss_t2i = rows_i2t.mean(), rows_t2i.mean()
    return (loss_i2t + loss_t2i) / 2, loss_i2t, loss_t2i, sim_i2t, sim_t2i


def itc_loss(image_feat, text_feat, image_feat_m, text_feat_m, image_store, text_store, temp, alpha, queue_size):
    """``loss_ita`` (0-dim f32) of f32 [B, D] unit-norm features; image_store / text_store: the row-major key buffers
    [QUEUE_HEAD + queue_size, D] of the image and the text queue (``BLIP_Retrieval._key_store``), whose first B rows the call
    overwrites with the momentum batch features; temp: 0-dim f32 tensor; alpha: float.  Differentiable with respect to
    ``image_feat``, ``text_feat`` and ``temp``; every other argument receives no gradient (the reference computes the momentum
    features, the queues and the soft targets under ``no_grad``).  Call ``backward`` before the queue rows change."""
    return itc_terms(image_feat, text_feat, image_feat_m, text_feat_m, image_store, text_store, temp, alpha, queue_size)[0]


def itc_terms_with_grads(grads, image_feat, text_feat, image_feat_m, text_feat_m, image_store, text_store, temp, alpha, queue_size):
    """``itc_terms`` (detached) for a model's forward; ``grads`` (dict) receives ``image_feat``, ``text_feat`` f32 [B, D] and
    ``temp`` (0-dim f32): the gradients of ``loss_ita`` only, with respect to the online features and the temperature.  Nothing
    is written to any ``.grad``."""
    with torch.enable_grad():
        leaves = [t.detach().clone().requires_grad_(True) for t in (image_feat, text_feat, temp)]
        terms = itc_terms(leaves[0], leaves[1], image_feat_m, text_feat_m, image_store, text_store, leaves[2], alpha, queue_size)
        g = torch.autograd.grad(terms[0], leaves)
    grads.update(image_feat=g[0], text_feat=g[1], temp=g[2])
    return tuple(t.detach() for t in terms)


# ------------------------------------------------------------------------------------------------ head backward
SPLIT_EXP = 10       # a scaled slice's largest magnitude lies in [2^10, 2^11): f16's third plane then stays above its subnormals


def split3_planes(v32, dtype, dim):
    """Exact three-plane split of f32 ``v32`` [R, C] into 16-bit operands: -> (hi, mid, lo, inv_scale) with
    (hi + mid + lo) * inv_scale == v32, hi = T16(v), mid = T16(v - hi), lo = T16(v - hi - mid) of v = v32 * scale.  The scale is one
    power of two per row (dim=1: inv_scale [R, 1]) or per column (dim=0: inv_scale [1, C]) that puts the slice's largest magnitude
    into [2^10, 2^11) — gradients are 1e-3 .. 1e-7, where f16's third plane would underflow —, so scaling and unscaling are
    exact.  bf16: 3 x 8 = 24 bits, exact for every f32; f16: 33 bits, exact for every element of at least 2^-12 of its slice's
    largest (the third plane's ulp meets f16's smallest subnormal 2^-24 there)."""
    amax = v32.abs().amax(dim=dim, keepdim=True)
    _, e = torch.frexp(amax)                                     # amax = m * 2^e, m in [0.5, 1)
    k = torch.where(amax > 0, SPLIT_EXP + 1 - e, torch.zeros_like(e)).clamp_(-120, 120)
    one = torch.ones_like(amax)
    v = v32 * torch.ldexp(one, k)
    hi = v.to(dtype)
    r = v - hi.float()
    mid = r.to(dtype)
    lo = (r - mid.float()).to(dtype)
    return hi, mid, lo, torch.ldexp(one, -k)


def _pad8(n):
    return (n + 7) // 8 * 8


def linear_backward(dy32, x16, w16, *, need_x=True, need_w=True, need_b=True):
    """Backward of ``y = x16 · w16^T + b`` as the library's forward computes it -> (dx f32 [M, Kin], dw f32 [Nout, Kin], db f32
    [Nout]); entries not asked for are None.  dy32 f32 [M, Nout]; x16 [M, Kin] and w16 [Nout, Kin]: the 16-bit tensors the forward
    GEMM read, exact operands.  Only dy32 has to become 16-bit: its three exact planes (``split3_planes``) are concatenated along
    the contraction axis — columns [hi | mid | lo] against [W; W; W] for dx, row blocks [hi; mid; lo] against [X; X; X] for dw,
    the contraction padded with zeros to a multiple of 8 where the form needs it — so the error left is the f32 accumulation's.
    db = dy32.sum(0), accumulated in f64."""
    M, Nout = dy32.shape
    Kin = w16.shape[1]
    T = w16.dtype
    if dy32.dtype != torch.float32 or x16.dtype != T or tuple(x16.shape) != (M, Kin) or w16.shape[0] != Nout:
        raise K.VidilHipError(f"linear_backward: dy f32 [M, Nout], x [M, Kin] and w [Nout, Kin] of one 16-bit type expected, got "
                              f"{dy32.dtype} {tuple(dy32.shape)}, {x16.dtype} {tuple(x16.shape)}, {w16.dtype} {tuple(w16.shape)}")
    dev = dy32.device
    Np = _pad8(Nout)
    dx = dw = db = None
    if need_x:
        hi, mid, lo, inv = split3_planes(dy32, T, 1)                    # one scale per row of dy: a row of dx
        a = torch.zeros((M, 3 * Np), dtype=T, device=dev)
        w3 = torch.zeros((3 * Np, Kin), dtype=T, device=dev)
        for i, plane in enumerate((hi, mid, lo)):
            a[:, i * Np:i * Np + Nout] = plane
            w3[i * Np:i * Np + Nout] = w16
        dx = K.gemm_grad_input(a, w3) * inv
    if need_w:
        hi, mid, lo, inv = split3_planes(dy32, T, 0)                    # one scale per column of dy: a row of dw
        a = torch.zeros((3 * M, Np), dtype=T, device=dev)
        for i, plane in enumerate((hi, mid, lo)):
            a[i * M:(i + 1) * M, :Nout] = plane
        x3 = torch.cat([x16, x16, x16], 0).contiguous()
        dw = K.gemm_grad_weight(a, x3)[:Nout] * inv.reshape(Nout, 1)
    if need_b:
        db = dy32.double().sum(0).float()
    return dx, dw, db


def normalize_backward(g, p):
    """Gradient at the un-normalised rows p of f = p / ||p|| given g = dL/df: (g - f (f·g)) / ||p||."""
    n = p.norm(dim=-1, keepdim=True)
    f = p / n
    return (g - f * (f * g).sum(-1, keepdim=True)) / n


def cross_entropy_backward(logits, labels):
    """d mean-cross-entropy / d logits = (softmax - onehot) / rows."""
    d = torch.softmax(logits, dim=-1)
    d[torch.arange(logits.shape[0], device=logits.device), labels] -= 1.0
    return d / logits.shape[0]


def proj_head_backward(g_feat, cls16, w16, b32, *, need_x=True):
    """Backward of ``feat = normalize(mean_frames(cls16 · w16^T + b32))`` (vision_proj / text_proj under the ITC loss) ->
    (dcls f32 [B*N, width], dw f32, db f32).  g_feat f32 [B, D]: the gradient at the unit-norm feature (``grads["image_feat"]``);
    cls16 [B*N, width]: the 16-bit [CLS] rows the head read, N >= 1 frames per sample in sample-major order (N = 1: no mean).  The
    un-normalised projection is recomputed with the forward's GEMM; every frame's row receives 1/N of its sample's gradient."""
    B, D = g_feat.shape
    rows = cls16.shape[0]
    if rows % B:
        raise K.VidilHipError(f"proj_head_backward: {rows} [CLS] rows for {B} features")
    N = rows // B
    cls16 = cls16.contiguous()
    p = K.gemm(cls16, w16, b32, out=torch.empty((rows, D), dtype=torch.float32, device=cls16.device))
    g_p = normalize_backward(g_feat, p.view(B, N, D).mean(dim=1) if N > 1 else p)
    dy = (g_p / N).repeat_interleave(N, dim=0).contiguous() if N > 1 else g_p.contiguous()
    return linear_backward(dy, cls16, w16, need_x=need_x)


def itm_head_backward(logits32, labels, cls16, w16, *, need_x=True):
    """Backward of ``cross_entropy(cls16 · w16^T + b, labels)`` over the pairs of the matching loss -> (dcls f32 [P, width], dw f32
    [2, width], db f32 [2]); logits32 f32 [P, 2] as the forward reported them."""
    return linear_backward(cross_entropy_backward(logits32.float(), labels).contiguous(), cls16.contiguous(), w16, need_x=need_x)
