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

Which gradients exist: those of ``loss_ita`` with respect to the online features and the temperature.  The projection heads, the
text stack and the ViT have no backward yet, and neither have the ITM and LM losses.
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
