"""The literal ITC loss of the reference (models/blip_retrieval.py:108-141: materialised similarity matrices, `log_softmax x
targets`) for torch autograd in any float type, the analytic gradients the fused backward implements, and the features of
tests/test_itc_backward_gpu.py.  Shared by tests/test_scan_grad_cpu.py (fp64, no GPU) and tests/test_itc_backward_gpu.py."""
from functools import lru_cache

import torch
import torch.nn.functional as F

BATCHES, WIDTHS, QUEUES, ALPHAS = (1, 6, 17, 33), (64, 256), (12, 257), (0.0, 0.4, 1.0)
CASES = [(B, D, Q, alpha) for B in BATCHES for D in WIDTHS for Q in QUEUES for alpha in ALPHAS]
TEMP = 0.07


def literal_loss(image_feat, text_feat, image_feat_m, text_feat_m, image_queue, text_queue, temp, alpha):
    """loss_ita as the reference writes it.  image_queue / text_queue: [queue, D] rows (the reference keeps them as columns);
    the momentum features, the queues and the targets carry no gradient."""
    with torch.no_grad():
        image_all = torch.cat([image_feat_m, image_queue]).t()
        text_all = torch.cat([text_feat_m, text_queue]).t()
        sim_i2t_m = image_feat_m @ text_all / temp
        sim_t2i_m = text_feat_m @ image_all / temp
        hard = torch.zeros_like(sim_i2t_m)
        hard.fill_diagonal_(1)
        i2t_targets = alpha * F.softmax(sim_i2t_m, dim=1) + (1 - alpha) * hard
        t2i_targets = alpha * F.softmax(sim_t2i_m, dim=1) + (1 - alpha) * hard
    sim_i2t = image_feat @ text_all / temp
    sim_t2i = text_feat @ image_all / temp
    loss_i2t = -torch.sum(F.log_softmax(sim_i2t, dim=1) * i2t_targets, dim=1).mean()
    loss_t2i = -torch.sum(F.log_softmax(sim_t2i, dim=1) * t2i_targets, dim=1).mean()
    return (loss_i2t + loss_t2i) / 2


def literal_grads(feats, queues, temp, alpha, dtype):
    """(loss, d/d image_feat, d/d text_feat, d/d temp) of the literal formula under torch autograd on the CPU in ``dtype``."""
    fi, ft, fim, ftm = (t.detach().cpu().to(dtype) for t in feats)
    qi, qt = (t.detach().cpu().to(dtype) for t in queues)
    fi.requires_grad_(True)
    ft.requires_grad_(True)
    t = torch.tensor(float(temp), dtype=dtype, requires_grad=True)
    loss = literal_loss(fi, ft, fim, ftm, qi, qt, t, alpha)
    g = torch.autograd.grad(loss, (fi, ft, t))
    return loss.detach(), g[0], g[1], g[2]


def analytic_direction(a, a_m, keys, temp, alpha):
    """The analytic gradients (vidil_amd/losses.py) of one direction, in the dtype of the arguments: (d mean_b L_b / d a, d mean_b L_b / d temp, the latter
    once more as -(1/t) sum_b (a_b / t) · (t dL_b/da_b), the former
    once more in the centred form the backward evaluates).
    keys [n, D]: the other modality's momentum batch features followed by the queue."""
    B = a.shape[0]
    s, m = a @ keys.t() / temp, a_m @ keys.t() / temp
    es = torch.exp(s - torch.logsumexp(s, 1, keepdim=True))
    em = torch.exp(m - torch.logsumexp(m, 1, keepdim=True))
    G = (es - alpha * em) @ keys                                     # scan_softmax_grad's G with cv = 1, cw = alpha
    T = (es * s).sum(1)                                              # and its T
    soft, diag = (em * s).sum(1), s.diagonal()
    g_a = (G - (1 - alpha) * keys[:B]) / temp / B
    g_t = -((T - alpha * soft - (1 - alpha) * diag) / temp).sum() / B
    g_t_dot = -((a / temp) * (G - (1 - alpha) * keys[:B])).sum() / temp / B          # the form the backward evaluates
    c = (es - alpha * em).clone()
    c[torch.arange(B), torch.arange(B)] = 0                          # the positive left out: scan_softmax_grad's hard class
    g_a_centred = (c @ keys - c.sum(1, keepdim=True) * keys[:B]) / temp / B          # sum_{j != b} c_j (K_j - K_b)
    return g_a, g_t, g_t_dot, g_a_centred


@lru_cache(maxsize=None)
def features(B, D, Q):
    """Unit-norm f32 features (image, text, momentum image, momentum text) [B,D] and the two queues [Q,D]: a momentum row is its
    student row slightly turned, and a text row leans on its image row, so that the diagonal carries weight.  Read-only."""
    g = torch.Generator().manual_seed(1000 * B + 10 * D + Q)
    unit = lambda x: F.normalize(x, dim=1)
    fi = unit(torch.randn(B, D, generator=g))
    ft = unit(fi + 0.8 * unit(torch.randn(B, D, generator=g)))
    fim = unit(fi + 0.1 * unit(torch.randn(B, D, generator=g)))
    ftm = unit(ft + 0.1 * unit(torch.randn(B, D, generator=g)))
    qi, qt = unit(torch.randn(Q, D, generator=g)), unit(torch.randn(Q, D, generator=g))
    return (fi, ft, fim, ftm), (qi, qt)
