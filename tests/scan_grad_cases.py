"""Cases of the gradient form of the scan (`vidil_scan_topk` with `topk == VIDIL_SCAN_FORM_GRAD`, `kernels.scan_softmax_grad`),
shared by tests/test_scan_grad_cpu.py (inputs, reference and bounds, no GPU) and tests/test_scan_grad_gpu.py.

Per pair p, over the classes j of ALL segments together, with v_j = values[p]·keys[j] and w_j = weights[p]·keys[j]:

    c_j = cv[p] exp(v_j - lv[p]) - cw[p] exp(w_j - lw[p]),    G[p,:] = sum_j c_j keys[j,:],    T[p] = sum_j exp(v_j - lv[p]) v_j,
    C[p] = sum_j c_j;  a pair's hard class h[p] (a class of the first segment; -1: none) is left out of G and C, not of T.

Rows and keys are those of tests/scan_stats_cases.py (`inputs`), at its shapes and at the key counts around the gradient form's
split of a segment into runs of 1024 classes (1023 / 1024 / 1025).  lv, lw are the fp64 log-sum-exp of v and w rounded to f32.
The expected values are G and T in fp64 on the f32 inputs (`reference`).

Bounds (`BOUNDS`): per case and per output, 4 x the error against fp64 of a plain f32 computation of the same formula on the CPU
(`plain_f32`: both contractions as one rounded multiply and one rounded add per term, torch's exp and sum), the factor being for
the kernel's other order of summation (fma chains, waves and splits added in fixed order); recorded at 3.8 x the measurement
with the measurement beside it, and floored at 2^-22 x max |reference| of that output.  tests/test_scan_grad_cpu.py recomputes
the measurement and asserts 2 x <= bound <= 4 x, or bound == floor.
"""
from dataclasses import dataclass
from functools import lru_cache

import torch

import scan_stats_cases as sc

SPLIT = 32 * sc.TILE     # classes per key split (scan.hip: GT * 32)
FORM = -2                # VIDIL_SCAN_FORM_GRAD (include/vidil_hip.h)
OUTPUTS = ("G", "T", "C")
FLOOR = 2.0 ** -22


@dataclass(frozen=True)
class Case:
    base: sc.Case
    cv: float            # coefficient of exp(v - lv)
    cw: float            # coefficient of exp(w - lw)
    per_p: bool = False  # cv, cw are divided by P and vary from pair to pair: x (1 + (p % 5) / 4)
    hard: bool = False   # pair p leaves class (7 p + 3) % (length of the first segment) out (the batch layout: class p, its own)

    @property
    def name(self):
        return f"{self.base.name}_cv{self.cv:g}_cw{self.cw:g}" + ("_perp" if self.per_p else "") + ("_hard" if self.hard else "")


_COEF = [(1.0, 0.4, False), (1.0, 0.0, False), (1.0, 1.0, False), (0.5, 0.2, True)]
_SPLIT_EDGE = [
    # one below, at, one above the split of a segment; and the queue layout with a split edge inside the queue segment
    sc.Case("d64_p17_c1023", 64, 17, SPLIT - 1, 0.07),
    sc.Case("d256_p16_c1024", 256, 16, SPLIT, 0.07),
    sc.Case("d64_p33_c1025", 64, 33, SPLIT + 1, 0.07),
    sc.Case("d8_p1_c1025", 8, 1, SPLIT + 1, 0.001),
    sc.Case("spiked_d256_p17_c1025_t07", 256, 17, SPLIT + 1, 0.07, spiked=True),
    sc.Case("batch_d256_p33_q1025_t07", 256, 33, SPLIT + 1, 0.07, batch=True),
]
CASES = [Case(b, *_COEF[i % 4]) for i, b in enumerate(list(sc.CASES) + _SPLIT_EDGE)]
# a hard class per pair: every batch layout (the loss's use) and single segments across the tile, chunk and split edges
_HARD = ("d64_p17_c32", "d256_p16_c257", "spiked_d64_p33_c257_t07", "d64_p33_c1025")
CASES += [Case(c.base, c.cv, c.cw, c.per_p, hard=True) for c in list(CASES) if c.base.batch or c.base.name in _HARD]


@lru_cache(maxsize=None)
def scores64(c):
    """v, w f64 [P, n] over the classes of all segments in order, and the keys of those classes f64 [n, D]."""
    val, wgt, keys, seg_start, seg_len = sc.inputs(c.base)
    k = torch.cat([keys[s0:s0 + n] for s0, n in zip(seg_start, seg_len)]).double()
    return val.double() @ k.T, wgt.double() @ k.T, k


@lru_cache(maxsize=None)
def inputs(c):
    """values, weights, keys, seg_start, seg_len as scan_stats_cases.inputs, then lv, lw, cv, cw f32 [P] and hard i32 [P].
    Read-only."""
    val, wgt, keys, seg_start, seg_len = sc.inputs(c.base)
    v, w, _ = scores64(c)
    P = val.shape[0]
    lv, lw = torch.logsumexp(v, 1).float(), torch.logsumexp(w, 1).float()
    ramp = (1 + (torch.arange(P) % 5) / 4) / P if c.per_p else torch.ones(P)
    cv, cw = (c.cv * ramp).float(), (c.cw * ramp).float()
    p = torch.arange(P)
    hard = (p if c.base.batch else (7 * p + 3) % seg_len[0]) if c.hard else torch.full((P,), -1)
    return val, wgt, keys, seg_start, seg_len, lv, lw, cv, cw, hard.to(torch.int32)


def formula(v, w, k, lv, lw, cv, cw, hard, contract):
    """G, T, C from score matrices v, w [P, n] and keys k [n, D] of any float type (the first segment's classes come first in
    n, so a hard class is its own column)."""
    ev, ew = torch.exp(v - lv[:, None]), torch.exp(w - lw[:, None])
    coef = cv[:, None] * ev - cw[:, None] * ew
    coef = torch.where(torch.arange(v.shape[1])[None, :] == hard[:, None].long(), torch.zeros_like(coef), coef)
    return contract(coef, k), (ev * v).sum(1), coef.sum(1)


@lru_cache(maxsize=None)
def reference(c):
    """fp64 on the f32 inputs: (G f64 [P,D], T f64 [P], C f64 [P])."""
    lv, lw, cv, cw = (t.double() for t in inputs(c)[5:9])
    v, w, k = scores64(c)
    return formula(v, w, k, lv, lw, cv, cw, inputs(c)[9], lambda a, b: a @ b)


def plain_f32(c):
    val, wgt, keys, seg_start, seg_len, lv, lw, cv, cw, hard = inputs(c)
    k = torch.cat([keys[s0:s0 + n] for s0, n in zip(seg_start, seg_len)])
    return formula(sc._dot32(val, k), sc._dot32(wgt, k), k, lv, lw, cv, cw, hard, lambda a, b: sc._dot32(a, b.T.contiguous()))


def floors(c):
    return [FLOOR * r.abs().max().item() for r in reference(c)]


def measured_error(c):
    """max |plain f32 - fp64| per output -> 3 floats."""
    return [(a.double() - r).abs().max().item() for a, r in zip(plain_f32(c), reference(c))]


def errors(c, G, T, C):
    return [(a.double().cpu() - r).abs().max().item() for a, r in zip((G, T, C), reference(c))]


def bounds(c):
    """The bound per output: the recorded one, or the floor where that is larger."""
    return [max(b, f) for b, f in zip(BOUNDS[c.name][0], floors(c))]


# name -> ((bound per output), (the CPU measurement it was taken from)); bound = 3.8 x measurement.  Written by `python
# tests/scan_grad_cases.py`, which prints this table from `measured_error`.
BOUNDS = {
    "d8_p1_c1_cv1_cw0.4": ((7.114e-07, 5.905e-06, 1.210e-06), (1.872e-07, 1.554e-06, 3.183e-07)),
    "d64_p16_c31_cv1_cw0": ((6.884e-07, 1.259e-05, 2.248e-06), (1.812e-07, 3.312e-06, 5.916e-07)),
    "d64_p17_c32_cv1_cw1": ((1.175e-04, 9.793e-02, 4.410e-04), (3.093e-05, 2.577e-02, 1.161e-04)),
    "d256_p33_c33_cv0.5_cw0.2_perp": ((3.479e-09, 2.571e-06, 1.447e-08), (9.156e-10, 6.765e-07, 3.807e-09)),
    "d8_p17_c256_cv1_cw0.4": ((1.945e-06, 2.542e-05, 2.302e-06), (5.118e-07, 6.689e-06, 6.057e-07)),
    "d256_p16_c257_cv1_cw0": ((6.176e-05, 5.167e-02, 3.157e-04), (1.625e-05, 1.360e-02, 8.309e-05)),
    "d64_p1_c257_cv1_cw1": ((7.424e-07, 1.498e-05, 1.777e-06), (1.954e-07, 3.942e-06, 4.677e-07)),
    "spiked_d64_p33_c257_t07_cv0.5_cw0.2_perp": ((6.160e-08, 9.774e-05, 2.366e-07), (1.621e-08, 2.572e-05, 6.226e-08)),
    "spiked_d256_p17_c257_t001_cv1_cw0.4": ((3.784e-04, 1.656e+00, 2.152e-03), (9.958e-05, 4.358e-01, 5.663e-04)),
    "spiked_d8_p16_c256_t07_cv1_cw0": ((1.223e-06, 2.040e-05, 1.741e-06), (3.218e-07, 5.369e-06, 4.581e-07)),
    "batch_d64_p17_q257_t07_cv1_cw1": ((5.311e-07, 4.821e-06, 9.795e-07), (1.398e-07, 1.269e-06, 2.578e-07)),
    "batch_d256_p33_q257_t001_cv0.5_cw0.2_perp": ((1.507e-06, 6.414e-02, 1.033e-05), (3.966e-07, 1.688e-02, 2.717e-06)),
    "batch_spiked_d64_p16_q257_t07_cv1_cw0.4": ((2.649e-06, 8.679e-05, 7.904e-06), (6.972e-07, 2.284e-05, 2.080e-06)),
    "d64_p17_c1023_cv1_cw0": ((3.673e-07, 4.403e-06, 6.016e-07), (9.666e-08, 1.159e-06, 1.583e-07)),
    "d256_p16_c1024_cv1_cw1": ((7.581e-08, 8.336e-07, 2.910e-07), (1.995e-08, 2.194e-07, 7.658e-08)),
    "d64_p33_c1025_cv0.5_cw0.2_perp": ((1.742e-08, 2.212e-05, 3.715e-08), (4.585e-09, 5.822e-06, 9.775e-09)),
    "d8_p1_c1025_cv1_cw0.4": ((5.374e-05, 6.588e-02, 2.991e-05), (1.414e-05, 1.734e-02, 7.872e-06)),
    "spiked_d256_p17_c1025_t07_cv1_cw0": ((9.033e-07, 8.298e-05, 5.786e-06), (2.377e-07, 2.184e-05, 1.523e-06)),
    "batch_d256_p33_q1025_t07_cv1_cw1": ((1.133e-07, 6.388e-07, 3.344e-07), (2.982e-08, 1.681e-07, 8.801e-08)),
    "d64_p17_c32_cv1_cw1_hard": ((1.175e-04, 9.793e-02, 4.410e-04), (3.093e-05, 2.577e-02, 1.161e-04)),
    "d256_p16_c257_cv1_cw0_hard": ((6.176e-05, 5.167e-02, 3.157e-04), (1.625e-05, 1.360e-02, 8.309e-05)),
    "spiked_d64_p33_c257_t07_cv0.5_cw0.2_perp_hard": ((6.228e-08, 9.774e-05, 2.362e-07), (1.639e-08, 2.572e-05, 6.217e-08)),
    "batch_d64_p17_q257_t07_cv1_cw1_hard": ((5.534e-07, 4.821e-06, 9.649e-07), (1.456e-07, 1.269e-06, 2.539e-07)),
    "batch_d256_p33_q257_t001_cv0.5_cw0.2_perp_hard": ((1.507e-06, 6.414e-02, 1.033e-05), (3.966e-07, 1.688e-02, 2.717e-06)),
    "batch_spiked_d64_p16_q257_t07_cv1_cw0.4_hard": ((2.706e-06, 8.679e-05, 7.934e-06), (7.122e-07, 2.284e-05, 2.088e-06)),
    "d64_p33_c1025_cv0.5_cw0.2_perp_hard": ((1.688e-08, 2.212e-05, 3.936e-08), (4.443e-09, 5.822e-06, 1.036e-08)),
    "batch_d256_p33_q1025_t07_cv1_cw1_hard": ((1.081e-07, 6.388e-07, 3.319e-07), (2.845e-08, 1.681e-07, 8.733e-08)),
}


if __name__ == "__main__":
    print("BOUNDS = {")
    for c in CASES:
        m = measured_error(c)
        print(f'    "{c.name}": (({", ".join(f"{3.8 * e:.3e}" for e in m)}), ({", ".join(f"{e:.3e}" for e in m)})),')
    print("}")
