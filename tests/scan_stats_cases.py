"""Cases of the paired softmax-statistics form of the scan (`vidil_scan_topk` with `topk == 0`, `kernels.scan_softmax_stats`),
shared by tests/test_scan_stats_cpu.py (inputs, reference and bounds, no GPU) and tests/test_scan_stats_gpu.py.

Per pair p and category c, over the classes j of the category, with v_j = values[p]·keys[j] and w_j = weights[p]·keys[j]:

    out[p, c] = (max v,  sum exp(v - max v),  max w,  sum exp(w - max w),  sum exp(w - max w) * v),   index[p, c] = argmax v.

Inputs are f32; the expected values are the same five numbers in fp64 on those f32 inputs (`reference`).

Bounds (`BOUNDS`): per case and per output, 4 x the error against fp64 of a plain f32 computation of the same quantity written
with torch ops on the CPU (`plain_f32`; maximum over the case's pairs and categories).  The f32 dot products of `plain_f32` run as
one rounded multiply and one rounded add per k, so the measurement does not depend on the host's BLAS; its exp and sum are torch's.
The factor is for the kernel's other order of summation (fma chain, per-lane online softmax, fixed-order merges).  Recorded at
3.8 x the measurement (the practice of attention_f32_cases.py); tests/test_scan_stats_cpu.py recomputes the measurement and asserts 2 x <= bound <= 4 x.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

TILE = 32            # classes per class tile (one MFMA)
CHUNK = 8 * TILE     # classes per workgroup (scan.hip: CT * 32)
OUTPUTS = ("max_v", "sum_exp_v", "max_w", "sum_exp_w", "sum_exp_w_v")


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    P: int
    classes: int            # one category of this many classes; with `batch`, the queue segment behind the batch segment
    temp: float
    spiked: bool = False
    batch: bool = False     # two categories: P batch rows, NaN rows up to the next multiple of 32, then `classes` queue rows


CASES = [
    # one category: the class-tile edge (31 / 32 / 33) and the chunk edge (256 / 257); pairs across the 16 + 16 row tile (16 / 17 / 33)
    Case("d8_p1_c1", 8, 1, 1, 0.07),
    Case("d64_p16_c31", 64, 16, 31, 0.07),
    Case("d64_p17_c32", 64, 17, 32, 0.001),
    Case("d256_p33_c33", 256, 33, 33, 0.07),
    Case("d8_p17_c256", 8, 17, 256, 0.07),
    Case("d256_p16_c257", 256, 16, 257, 0.001),
    Case("d64_p1_c257", 64, 1, 257, 0.07),
    # spiked keys: every lane's second tile, every merged list and every later chunk raises the maximum (alpha != 0, 1)
    Case("spiked_d64_p33_c257_t07", 64, 33, 257, 0.07, spiked=True),
    Case("spiked_d256_p17_c257_t001", 256, 17, 257, 0.001, spiked=True),
    Case("spiked_d8_p16_c256_t07", 8, 16, 256, 0.07, spiked=True),
    # batch segment + NaN padding + queue segment, as the contrastive loss lays its keys out
    Case("batch_d64_p17_q257_t07", 64, 17, 257, 0.07, batch=True),
    Case("batch_d256_p33_q257_t001", 256, 33, 257, 0.001, batch=True),
    Case("batch_spiked_d64_p16_q257_t07", 64, 16, 257, 0.07, spiked=True, batch=True),
]


def _seed(c):
    return [c.D, c.P, c.classes, int(c.temp * 1e4), int(c.spiked), int(c.batch)]


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def spike_gain(i, n):
    """Length of the i-th of n spike keys along the queries' common direction: rises from 0.35 to 0.95."""
    return 0.35 + 0.6 * i / max(1, n - 1)


def layout(c):
    """(seg_start, seg_len, key rows)"""
    if not c.batch:
        return [0], [c.classes], c.classes
    q0 = (c.P + TILE - 1) // TILE * TILE
    return [0, q0], [c.P, c.classes], q0 + c.classes


@lru_cache(maxsize=None)
def inputs(c):
    """values, weights f32 [P,D] (unit rows divided by the temperature), keys f32 [NCpad,D], seg_start, seg_len.  Read-only."""
    rng = np.random.default_rng(_seed(c))
    seg_start, seg_len, rows = layout(c)
    e0 = _unit(rng.standard_normal((1, c.D)))
    val = rng.standard_normal((c.P, c.D))
    wgt = rng.standard_normal((c.P, c.D))
    keys = np.full((rows, c.D), np.nan)
    for s0, n in zip(seg_start, seg_len):
        keys[s0:s0 + n] = _unit(rng.standard_normal((n, c.D)))
    if c.spiked:
        # every query row leans on e0; two keys of every class tile (one in either half of the MFMA's class interleave: offsets
        # 1 and 5) point along e0 with a length that grows from tile to tile, everything else is short
        val, wgt = val + 3.0 * np.sqrt(c.D) * e0, wgt + 3.0 * np.sqrt(c.D) * e0
        s0, n = seg_start[-1], seg_len[-1]
        keys[s0:s0 + n] *= 0.1
        spots = [t + o for t in range(0, n, TILE) for o in (1, 5) if t + o < n]
        for i, j in enumerate(spots):
            keys[s0 + j] = spike_gain(i, len(spots)) * e0 + 0.02 * keys[s0 + j]
    val, wgt = _unit(val) / c.temp, _unit(wgt) / c.temp
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
    return t(val), t(wgt), t(keys), seg_start, seg_len


def five(v, w):
    """The five numbers and the argmax from score matrices v, w [P, n] (any float type)."""
    mv, iv = v.max(1)
    mw = w.max(1).values
    ew = torch.exp(w - mw[:, None])
    return torch.stack([mv, torch.exp(v - mv[:, None]).sum(1), mw, ew.sum(1), (ew * v).sum(1)], 1), iv


@lru_cache(maxsize=None)
def reference(c):
    """fp64 on the f32 inputs: (stats f64 [P,ncat,5], argmax i64 [P,ncat], v f64 per category)."""
    val, wgt, keys, seg_start, seg_len = inputs(c)
    out, idx, vs = [], [], []
    for s0, n in zip(seg_start, seg_len):
        k = keys[s0:s0 + n].double()
        v, w = val.double() @ k.T, wgt.double() @ k.T
        o, i = five(v, w)
        out.append(o); idx.append(i); vs.append(v)
    return torch.stack(out, 1), torch.stack(idx, 1), vs


def _dot32(a, b):
    """a [P,D] · b [n,D]^T in f32, k in order, one rounded multiply and one rounded add per k."""
    s = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32)
    for k in range(a.shape[1]):
        s = s + a[:, k:k + 1] * b[:, k][None, :]
    return s


def plain_f32(c):
    val, wgt, keys, seg_start, seg_len = inputs(c)
    out = []
    for s0, n in zip(seg_start, seg_len):
        out.append(five(_dot32(val, keys[s0:s0 + n]), _dot32(wgt, keys[s0:s0 + n]))[0])
    return torch.stack(out, 1)


def measured_error(c):
    """max |plain f32 - fp64| per output over the case's pairs and categories -> 5 floats."""
    ref = reference(c)[0]
    return [(plain_f32(c).double() - ref)[..., q].abs().max().item() for q in range(5)]


def errors(c, stats):
    """max |stats - fp64| per output for a result f32 [P,ncat,5]."""
    ref = reference(c)[0]
    return [(stats.double().cpu() - ref)[..., q].abs().max().item() for q in range(5)]


def undecided_argmax(c):
    """[P,ncat] bool: the two largest fp64 values of v are closer than f32 arithmetic decides (never the case on these inputs;
    asserted on the CPU, so that the argmax may be compared with fp64's as well as with the top-k form's)."""
    out = []
    for v in reference(c)[2]:
        if v.shape[1] == 1:
            out.append(torch.zeros(v.shape[0], dtype=torch.bool))
            continue
        top = v.topk(2, 1).values
        out.append((top[:, 0] - top[:, 1]) < 1e-4 * top[:, 0].abs().clamp(min=1.0))
    return torch.stack(out, 1)


# name -> ((bound per output), (the CPU measurement it was taken from)); bound = 3.8 x measurement.  Written by `python
# tests/scan_stats_cases.py`, which prints this table from `measured_error`.
BOUNDS = {
    "d8_p1_c1": ((9.744e-07, 0.000e+00, 8.711e-07, 0.000e+00, 9.744e-07),
                (2.564e-07, 0.000e+00, 2.292e-07, 0.000e+00, 2.564e-07)),
    "d64_p16_c31": ((3.443e-06, 5.452e-06, 3.594e-06, 1.094e-05, 1.463e-05),
                   (9.059e-07, 1.435e-06, 9.459e-07, 2.879e-06, 3.850e-06)),
    "d64_p17_c32": ((3.166e-04, 3.685e-06, 1.948e-04, 2.373e-07, 1.642e-04),
                   (8.331e-05, 9.698e-07, 5.125e-05, 6.245e-08, 4.322e-05)),
    "d256_p33_c33": ((3.306e-06, 2.130e-05, 4.609e-06, 3.729e-05, 1.183e-05),
                    (8.701e-07, 5.604e-06, 1.213e-06, 9.813e-06, 3.112e-06)),
    "d8_p17_c256": ((4.146e-06, 1.091e-05, 5.369e-06, 1.095e-05, 3.371e-05),
                   (1.091e-06, 2.870e-06, 1.413e-06, 2.881e-06, 8.871e-06)),
    "d256_p16_c257": ((3.166e-04, 1.226e-05, 3.660e-04, 1.045e-04, 3.435e-03),
                     (8.331e-05, 3.227e-06, 9.632e-05, 2.749e-05, 9.040e-04)),
    "d64_p1_c257": ((4.990e-06, 7.569e-06, 2.836e-06, 1.725e-05, 1.417e-05),
                   (1.313e-06, 1.992e-06, 7.463e-07, 4.539e-06, 3.730e-06)),
    "spiked_d64_p33_c257_t07": ((1.347e-05, 2.391e-05, 9.767e-06, 1.879e-05, 2.334e-04),
                               (3.544e-06, 6.293e-06, 2.570e-06, 4.944e-06, 6.142e-05)),
    "spiked_d256_p17_c257_t001": ((1.841e-03, 0.000e+00, 1.079e-03, 0.000e+00, 1.841e-03),
                                 (4.846e-04, 0.000e+00, 2.841e-04, 0.000e+00, 4.846e-04)),
    "spiked_d8_p16_c256_t07": ((4.130e-06, 6.517e-06, 3.292e-06, 4.752e-06, 6.432e-05),
                              (1.087e-06, 1.715e-06, 8.662e-07, 1.251e-06, 1.693e-05)),
    "batch_d64_p17_q257_t07": ((4.899e-06, 3.280e-05, 3.906e-06, 4.879e-05, 1.545e-05),
                              (1.289e-06, 8.632e-06, 1.028e-06, 1.284e-05, 4.067e-06)),
    "batch_d256_p33_q257_t001": ((3.827e-04, 6.700e-05, 3.721e-04, 3.510e-04, 4.310e-03),
                                (1.007e-04, 1.763e-05, 9.792e-05, 9.237e-05, 1.134e-03)),
    "batch_spiked_d64_p16_q257_t07": ((1.118e-05, 2.338e-05, 1.087e-05, 1.495e-05, 1.654e-04),
                                     (2.942e-06, 6.151e-06, 2.861e-06, 3.933e-06, 4.354e-05)),
}


if __name__ == "__main__":
    print("BOUNDS = {")
    for c in CASES:
        m = measured_error(c)
        print(f'    "{c.name}": (({", ".join(f"{3.8 * e:.3e}" for e in m)}),\n        {" " * len(c.name)}({", ".join(f"{e:.3e}" for e in m)})),')
    print("}")
