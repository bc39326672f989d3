"""Case table, fp64 references and bounds for the backward forms of vidil_gemm (VIDIL_EPI_GRAD_IN / VIDIL_EPI_GRAD_W,
include/vidil_hip.h "Backward forms"; csrc/gemm_grad.hip).  Shared by test_gemm_grad_cases_cpu.py (which proves the
table's preconditions without a GPU) and test_gemm_grad_gpu.py.

A case is (form, M, N, K, lda) in the LIBRARY's terms:
  GRAD_IN: out[M,N] = A[M,K] · W[K,N]      contraction K
  GRAD_W : out[N,K] = A[M,N]^T · W[M,K]    contraction M
"""
import itertools

import numpy as np

GRAD_IN, GRAD_W = 6, 7

# constants of csrc/gemm_grad.hip, restated: the straddle cases below name them
GK = 64               # contraction rows per step
BIG_TILES = 64        # 128 x 128 tiles from which the 128-tile serves
TARGET_BLOCKS = 512
MIN_SPLIT = 128
MAX_SPLIT = 16
INT_RANGE = 7         # exact tier: integer operands in [-7, 7]


def cdiv(a, b):
    return -(-a // b)


def dims(form, M, N, K):
    """(R, C, L): output rows, output columns, contraction length."""
    return (M, N, K) if form == GRAD_IN else (N, K, M)


def plan(form, M, N, K):
    """Literal restatement of the header's formula: (tile, nsplit, split_len)."""
    R, C, L = dims(form, M, N, K)
    bt = 128 if cdiv(R, 128) * cdiv(C, 128) >= 64 else 64
    tiles = cdiv(R, bt) * cdiv(C, bt)
    ns = cdiv(L, 128)
    ns = min(ns, 512 // tiles, 16)
    ns = max(ns, 1)
    ln = 64 * cdiv(cdiv(L, ns), 64)
    return bt, cdiv(L, ln), ln


def ws_bytes(form, M, N, K):
    R, C, _ = dims(form, M, N, K)
    _, ns, _ = plan(form, M, N, K)
    return 4 * ns * R * C if ns > 1 else 0


# ------------------------------------------------------------------------------------------------ exact tier
def _in_cases():
    out = []
    # the issue's grid: every M x N x K, lda > K
    for M, N, K in itertools.product((1, 33, 129), (8, 72, 136, 264), (8, 64, 72, 200)):
        out.append((GRAD_IN, M, N, K, K + 8))
    # 64-tile edges (rows 63 / 64 / 65, columns 56 / 64 / 72), dense A
    for M, N in itertools.product((63, 64, 65), (56, 64, 72)):
        out.append((GRAD_IN, M, N, 72, 0))
    # GK = 64: one step, one step + 8;  MIN_SPLIT = 128: unsplit at 128, two ranges at 136, three at 264
    for K in (56, 64, 72, 128, 136, 264):
        out.append((GRAD_IN, 65, 72, K, K + 16))
    # BIG_TILES = 64: 7 x 8 tiles of 128 (64-tile) against 8 x 8 (128-tile); the 128-tile with a row edge and a split
    out.append((GRAD_IN, 896, 1024, 72, 0))
    out.append((GRAD_IN, 897, 1024, 72, 80))
    out.append((GRAD_IN, 1000, 1024, 136, 0))
    return out


def _w_cases():
    out = []
    lda_of = {1: 8, 2: 8, 33: 40, 130: 136}
    for M, N, K in itertools.product((1, 9, 63, 64, 65, 130), (1, 2, 33, 130), (8, 72, 136)):
        out.append((GRAD_W, M, N, K, lda_of[N]))
    # split lengths (MIN_SPLIT = 128 -> split_len 128 here): one and seven rows past one and two of them, and the last full one
    for M in (127, 128, 129, 135, 256, 257, 263):
        out.append((GRAD_W, M, 33, 72, 40))
    # MAX_SPLIT = 16: sixteen ranges of 128 at 2048, eleven of 192 at 2049
    out.append((GRAD_W, 2048, 2, 8, 8))
    out.append((GRAD_W, 2049, 2, 8, 8))
    # TARGET_BLOCKS = 512: 32 tiles allow 16 ranges (of 128), 36 tiles 14 (of 192 once rounded to the step: 11 ranges)
    out.append((GRAD_W, 2048, 256, 512, 0))
    out.append((GRAD_W, 2048, 256, 520, 0))
    # 64-tile edges in both output axes, dense A
    for N, K in itertools.product((56, 64, 72), (56, 64, 72)):
        out.append((GRAD_W, 65, N, K, 0))
    # BIG_TILES = 64: 7 x 8 tiles of 128 (64-tile, two ranges) against 8 x 8 (128-tile, three ranges)
    out.append((GRAD_W, 300, 896, 1024, 0))
    out.append((GRAD_W, 300, 897, 1024, 904))
    return out


EXACT_CASES = _in_cases() + _w_cases()

# (case, name of the constant, (value on one side, value on the other)) — what the table claims to straddle; the CPU test checks it
STRADDLES = [
    ("tile", (GRAD_IN, 896, 1024, 72, 0), (GRAD_IN, 897, 1024, 72, 80), (64, 128)),
    ("tile", (GRAD_W, 300, 896, 1024, 0), (GRAD_W, 300, 897, 1024, 904), (64, 128)),
    ("nsplit", (GRAD_IN, 65, 72, 128, 144), (GRAD_IN, 65, 72, 136, 152), (1, 2)),
    ("nsplit", (GRAD_W, 128, 33, 72, 40), (GRAD_W, 129, 33, 72, 40), (1, 2)),
    ("nsplit", (GRAD_W, 256, 33, 72, 40), (GRAD_W, 257, 33, 72, 40), (2, 3)),
    ("nsplit", (GRAD_W, 2048, 2, 8, 8), (GRAD_W, 2049, 2, 8, 8), (16, 11)),
    ("nsplit", (GRAD_W, 2048, 256, 512, 0), (GRAD_W, 2048, 256, 520, 0), (16, 11)),
    ("split_len", (GRAD_W, 2048, 2, 8, 8), (GRAD_W, 2049, 2, 8, 8), (128, 192)),
]

# representatives of every kernel path for the confinement / resid / determinism tests: (64 | 128 tile) x (unsplit | split)
PATH_CASES = [
    (GRAD_IN, 33, 72, 72, 80), (GRAD_IN, 65, 72, 264, 280), (GRAD_IN, 897, 1024, 72, 80), (GRAD_IN, 1000, 1024, 136, 0),
    (GRAD_W, 65, 33, 72, 40), (GRAD_W, 263, 33, 72, 40), (GRAD_W, 100, 897, 1024, 904), (GRAD_W, 300, 897, 1024, 904),
]


def case_id(c):
    form, M, N, K, lda = c
    return f"{'in' if form == GRAD_IN else 'w'}-M{M}-N{N}-K{K}-lda{lda}"


def operand_shapes(form, M, N, K, lda):
    """((A rows, A row stride, A valid columns), (W rows, W columns))"""
    if form == GRAD_IN:
        return (M, lda or K, K), (K, N)
    return (M, lda or N, N), (M, K)


def exact_operands(case):
    """Small-integer operands (exact in f16 and bf16): A [rows, valid columns], W [rows, columns] as float64."""
    form, M, N, K, lda = case
    (ar, _, ac), (wr, wc) = operand_shapes(*case)
    rng = np.random.default_rng(abs(hash((form, M, N, K))) % (2 ** 31))
    a = rng.integers(-INT_RANGE, INT_RANGE + 1, size=(ar, ac)).astype(np.float64)
    w = rng.integers(-INT_RANGE, INT_RANGE + 1, size=(wr, wc)).astype(np.float64)
    return a, w


def normal_operands(case, seed=0):
    form, M, N, K, lda = case
    (ar, _, ac), (wr, wc) = operand_shapes(*case)
    rng = np.random.default_rng(1000 + seed + abs(hash((form, M, N, K))) % (2 ** 31))
    return rng.standard_normal((ar, ac)).astype(np.float32), rng.standard_normal((wr, wc)).astype(np.float32)


def reference(form, a, w):
    """fp64 product and the per-element sum of |a||b|."""
    a = np.asarray(a, np.float64)
    w = np.asarray(w, np.float64)
    if form == GRAD_IN:
        return a @ w, np.abs(a) @ np.abs(w)
    return a.T @ w, np.abs(a).T @ np.abs(w)


def rounded_bound(L, sum_abs):
    """Products of two 16-bit numbers are exact in f32, so the error is that of L f32 additions in any order plus the merge
    and the residual add: (L + 8) * 2^-24 * sum |a||b| per element (derived, not measured)."""
    return (L + 8) * 2.0 ** -24 * sum_abs
