"""Cases, inputs and references for the tests of the epilogue FEATURES of `vidil_gemm` that tests/gemm_cases.py has no field for
(tests/test_gemm_stat_forms_gpu.py; this table's own preconditions are asserted without a GPU by
tests/test_gemm_stat_cases_cpu.py):

  fold    the LayerNorm-fold consumer (ln_fold, ln_colsum, ln_stats, ln_eps) on EPI_F16 / EPI_HEADS / EPI_ARENA
  prod    the row-partials producer (EPI_F32 + out16 + ln_stats_out) and the plain out16 copy
  rln     the residual LayerNorm (rln_gamma / rln_beta + ln_stats + ln_stats_out)
  split3  out16_split3 = 1 / 2, with and without `out`, on the 8-wave, the 4-wave and the compensated (split_k) kernel
  fp8     e4m3 operands with per-column w_scale: EPI_F32 / EPI_PATCH / EPI_HEADS in the companion type, EPI_F8

Every case names the kernel bodies it runs on (`SCase.bodies`: gemm256_kernel with VIDIL_GEMM4W=0 and gemm4w_kernel with
VIDIL_GEMM4W=1, or the compensated 128-row form); `expected_kernel` restates the dispatcher for these features.

Two tiers of reference.
EXACT (bit equality).  Operands are small integers, so accumulators are exact.  `ln_stats` is an INPUT — both kernels use the
partials they are handed and never recompute them from A — so the table hands in integer partials whose sums give a dyadic mean
and var + eps = 4^j with eps = 2^-6 at a power-of-two width: rstd = 2^-j, mean * rstd and both fused multiply-adds of the fold
(and of the residual LayerNorm) are then exact in f32 in any order, and the stored value is the ONE rounding of the exact result
to the output type.  Every row has its own (mean, rstd); every part is non-zero and differs from the row's other parts.
BOUND.  Widths whose reciprocal is inexact (192, 320, 576, 768, 832, 960) and the activation cases: float64 from the same f32
inputs, with a bound propagated through the kernel's chain (`stat_chain`, `pre_activation`, `source_values`): sums of the partials in
any order, s * inv_k, ss * inv_k - mean^2 (fused or not), 1 / sqrtf, two fused multiply-adds, the rounding of the output type.

Destinations live in sentinel-filled allocations with guards exactly as in gemm_cases; `expected` returns per destination the
values, the mask of what a correct launch writes and, for the bound tier, the elementwise bound."""
import zlib
from dataclasses import dataclass

import numpy as np
import torch

import gemm_cases as gc
from branch_cases import ulp
from gemm_cases import (ACT_GELU_ERF, ACT_NONE, ACT_QUICK_GELU, C3_128, EPI_ARENA, EPI_F16, EPI_F32, EPI_HEADS, EPI_PATCH, G256, GUARD,
                        NAN_ROWS, SENTINEL16, SENTINEL32, T16, W4, _cdiv)

EPI_F8 = 5                       # include/vidil_hip.h VIDIL_EPI_F8
F8 = torch.float8_e4m3fn
SENTINEL8 = 0x7F                 # S.1111.111: the NaN of e4m3fn
F8_MAX = 448.0
U = 2.0 ** -23                   # charged per f32 operation of the chain: ONE ulp (a faithfully rounded result), twice the unit
#                                  roundoff of a correctly rounded one — so the round-to-nearest emulation of the same chain on
#                                  the CPU has to stay within HALF of every bound below (tests/test_gemm_stat_cases_cpu.py)
EXACT_EPS = 2.0 ** -6
BOUND_EPS = float(np.float32(1e-5))
M_SET = (1, 31, 33, 127, 129, 255, 257, 300)        # the 32-row tile, the 128-row group, the 256-row tile; M - 1 clamping at one row
FOLD_K = (128, 192, 256, 320, 576, 768, 832, 1024)  # nparts 2, 3, 4, 5, 9, 12, 13, 16: every on / off pattern of the part guards
EXACT_WIDTHS = (64, 128, 256, 512, 1024)
RLN_BOUND_N = (192, 320, 768, 960)
FEATURES = ("fold", "prod", "rln", "split3", "fp8")
ENV = {G256: {"VIDIL_GEMM4W": "0"}, W4: {"VIDIL_GEMM4W": "1"}, C3_128: {}}
GELU_LIPSCHITZ = 1.13            # max |d/dx| of erf-GELU (1.129) and of quick-GELU (1.100)


@dataclass(frozen=True)
class SCase(gc.Case):
    feature: str = "fold"
    tier: str = "exact"         # exact | bound (the statistics; an activation makes a case inexact whatever the tier)
    bodies: tuple = (G256, W4)
    out16: bool = False
    stats: bool = False         # ln_stats_out
    rln: bool = False
    ldo16_pad: int = 0          # ldo16 = N + pad (split3: three planes of N + pad columns)
    split3: int = 0             # out16_split3
    fp8: bool = False

    @property
    def exact(self):
        return self.tier == "exact" and self.act == ACT_NONE

    @property
    def fold(self):
        return self.feature == "fold"

    @property
    def plane(self):
        return self.N + self.ldo16_pad

    @property
    def ldo16(self):
        return 3 * self.plane if self.split3 else self.plane

    @property
    def width(self):            # the normalised row: A's for the fold, the residual's for the residual LayerNorm
        return self.K if self.fold else self.N

    @property
    def nstat(self):
        return self.width // 64

    @property
    def eps(self):
        return EXACT_EPS if self.tier == "exact" else BOUND_EPS


# ================================================================================================================ the dispatcher
def c3_serves(c, cus=256):
    """vidil_gemm_c3_serves (gemm.hip): the K-loop compensated form takes split_k launches with the f32 / patch / per-head
    (T >= 8) epilogue — out16_split3 included, but no fp8, ln_fold, ln_stats_out or rln."""
    if not c.split_k or c.fp8 or c.fold or c.stats or c.rln or c.K % 96:
        return False
    return c.epi in (EPI_F32, EPI_PATCH) or (c.epi == EPI_HEADS and c.T >= 8)


def prefer_4w(c, cus=256):
    """prefer_4w (gemm256.hip) for the features of this table."""
    if c.epi == EPI_HEADS and c.T < 8:
        return False
    sw = c.env.get("VIDIL_GEMM4W")
    if sw is not None:
        return int(sw) != 0
    tiles = _cdiv(c.M, 256) * _cdiv(c.N, 256)
    if tiles < 3 * cus // 2:
        return False
    if c.fp8:
        return c.epi in (EPI_F8, EPI_HEADS) or (c.epi == EPI_F32 and c.act == ACT_NONE)
    if c.fold or c.epi in (EPI_F16, EPI_HEADS, EPI_ARENA):
        return True
    return c.epi == EPI_F32 and (c.stats or c.K >= 1536)


def not_built_4w(c):
    """The -1000 answers of launch4w_fp8 (gemm4w.hip): fp8 operands with an activation on f32 rows, or with the patch epilogue,
    run on gemm256_kernel whatever the switch says (built_4w in gemm256.hip; vidil_gemm_kernel_name says so too)."""
    return c.fp8 and ((c.epi == EPI_F32 and c.act != ACT_NONE) or c.epi == EPI_PATCH)


def expected_kernel(c, cus=256):
    """The kernel vidil_gemm LAUNCHES for a case under c.env, as vidil_gemm_kernel_name spells it: forced_big of choose_tile
    (ln_fold, out16, ln_stats_out and fp8 operands run a 256 x 256 kernel whatever M is), prefer_4w, and the -1000 fall-backs."""
    t16 = gc.CNAME[c.dtype]
    act = c.act if c.epi in (EPI_F16, EPI_F32, EPI_F8) else 0
    if c3_serves(c, cus):
        tm = 4 if (_cdiv(c.M, 256) * _cdiv(c.N, 256) >= 5 * cus // 8 or c.epi == EPI_PATCH) else 2
        return f"gemm4w_kernel<{t16}, {t16}, {c.epi}, {act if c.epi == EPI_F32 else 0}, false, false, false, {tm}, true>"
    assert c.fold or c.out16 or c.stats or c.fp8, c.name         # forced_big
    t = "fp8" if c.fp8 else t16
    flags = ", ".join("true" if f else "false" for f in (c.fold, c.stats and c.epi == EPI_F32, c.rln))
    if prefer_4w(c, cus) and not not_built_4w(c):
        return f"gemm4w_kernel<{t}, {t16}, {c.epi}, {act}, {flags}, 4, false>"
    return f"gemm256_kernel<{t}, {t16}, {c.epi}, {act}, {flags}>"


def with_body(c, body):
    """The case with the developer switches of one of its bodies."""
    assert body in c.bodies
    return SCase(**{**{f: getattr(c, f) for f in c.__dataclass_fields__}, "kernel": body, "env": dict(ENV[body])})


def instantiation(c, body):
    """(feature flags, epilogue, activation, body, 16-bit type, fp8): one template instantiation of the launchers."""
    return (c.fold, c.stats, c.rln, c.epi, c.act if c.epi in (EPI_F16, EPI_F32, EPI_F8) else 0, body, c.dtype, c.fp8)


# what the launchers build and no case can reach, with what excludes it (tests/test_gemm_stat_cases_cpu.py checks the names)
UNREACHABLE = {
    "fold x EPI_F32 / EPI_PATCH": "VIDIL_REQUIRE gemm/ln_fold: only EPI_F16 / EPI_HEADS / EPI_ARENA consume a folded LayerNorm",
    "stats x activation": "VIDIL_REQUIRE gemm/ln_stats_out: ... f32 residual epilogue without activation",
    "rln without stats": "VIDIL_REQUIRE gemm/rln: the residual LayerNorm needs ... ln_stats_out",
    "fp8 x fold / out16 / stats / rln": "VIDIL_REQUIRE gemm/fp8: the LayerNorm fold is a 16-bit feature",
    "fp8 x EPI_F16 / EPI_ARENA": "VIDIL_REQUIRE gemm/fp8: epilogue %d is not built for fp8 operands",
    "gemm4w x fp8 x EPI_F32 + activation": "-1000 in launch4w_fp8",
    "gemm4w x fp8 x EPI_PATCH": "-1000 in launch4w_fp8",
    "gemm4w x EPI_HEADS with T < 8": "prefer_4w returns false: the 4-wave scatter steps (image, token) by 8 rows",
    "gemm4w/128 x any feature": "-1000 in launch4w128_dispatch; vidil_gemm4w128_wanted refuses ln_fold / ln_stats_out / rln / out16 / fp8",
    "C3 x fold / stats / rln / fp8": "vidil_gemm_c3_serves returns false (VIDIL_REQUIRE gemm/split_k: no ln_fold, 16-bit operands)",
    "C3/256 x out16_split3": "vidil_gemm4w_c3_launch takes 256-row tiles from 5/8 of the CUs in tiles on: M above this table's 600 rows",
}


# ================================================================================================================ the table
def _heads_kw(T, H, part0, parts, layout, t_off):
    span = t_off + T
    kw = dict(T=T, H=H, part0=part0, t_off=t_off if part0 + parts > 1 else 0, Tq_cap=T + T // 8 + 2, N=parts * H * 64,
              q_scale=0.5 if T % 2 else 0.25)
    if layout == "tiled":
        kw.update(tiled=True, Tk_cap=_cdiv(span + span // 8 + 1, 32) * 32)
    elif layout == "vt":
        kw.update(Tk_cap=span + span // 8 + 2, NP=_cdiv(span + span // 8 + 1, 16) * 16)
    else:
        kw.update(Tk_cap=span + span // 8 + 2)
    return kw


def _cases():
    cs = []

    def add(name, feature, **kw):
        for dt in ("f16", "bf16"):
            cs.append(SCase(name=f"{feature}_{name}_{dt}", kernel="", dtype=dt, feature=feature, **kw))

    tier_of = lambda w: "exact" if w in EXACT_WIDTHS else "bound"
    acts = ((ACT_NONE, "none"), (ACT_GELU_ERF, "gelu"), (ACT_QUICK_GELU, "quick"))
    # ---- 1. the consumer.  EPI_F16: every width x every activation, M / N / ldo / bias rotating; every M at 13 parts and at 2
    for i, K in enumerate(FOLD_K):
        for a, (act, an) in enumerate(acts):
            j = i * 3 + a
            N = (8, 72, 264, 520)[(i + a) % 4]
            add(f"f16_K{K}_{an}_M{M_SET[j % 8]}_N{N}", "fold", tier=tier_of(K), epi=EPI_F16, act=act, K=K, M=M_SET[j % 8], N=N,
                ldo_pad=8 * (j % 2), bias=j % 3 != 0)
    for i, M in enumerate(M_SET):
        K = (832, 128)[i % 2]
        add(f"f16_K{K}_sweep_M{M}", "fold", tier=tier_of(K), epi=EPI_F16, K=K, M=M, N=(264, 8, 520, 72)[i % 4], ldo_pad=8 * ((i + 1) % 2),
            bias=i % 2 == 0)
        add(f"f16_K{(1024, 576)[i % 2]}_sweep_M{M}", "fold", tier=tier_of((1024, 576)[i % 2]), epi=EPI_F16, K=(1024, 576)[i % 2], M=M,
            N=(72, 520, 8, 264)[i % 4], ldo_pad=8 * (i % 2), bias=i % 4 != 1)
    # EPI_HEADS: T x V layout, t_off > 0 and capacity rows; T < 8 runs on the 8-wave kernel only
    heads = ((1, 3, 0, 3, "vt", 5, 129), (7, 1, 0, 3, "row", 2, 133), (8, 3, 1, 2, "tiled", 3, 256), (9, 1, 0, 3, "vt", 6, 261),
             (33, 3, 0, 3, "tiled", 7, 297), (9, 3, 0, 1, "row", 0, 36), (33, 1, 1, 2, "row", 4, 132), (8, 1, 0, 3, "vt", 13, 40),
             (9, 1, 0, 3, "tiled", 1, 126), (33, 1, 0, 3, "row", 2, 33), (1, 1, 1, 2, "tiled", 9, 31))
    for i, (T, H, part0, parts, layout, t_off, M) in enumerate(heads):
        K = FOLD_K[i % 8]
        add(f"heads_K{K}_T{T}_H{H}_p{part0}x{parts}_{layout}_M{M}", "fold", tier=tier_of(K), epi=EPI_HEADS, K=K, M=M, bias=i % 3 != 1,
            bodies=(G256,) if T < 8 else (G256, W4), **_heads_kw(T, H, part0, parts, layout, t_off))
    # EPI_ARENA: the decode step (T = 1, slot stride 1) and the shared prompt pass (T = P, slot stride nb)
    for i, (T, stride, part0, parts, M) in enumerate(((1, 1, 0, 3, 129), (5, 3, 0, 3, 255), (1, 1, 1, 2, 33), (5, 3, 1, 2, 300), (1, 1, 0, 3, 1))):
        K = FOLD_K[(3 * i + 2) % 8]
        B = M // T
        add(f"arena_K{K}_T{T}_s{stride}_p{part0}_M{M}", "fold", tier=tier_of(K), epi=EPI_ARENA, K=K, M=M, N=parts * 64, T=T, H=1,
            part0=part0, t_off=2, Tk_cap=2 + T + 2, arena_rows=(B - 1) * stride + 1 + 2, slot_stride=stride, bias=i % 2 == 0)
    # ---- 2. the producer: out16 + ln_stats_out, and out16 alone (has16 && !STATS)
    j = 0
    for N in (64, 192, 320, 1088):
        for K in (128, 192, 1024):
            add(f"N{N}_K{K}_M{M_SET[j % 8]}", "prod", epi=EPI_F32, N=N, K=K, M=M_SET[j % 8], out16=True, stats=True, ldo_pad=4 * (j % 2),
                ldo16_pad=4 * ((j // 2) % 2), resid=("none", "alias", "own")[j % 3], bias=j % 4 != 3)
            j += 1
    for i, M in enumerate(M_SET):
        add(f"sweep_M{M}", "prod", epi=EPI_F32, N=192, K=128, M=M, out16=True, stats=True, ldo_pad=4 * ((i + 1) % 2), ldo16_pad=4 * (i % 2),
            resid=("own", "none", "alias")[i % 3])
    for i, (N, M) in enumerate(((64, 33), (260, 257), (320, 1), (1088, 129), (68, 300))):
        add(f"copy_N{N}_M{M}", "prod", epi=EPI_F32, N=N, K=(128, 192, 1024)[i % 3], M=M, out16=True, ldo_pad=4 * (i % 2),
            ldo16_pad=4 * ((i + 1) % 2), resid=("alias", "own", "none")[i % 3], bias=i != 2)
    # ---- 3. the residual LayerNorm: in place and with its own resid (ldo = N: check_args)
    j = 0
    for N in EXACT_WIDTHS + RLN_BOUND_N:
        for resid in ("alias", "own"):
            add(f"N{N}_{resid}_M{M_SET[j % 8]}", "rln", tier=tier_of(N), epi=EPI_F32, N=N, K=(128, 192)[j % 2], M=M_SET[j % 8], out16=True,
                stats=True, rln=True, resid=resid, ldo16_pad=4 * (j % 2), bias=j % 3 != 2)
            j += 1
    # ---- 4. out16_split3: 8-wave, 4-wave and compensated producer; `out` given and NULL are two launches of one case
    j = 0
    for s3 in (1, 2):
        for act, an in acts:
            for pad in (0, 4):
                N, M = (12, 72, 260, 520)[j % 4], M_SET[(j * 3 + 1) % 8]
                add(f"v{s3}_{an}_ldo16+{3 * pad}_M{M}_N{N}", "split3", epi=EPI_F32, act=act, N=N, K=128, M=M, out16=True, split3=s3,
                    ldo16_pad=pad, ldo_pad=4 * ((j + 1) % 2))
                add(f"c3_v{s3}_{an}_ldo16+{3 * pad}_M{M}_N{N}", "split3", epi=EPI_F32, act=act, N=N, K=(192, 384)[j % 2], M=M, out16=True,
                    split3=s3, ldo16_pad=pad, ldo_pad=4 * (j % 2), split_k=1, bodies=(C3_128,))
                j += 1
    add("v2_none_M600_N1088", "split3", epi=EPI_F32, N=1088, K=128, M=600, out16=True, split3=2, ldo16_pad=4)
    # ---- 5. fp8 operands
    j = 0
    for K in (128, 384, 1024):
        for pad in (0, 16):
            add(f"f32_K{K}_lda+{pad}_M{M_SET[j % 8]}", "fp8", fp8=True, epi=EPI_F32, K=K, lda_pad=pad, M=M_SET[j % 8], N=(68, 264, 520)[j % 3],
                ldo_pad=4 * (j % 2), resid=("own", "alias", "none")[j % 3], bias=j % 4 != 1)
            j += 1
    for act, an in acts[1:]:
        add(f"f32_{an}_M129", "fp8", fp8=True, epi=EPI_F32, act=act, K=128, M=129, N=72, ldo_pad=4, bodies=(G256,))
    for tpi, K, pad in ((4, 128, 16), (49, 384, 0)):
        add(f"patch_tpi{tpi}_K{K}", "fp8", fp8=True, epi=EPI_PATCH, K=K, lda_pad=pad, M=3 * tpi * (8 if tpi == 4 else 1), N=264, tpi=tpi, ldo_pad=8,
            bodies=(G256,))
    for i, (T, H, part0, parts, layout, t_off, M) in enumerate(((9, 1, 0, 3, "vt", 5, 261), (33, 3, 0, 3, "tiled", 7, 132), (8, 1, 0, 3, "row", 2, 256),
                                                                 (7, 1, 0, 3, "vt", 3, 35), (33, 1, 1, 2, "tiled", 3, 33))):
        add(f"heads_T{T}_H{H}_p{part0}x{parts}_{layout}_M{M}", "fp8", fp8=True, epi=EPI_HEADS, K=(128, 384, 1024)[i % 3], lda_pad=16 * (i % 2), M=M,
            bodies=(G256,) if T < 8 else (G256, W4), **_heads_kw(T, H, part0, parts, layout, t_off))
    j = 0
    for N in (16, 80, 272):
        for pad in (0, 16):
            for act, an in acts:
                add(f"f8_N{N}_ldo+{pad}_{an}_M{M_SET[j % 8]}", "fp8", fp8=True, epi=EPI_F8, act=act, K=(128, 384, 1024)[j % 3], lda_pad=16 * ((j // 3) % 2),
                    M=M_SET[j % 8], N=N, ldo_pad=pad, bias=j % 5 != 4)
                j += 1
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ================================================================================================================ inputs
def _rng(c, stream):
    return np.random.default_rng([zlib.crc32(c.name.encode()), stream])


_ints = gc._ints


def _pairs(c, M, means, js):
    """(mean [M], j [M]) with var + eps = 4^j: the (mean, j) combinations in a shuffled order, row m taking combination m (modulo
    their number when there are fewer than rows: rows 1, 32, 128 and 256 apart still differ)."""
    combos = [(a, j) for a in means for j in js]
    n = len(combos)
    assert n >= M or all(d % n for d in (1, 32, 128, 256)), (c.name, n)
    order = _rng(c, 20).permutation(n)
    pick = [combos[order[m % n]] for m in range(M)]
    return np.array([p[0] for p in pick], dtype=np.float64), np.array([p[1] for p in pick], dtype=np.int64)


def _distinct_parts(g, total, n):
    """n distinct non-zero integers that sum to `total`."""
    if n == 1:
        assert total != 0
        return np.array([total], dtype=np.float64)
    span = 8 * n + 50
    pool = np.concatenate([np.arange(-span, 0), np.arange(1, span + 1)])
    while True:
        head = g.choice(pool, size=n - 1, replace=False)
        last = total - head.sum()
        if last != 0 and last not in head:
            return np.append(head, last).astype(np.float64)


def exact_stats(c, M, width, means, js):
    """f32-exact partials [M, width / 64, 2] and the (mean, rstd) they mean, all float64."""
    mean, j = _pairs(c, M, means, js)
    s_tot = width * mean
    ss_tot = width * (4.0 ** j - EXACT_EPS + mean * mean)
    assert np.array_equal(s_tot, np.round(s_tot)) and np.array_equal(ss_tot, np.round(ss_tot)) and (ss_tot > 0).all()
    g = _rng(c, 21)
    st = np.zeros((M, width // 64, 2))
    for m in range(M):
        st[m, :, 0] = _distinct_parts(g, int(s_tot[m]), width // 64)
        st[m, :, 1] = _distinct_parts(g, int(ss_tot[m]), width // 64)
    return st, mean, 2.0 ** -j.astype(np.float64)


def natural_stats(c, M, width, lg=(-2, 2), mu_max=1.5):
    """The f32 partials of rows x = mu + sigma * randn with |mu| <= 1.5 sigma (mean^2 <= 4 var: the cancellation in ss / k -
    mean^2 stays bounded; heavy-mean rows are the job of test_ln_fold_robustness_gpu.py), sigma log-uniform in [1/4, 4]
    (activation cases: sigma in [0.57, 1], |mu| <= 0.75 sigma, which keeps the pre-activation within [-6, 6])."""
    g = _rng(c, 22)
    sigma = 2.0 ** g.uniform(lg[0], lg[1], size=M)
    mu = sigma * g.uniform(-mu_max, mu_max, size=M)
    x = (mu[:, None] + sigma[:, None] * g.standard_normal((M, width))).astype(np.float32).astype(np.float64)
    p = x.reshape(M, width // 64, 64)
    return np.stack([p.sum(2), (p * p).sum(2)], axis=2).astype(np.float32).astype(np.float64)


def inputs(c):
    """float64 arrays (values exact in the types they are launched in): A [M, K], W [N, K], bias, resid, pos as in gemm_cases, and
    colsum [N] / stats_in [M, width / 64, 2] / gamma, beta [N] / w_scale [N] where the feature has them."""
    M, N, K = c.M, c.N, c.K
    d = dict(bias=None, resid=None, pos=None, colsum=None, stats_in=None, gamma=None, beta=None, w_scale=None)
    act = c.act != ACT_NONE
    bf = c.dtype == "bf16" and not c.fp8
    if act:
        # one 1 per A row: the pre-activation is a single product (plus the epilogue's vectors), a multiple of 1/8 within [-6, 6]
        Kl = K // 3 if c.split_k else K
        A = np.zeros((M, K))
        A[np.arange(M), _rng(c, 1).integers(0, Kl, size=M)] = 1.0
        if c.fp8:
            W = _ints(c, 2, (N, Kl), -4, 4)                                 # x w_scale in {1/8 .. 1}: eighths within [-4, 4]
        elif c.fold:
            W = _ints(c, 2, (N, Kl), -16, 16) / 8.0                         # x rstd in {1, 2}: within [-4, 4]
        else:
            W = _ints(c, 2, (N, Kl), -40, 40) / 8.0
        if c.split_k:
            A[:, 2 * Kl:] = A[:, :Kl]
            W = np.concatenate([W, W, np.zeros_like(W)], axis=1)
        d["bias"] = _ints(c, 5, (N,), -1, 1) if c.bias else None
    elif c.split_k:
        Kl = K // 3
        xh, xl = _ints(c, 1, (M, Kl), -1, 1, 0.25 if bf else 1.0), _ints(c, 3, (M, Kl), -1, 1, 0.25)
        wh, wl = _ints(c, 2, (N, Kl), -2, 2), _ints(c, 4, (N, Kl), -1, 1)
        A, W = np.concatenate([xh, xl, xh], axis=1), np.concatenate([wh, wh, wl], axis=1)
    else:
        dense = K <= 256 and not bf and not c.rln     # (rln: |v| < 128 in quarters, so that 64 squares sum exactly)
        A = _ints(c, 1, (M, K), -2, 2) if dense else _ints(c, 1, (M, K), -1, 1, 0.25)
        W = _ints(c, 2, (N, K), -2, 2)
    d["A"], d["W"] = A, W
    if not act and c.bias:
        # split3: integers up to 6 x 10^4 so that the low plane is not zero (f16: ulp 32 there; bf16: ulp 256)
        d["bias"] = _ints(c, 5, (N,), -60000, 60000) if c.split3 else _ints(c, 5, (N,), -4, 4)
    if c.resid != "none":
        d["resid"] = _ints(c, 6, (M, N), -4, 4) * 2.0 if c.rln else _ints(c, 6, (M, N), -8, 8)
    if c.epi == EPI_PATCH:
        d["pos"] = _ints(c, 7, (c.tpi + 1, N), -8, 8)
    if c.fp8:
        e = _rng(c, 8).integers(-3, 1 if act else 4, size=N)       # 2^-3 .. 2^3 per column (with an activation: up to 2^0)
        if not act:
            e[:7] = (-3, 3, -2, 2, -1, 1, 0)                         # (N >= 16: every scale occurs, neighbours differ)
        d["w_scale"] = 2.0 ** e.astype(np.float64)
    if c.fold:
        d["colsum"] = _ints(c, 9, (N,), -1, 1) if act else _ints(c, 9, (N,), -8, 8)
        if c.tier == "bound":
            d["stats_in"] = natural_stats(c, M, K, (-0.8, 0), 0.75) if act else natural_stats(c, M, K)
        elif act:                    # mean in eighths up to 1/2, rstd 1 or 2: mean * rstd * colsum within [-1, 1]
            d["stats_in"], _, _ = exact_stats(c, M, K, [a / 8.0 for a in range(-4, 5)], (-1, 0))
        else:                        # mean in eighths up to 4, rstd 4 .. 1/8
            d["stats_in"], _, _ = exact_stats(c, M, K, [a / 8.0 for a in range(-32, 33) if a], (-2, -1, 0, 1, 2, 3))
    if c.rln:
        d["gamma"] = _rng(c, 10).choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=N)
        d["beta"] = _ints(c, 11, (N,), -8, 8) / 4.0
        if c.tier == "bound":
            d["stats_in"] = natural_stats(c, M, N)
        else:                        # integer mean, rstd in {2, 1, 1/2}: the values written are quarters below 128, whose 64-column
            d["stats_in"], _, _ = exact_stats(c, M, N, [a for a in range(-8, 9) if a], (-1, 0, 1))     # sums of squares are exact
    return d


def operand_tensors(c, d):
    """(A [M + NAN_ROWS, lda], W [N + NAN_ROWS, K]) in the operand type, NaN in A's padding columns and in the rows behind both."""
    dt = F8 if c.fp8 else T16[c.dtype]
    A = torch.full((c.M + NAN_ROWS, c.lda), float("nan")).to(dt)
    A[:c.M, :c.K] = torch.from_numpy(d["A"]).float().to(dt)
    W = torch.full((c.N + NAN_ROWS, c.K), float("nan")).to(dt)
    W[:c.N] = torch.from_numpy(d["W"]).float().to(dt)
    return A, W


# ================================================================================================================ the statistics chain
def stat_chain(stats, width, eps):
    """From partials [M, n, 2] (float64 holding f32 values): float64 mean, rstd, mean * rstd [M] and first-order-plus bounds on what
    the kernels' f32 chain makes of them.  The chain (gemm256.hip / gemm4w.hip, ROWSTAT): the n <= 16 parts are added in a fixed
    tree (half-wave pairs, the two half-waves, four waves) — bounded here for ANY order by (n - 1) u sum |part|; inv_k = 1 / width
    rounded; mean = s * inv_k; var = ss * inv_k - mean * mean, contracted to a fused multiply-add or not (both are covered: every
    product and the difference are charged one rounding); t = var + eps; rstd = 1 / sqrtf(t), charged 1 ulp for the square root and
    2.5 ulp for the division — HIP's documented worst case, the correctly rounded forms are inside it; mrs = mean * rstd rounded.
    Every other operation is charged U = one ulp."""
    n = stats.shape[1]
    g = (n - 1) * U / (1 - (n - 1) * U)
    s, ss = stats[..., 0].sum(1), stats[..., 1].sum(1)
    ds, dss = g * np.abs(stats[..., 0]).sum(1), g * np.abs(stats[..., 1]).sum(1)
    mean, E = s / width, ss / width
    dmean = ds / width + 2 * U * (np.abs(mean) + ds / width)
    dE = dss / width + 2 * U * (np.abs(E) + dss / width)
    var = np.maximum(E - mean * mean, 0.0)       # (the kernels clamp; no case of the table needs it — only the wrong variants of the CPU test)
    dvar = dE + (2 * np.abs(mean) + dmean) * dmean + U * (mean * mean + dmean) + U * (np.abs(var) + dE)
    t = var + eps
    dt = dvar + U * (t + dvar)
    rstd = 1.0 / np.sqrt(t)
    drstd = rstd * (0.5 * dt / np.maximum(t - dt, 0.5 * t) + 3.5 * U) * (1 + 8 * U)      # (dt < t / 2 is asserted per case on the CPU)
    mrs = mean * rstd
    dmrs = np.abs(mean) * drstd + (rstd + drstd) * dmean
    dmrs = dmrs + U * (np.abs(mrs) + dmrs)
    return dict(mean=mean, rstd=rstd, mrs=mrs, dmean=dmean, drstd=drstd, dmrs=dmrs, var=var, t=t, dt=dt)


def acc64(c, d):
    """A . W^T in float64: exact."""
    return d["A"] @ d["W"].T


def pre_activation(c, d, st=None):
    """float64 [M, N] in front of the activation, and its bound [M, N] (zeros where the chain is exact)."""
    acc = acc64(c, d)
    b = d["bias"] if d["bias"] is not None else np.zeros(c.N)
    if c.fold:
        st = st or stat_chain(d["stats_in"], c.K, c.eps)
        inner = b[None, :] - st["mrs"][:, None] * d["colsum"][None, :]
        y = acc * st["rstd"][:, None] + inner
        dinner = np.abs(d["colsum"])[None, :] * st["dmrs"][:, None]
        dinner = dinner + U * (np.abs(inner) + dinner)
        dy = np.abs(acc) * st["drstd"][:, None] + dinner
        dy = dy + U * (np.abs(y) + dy)
        return y, (dy if c.tier == "bound" else np.zeros_like(y))
    if c.fp8:
        return acc * d["w_scale"][None, :] + b[None, :], np.zeros_like(acc)
    return acc + b[None, :], np.zeros_like(acc)


def source_values(c, d):
    """(V, dV) float64 [M, N]: what the epilogue hands to the store for source element (m, n) before the rounding to the output
    type, and the bound on the f32 chain's deviation from it (without the activation's own error and the output rounding)."""
    P, dP = pre_activation(c, d)
    V = gc.activation64(c.act, P)
    dV = dP * (GELU_LIPSCHITZ if c.act != ACT_NONE else 1.0)
    if c.epi == EPI_F32 and d["resid"] is not None:
        u = d["resid"]
        if c.rln:
            st = stat_chain(d["stats_in"], c.N, c.eps)
            inner = u * st["rstd"][:, None] - st["mrs"][:, None]
            ad = inner * d["gamma"][None, :] + d["beta"][None, :]
            if c.tier == "bound":
                dinner = np.abs(u) * st["drstd"][:, None] + st["dmrs"][:, None]
                dinner = dinner + U * (np.abs(inner) + dinner)
                dad = np.abs(d["gamma"])[None, :] * dinner
                dad = dad + U * (np.abs(ad) + dad)
                dV = dV + dad
                dV = dV + U * (np.abs(V + ad) + dV)
            V = V + ad
        else:
            V = V + u
    if c.epi == EPI_PATCH:
        V = V + d["pos"][np.arange(c.M) % c.tpi + 1, :]
    if c.epi in (EPI_HEADS, EPI_ARENA) and c.part0 == 0:
        V, dV = V.copy(), dV.copy()
        V[:, :c.HD] *= c.q_scale
        dV[:, :c.HD] *= c.q_scale
    return V, dV


def emulate_f32(c, d, order=0):
    """The statistics chain and the fused multiply-adds in numpy f32, the way the kernels run them (order: 0 = the parts added
    front to back, 1 = back to front): [M, N] f32 in front of the activation / output rounding.  Fold and rln cases."""
    f = np.float32
    st = d["stats_in"].astype(f)
    idx = range(st.shape[1]) if order == 0 else range(st.shape[1] - 1, -1, -1)
    s, ss = np.zeros(c.M, f), np.zeros(c.M, f)
    for p in idx:
        s, ss = s + st[:, p, 0], ss + st[:, p, 1]
    inv_k = f(1.0) / f(c.width)
    mean = s * inv_k
    var = np.maximum(ss * inv_k - mean * mean, f(0))
    rstd = f(1.0) / np.sqrt(var + f(c.eps))
    mrs = mean * rstd
    acc = acc64(c, d).astype(f)
    b = (d["bias"] if d["bias"] is not None else np.zeros(c.N)).astype(f)
    fma = lambda x, y, z: (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f)   # one rounding (the product is exact in f64)
    if c.fold:
        inner = fma(-mrs[:, None], d["colsum"].astype(f)[None, :], b[None, :])
        return fma(acc, rstd[:, None] + 0 * acc, inner)
    u = d["resid"].astype(f)
    ad = fma(fma(u, rstd[:, None] + 0 * u, -mrs[:, None] + 0 * u), d["gamma"].astype(f)[None, :] + 0 * u, d["beta"].astype(f)[None, :] + 0 * u)
    return (acc + b[None, :]) + ad


# ================================================================================================================ destinations
def dest_shapes(c):
    """name -> (shape, "t16" | "f32" | "f8") of every destination view of a case; `out` is allocated (and must stay untouched)
    when a split3 launch is made without it."""
    s = {"out": ((c.cap_rows, c.ldo), "f8")} if c.epi == EPI_F8 else dict(gc.dest_shapes(c))
    if c.out16:
        s["out16"] = ((c.cap_rows, c.ldo16), "t16")
    if c.stats:
        s["stats"] = ((c.cap_rows, c.N // 64, 2), "f32")
    return s


def int_type(kind):
    return {"f32": (np.int32, SENTINEL32), "t16": (np.int16, SENTINEL16), "f8": (np.int8, SENTINEL8)}[kind]


def float_type(c, kind):
    return {"f32": torch.float32, "t16": T16[c.dtype], "f8": F8}[kind]


def to_type(c, kind, vals):
    """float64 values rounded ONCE to a destination's type (e4m3: saturating at +-448 first, as pack4_fp8 does), as a torch tensor."""
    x = torch.from_numpy(np.ascontiguousarray(vals))
    if kind == "f8":
        x = x.clamp(-F8_MAX, F8_MAX)
    return x.float().to(float_type(c, kind))        # (through f32: every value here is exact in f32, or compared within a bound)


def bits_of(c, kind, vals):
    it = {"f32": torch.int32, "t16": torch.int16, "f8": torch.int8}[kind]
    return to_type(c, kind, vals).view(it).numpy()


def values_of(c, kind, bits):
    it = {"f32": torch.int32, "t16": torch.int16, "f8": torch.int8}[kind]
    return torch.from_numpy(np.ascontiguousarray(bits)).view(float_type(c, kind)).double().numpy()


def out_bound(c, kind, ref, dV):
    """Elementwise bound on |stored - float64| for an inexact case: the chain's bound, the activation's (gemm_cases.act_bound: its
    f32 bound, or the polynomial's for 16-bit and narrower rows) and half an ulp of the output type at the largest magnitude the
    value can have."""
    a = np.zeros_like(ref)
    if c.act != ACT_NONE:
        f32 = gc.BOUNDS["gelu_erf_f32" if c.act == ACT_GELU_ERF else "quick_gelu_f32"][0]
        a += f32 if (kind == "f32" or c.act == ACT_QUICK_GELU) else gc.GELU16_ABS[c.dtype]
    slack = dV + a
    if kind == "f32":
        return slack
    mag = np.abs(ref) + slack
    if kind == "f8":
        return slack + 0.5 * ulp(np.minimum(mag, F8_MAX), F8) + np.maximum(np.abs(ref) - F8_MAX, 0.0)
    if c.act != ACT_NONE:
        return dV + gc.act_bound(c, mag)
    return slack + 0.5 * ulp(mag, T16[c.dtype])


def stats_bound(vals64):
    """Bound on a (sum, sum of squares) pair of 64 f32 values summed in f32 in any order, squares rounded or fused: 64 u (1 + 64 u)
    times the sum of magnitudes."""
    return 64 * U * (1 + 64 * U) * vals64


def expected(c, d=None, out_rows=None, out_null=False):
    """name -> (values float64 [numel], written bool [numel], bound float64 [numel] | None) for every destination view.
    bound None: bit equality with the values rounded once to the destination's type.  out_rows (f32 [M, N], the rows a launch
    actually wrote): the 16-bit copy, the planes and the row partials are then derived from THOSE rows — for the inexact cases,
    whose `out` is only known within a bound."""
    d = inputs(c) if d is None else d
    V, dV = source_values(c, d)
    shapes = dest_shapes(c)
    res = {}
    for name, (shape, kind) in shapes.items():
        n = int(np.prod(shape))
        res[name] = [np.zeros(n), np.zeros(n, dtype=bool), None if c.exact else np.zeros(n)]
    m = np.arange(c.M, dtype=np.int64)[:, None]
    width = c.HD if c.epi in (EPI_HEADS, EPI_ARENA) else c.N
    g = c if c.epi != EPI_F8 else _as_epi(c, EPI_F16)
    for n0 in range(0, c.N, width):
        n = np.arange(n0, n0 + width, dtype=np.int64)[None, :]
        name, idx = gc.dest_of(g, m + 0 * n, n + 0 * m)
        vals, written, bound = res[name]
        idx = idx.reshape(-1)
        assert idx.min() >= 0 and idx.max() < vals.size and np.unique(idx).size == idx.size, (c.name, name)
        vals[idx] = V[:, n0:n0 + width].reshape(-1)
        written[idx] = True
        if bound is not None:
            bound[idx] = out_bound(c, shapes[name][1], V[:, n0:n0 + width], dV[:, n0:n0 + width]).reshape(-1)
    if out_null:                                # split3 without `out`: the f32 rows are not written at all
        res["out"][1][:] = False
    rows = V if out_rows is None else out_rows.astype(np.float64)
    if c.out16:
        vals, written, _ = res["out16"]
        r32 = torch.from_numpy(np.ascontiguousarray(rows)).float()
        hi = r32.to(T16[c.dtype])
        img = np.zeros((c.cap_rows, c.ldo16))
        w = np.zeros((c.cap_rows, c.ldo16), dtype=bool)
        img[:c.M, :c.N], w[:c.M, :c.N] = hi.double().numpy(), True
        if c.split3:
            lo = (r32 - hi.float()).to(T16[c.dtype])
            img[:c.M, c.plane:c.plane + c.N], w[:c.M, c.plane:c.plane + c.N] = lo.double().numpy(), True
            if c.split3 == 1:
                img[:c.M, 2 * c.plane:2 * c.plane + c.N], w[:c.M, 2 * c.plane:2 * c.plane + c.N] = hi.double().numpy(), True
        vals[:], written[:] = img.reshape(-1), w.reshape(-1)
        # (exact, or derived from the launch's own rows: bit equality; inexact without those rows: nothing to compare with)
        res["out16"][2] = None if (c.exact or out_rows is not None) else np.full(vals.size, np.inf)
    if c.stats:
        vals, written, _ = res["stats"]
        p = rows.reshape(c.M, c.N // 64, 64)
        img = np.zeros((c.cap_rows, c.N // 64, 2))
        img[:c.M, :, 0], img[:c.M, :, 1] = p.sum(2), (p * p).sum(2)
        w = np.zeros(img.shape, dtype=bool)
        w[:c.M] = True
        vals[:], written[:] = img.reshape(-1), w.reshape(-1)
        if not c.exact:
            b = np.zeros(img.shape)
            b[:c.M, :, 0], b[:c.M, :, 1] = stats_bound(np.abs(p).sum(2)), stats_bound((p * p).sum(2))
            res["stats"][2] = b.reshape(-1) if out_rows is not None else np.full(vals.size, np.inf)
    return {k: tuple(v) for k, v in res.items()}


def _as_epi(c, epi):
    return SCase(**{**{f: getattr(c, f) for f in c.__dataclass_fields__}, "epi": epi})


def written_rows(c, got_out):
    """The f32 rows [M, N] of an EPI_F32 launch, from the integer allocation of `out`."""
    n = c.cap_rows * c.ldo
    return values_of(c, "f32", got_out[GUARD:GUARD + n]).reshape(c.cap_rows, c.ldo)[:c.M, :c.N]


# ================================================================================================================ the verdict
def verdict(c, dest, got, vals, written, bound=None):
    """(None or what is wrong with `got` — the whole integer allocation of destination `dest` after the launch —, the worst
    error / bound over the written elements, 0 for bit equality)."""
    shape, kind = dest_shapes(c)[dest]
    _, sentinel = int_type(kind)
    sentinel = np.array(sentinel).astype(got.dtype)
    n = vals.size
    if got.size != n + 2 * GUARD:
        return f"{dest}: allocation of {got.size} elements, expected {n + 2 * GUARD}", np.inf
    if (got[:GUARD] != sentinel).any():
        return f"{dest}: a store landed in the guard in front of the view", np.inf
    if (got[GUARD + n:] != sentinel).any():
        return f"{dest}: a store landed in the guard behind the view", np.inf
    inside = got[GUARD:GUARD + n]
    escaped = np.flatnonzero((inside != sentinel) & ~written)
    where = lambda e: [tuple(int(i) for i in np.unravel_index(x, shape)) for x in e[:4]]
    if escaped.size:
        return f"{dest}: {escaped.size} elements outside the written region were overwritten, first at {where(escaped)}", np.inf
    if bound is None:
        bad = np.flatnonzero((inside != bits_of(c, kind, vals)) & written)
        if bad.size:
            return (f"{dest}: {bad.size} of {int(written.sum())} written elements differ from the exact result, first at {where(bad)}: got "
                    f"{values_of(c, kind, inside[bad[:4]]).tolist()}, want {vals[bad[:4]].tolist()}"), np.inf
        return None, 0.0
    val = values_of(c, kind, inside)[written]
    if not np.isfinite(val).all():
        return f"{dest}: {int((~np.isfinite(val)).sum())} written elements are not finite", np.inf
    ratio = np.abs(val - vals[written]) / bound[written]
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        at = np.flatnonzero(written)[int(ratio.argmax())]
        return f"{dest}: {worst:.2f} of the bound at {where(np.array([at]))}: got {val[int(ratio.argmax())]!r}, want {vals[at]!r}", worst
    return None, worst


# ================================================================================================================ wrong variants
def wrong_inputs(c, d, kind):
    """The inputs a mistaken kernel would in effect have used, for the CPU test of the checker (never a kernel run): statistics of
    row m +- 1, one part dropped or counted twice, a per-column vector read one quad (4 columns) further."""
    w = dict(d)
    st = d["stats_in"]
    if kind in ("row+1", "row-1"):
        w["stats_in"] = np.roll(st, -1 if kind == "row+1" else 1, axis=0)
    elif kind in ("part_dropped", "part_doubled"):
        p = st.shape[1] - 1
        w["stats_in"] = st.copy()
        w["stats_in"][:, p] *= 0.0 if kind == "part_dropped" else 2.0
    else:
        vec = kind.split("_")[0]            # "<vector>_quad"
        key = {"colsum": "colsum", "bias": "bias", "scale": "w_scale", "gamma": "gamma", "beta": "beta"}[vec]
        w[key] = np.roll(d[key], -4)
    return w
