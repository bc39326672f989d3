"""Cases, inputs and exact references for the form / edge tests of `vidil_gemm` (tests/test_gemm_forms_gpu.py; the table's own
preconditions are asserted without a GPU by tests/test_gemm_cases_cpu.py).  Everything here is numpy / torch on the CPU.

One call, several kernel bodies (`FORMS`): the four small-tile instantiations of csrc/gemm.hip (scalar epilogue), gemm256_kernel
(eager form of gemm_epilogue.inc), gemm4w_kernel with 256- and with 128-row tiles (lazy / descriptor-store form) and the in-loop
compensated ("C3", split_k) form of gemm4w_kernel in both tile heights.  Every case names the form it is for (`Case.kernel`);
`expected_kernel` is a pure-Python copy of the dispatcher's decision and returns the name `vidil_gemm_kernel_name` prints.

Operands are SMALL INTEGERS (numpy PCG64 streams, bit-identical on every host), so every partial sum of the product is an
integer below 2^24: any f32 summation order gives the same, exact, result, every expected value is representable in its output
type, and the GPU test asserts bit equality — there is no tolerance.  The only cases with a bound are the activation cases
(`Case.exact == False`): their pre-activations are exact multiples of 1/8 in [-6, 6] and the bound is on the activation alone
(`BOUNDS`, `act_bound`).

Every destination is a view into a larger allocation prefilled with a NaN bit pattern (`SENTINEL16` / `SENTINEL32`), with
`GUARD` elements on both sides, and has capacity beyond what the launch writes (rows behind M, columns behind N, token rows on
both sides of t_off .. t_off + T, unused V^T columns, unused arena slots): `expected` returns, per destination, the values and
the mask of what a correct launch writes; everything else must still hold the sentinel afterwards."""
import math
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

T16 = {"f16": torch.float16, "bf16": torch.bfloat16}
CNAME = {"f16": "_Float16", "bf16": "__bf16"}
EPI_F16, EPI_F32, EPI_HEADS, EPI_PATCH, EPI_ARENA = 0, 1, 2, 3, 4       # include/vidil_hip.h VIDIL_EPI_*
ACT_NONE, ACT_GELU_ERF, ACT_QUICK_GELU = 0, 1, 2

SENTINEL16 = 0x7FEE             # a NaN in f16 and in bf16 (exponent all ones, mantissa non-zero); twice: a NaN in f32
SENTINEL32 = 0x7FEE7FEE
GUARD = 4096                    # elements on each side of every destination view: 8 KiB (16-bit), 16 KiB (f32)
NAN_ROWS = 256                  # NaN rows behind A and behind W: a whole tile of the tallest kernel

S64, S128x64, S128_3, S128_2 = "gemm_kernel<64,64,3>", "gemm_kernel<128,64,2>", "gemm_kernel<128,128,3>", "gemm_kernel<128,128,2>"
G256, W4, W4_128, C3_256, C3_128 = "gemm256_kernel", "gemm4w_kernel/256", "gemm4w_kernel/128", "gemm4w_kernel/256/C3", "gemm4w_kernel/128/C3"
SMALL = (S64, S128x64, S128_3, S128_2)
FORMS = SMALL + (G256, W4, W4_128, C3_256, C3_128)
TILE = {S64: (64, 64), S128x64: (128, 64), S128_3: (128, 128), S128_2: (128, 128), G256: (256, 256), W4: (256, 256),
        W4_128: (128, 256), C3_256: (256, 256), C3_128: (128, 256)}
RING = {S64: 3, S128x64: 2, S128_3: 3, S128_2: 2}
ENV_KEYS = ("VIDIL_GEMM4W", "VIDIL_GEMM4W128")
ENV = {G256: {"VIDIL_GEMM4W": "0"}, W4: {"VIDIL_GEMM4W": "1"}, W4_128: {"VIDIL_GEMM4W128": "1"}}


@dataclass(frozen=True)
class Case:
    name: str
    kernel: str                 # the form (one of FORMS) this case is for
    dtype: str = "f16"          # f16 | bf16: A, W and every 16-bit output
    epi: int = EPI_F16
    act: int = ACT_NONE
    M: int = 1
    N: int = 8
    K: int = 64                 # (C3: all three planes, K = 3 Kl)
    lda_pad: int = 0            # lda = K + lda_pad; the padding columns are NaN
    ldo_pad: int = 0            # ldo = N + ldo_pad (f16 / f32 / patch rows)
    bias: bool = True
    resid: str = "none"         # f32 rows: none | alias (resid is out) | own
    T: int = 1                  # heads / arena: tokens per sequence
    H: int = 1
    part0: int = 0
    t_off: int = 0
    Tq_cap: int = 0
    Tk_cap: int = 0
    NP: int = 0                 # heads: V^T row stride; 0 = V row-major
    tiled: bool = False         # heads: fragment-tiled K / V
    q_scale: float = 0.5
    arena_rows: int = 0
    slot_stride: int = 1
    tpi: int = 0                # patch: patches per image
    split_k: int = 0
    env: dict = field(default_factory=dict, compare=False)      # developer switches (ENV_KEYS) set for the launch; others unset

    @property
    def exact(self):
        return self.act == ACT_NONE

    @property
    def lda(self):
        return self.K + self.lda_pad

    @property
    def ldo(self):
        return self.N + self.ldo_pad

    @property
    def HD(self):
        return self.H * 64

    @property
    def nparts(self):
        return self.N // self.HD

    @property
    def B(self):                # sequences (heads / arena) or images (patch)
        return self.M // (self.tpi if self.epi == EPI_PATCH else self.T)

    @property
    def out_rows(self):         # rows the launch may write in `out`
        return self.M + self.B if self.epi == EPI_PATCH else self.M

    @property
    def cap_rows(self):         # rows of the `out` / arena-Q view: capacity behind the last row, at least an eighth
        return self.out_rows + self.out_rows // 8 + 2


def _cdiv(a, b):
    return -(-a // b)


# ================================================================================================================ the dispatcher
def _eligible256(c, any_size, cus):
    """vidil_gemm256_eligible (gemm256.hip) for 16-bit operands and 16-byte aligned buffers (every view here is)."""
    if _cdiv(c.M, 256) * _cdiv(c.N, 256) < 5 * cus // 8 and not any_size:
        return False
    if c.K < 128 or 256 * c.lda >= 2 ** 31 or c.N * c.K >= 2 ** 31:
        return False
    if c.epi == EPI_F16:
        return c.N % 8 == 0 and c.ldo % 8 == 0
    if c.epi in (EPI_F32, EPI_PATCH):
        return c.N % 4 == 0 and c.ldo % 4 == 0
    return True


def _switch(c, key):
    v = c.env.get(key)
    return None if v is None else int(v)


def _prefer_4w(c, cus):
    if c.epi == EPI_HEADS and c.T < 8:
        return False
    sw = _switch(c, "VIDIL_GEMM4W")
    if sw is not None:
        return sw != 0
    if _cdiv(c.M, 256) * _cdiv(c.N, 256) < 3 * cus // 2:
        return False
    if c.epi in (EPI_F16, EPI_HEADS, EPI_ARENA):
        return True
    return c.epi == EPI_F32 and c.K >= 1536


def _gemm4w128_wanted(c, cus):
    mode = _switch(c, "VIDIL_GEMM4W128")
    if mode == 0 or (c.epi == EPI_HEADS and c.T < 8):
        return False
    if not (c.epi in (EPI_F16, EPI_HEADS, EPI_ARENA) or (c.epi == EPI_F32 and c.act == ACT_NONE)):
        return False
    if not _eligible256(c, True, cus):
        return False
    if mode == 1:
        return True
    t256, t128 = _cdiv(c.M, 256) * _cdiv(c.N, 256), _cdiv(c.M, 128) * _cdiv(c.N, 256)
    return t256 < 5 * cus // 8 and t128 >= 25 * cus // 32 and c.K >= 512


def _c3_serves(c, cus):
    if not c.split_k or c.K % 96 != 0:
        return False
    if not (c.epi in (EPI_F32, EPI_PATCH) or (c.epi == EPI_HEADS and c.T >= 8)):
        return False
    return _eligible256(c, True, cus)


def _choose_tile(c, cus):
    """choose_tile (gemm.hip) -> (big, bm, bn, st): big 2 = the 128-row 4-wave form, 1 = a 256 x 256 kernel, 0 = small tiles."""
    if _gemm4w128_wanted(c, cus):
        return 2, 128, 256, 2
    if _eligible256(c, False, cus):
        return 1, 256, 256, 2
    n128 = _cdiv(c.M, 128) * _cdiv(c.N, 128)
    if n128 >= 25 * cus // 32 and c.N <= 1024:
        return 0, 128, 128, (2 if n128 > cus else 3)
    if _cdiv(c.M, 64) * _cdiv(c.N, 64) <= 5 * cus:
        return 0, 64, 64, 3
    if _cdiv(c.M, 128) * _cdiv(c.N, 64) <= 10 * cus:
        return 0, 128, 64, 2
    return 0, 128, 128, 2


def expected_kernel(c, cus=256):
    """The kernel instantiation vidil_gemm launches for a case, spelled as vidil_gemm_kernel_name prints it: the decision of
    vidil_gemm / pick_tile / vidil_gemm256_launch with the "-1000: not built here" fall-backs of the 4-wave dispatchers."""
    t = CNAME[c.dtype]
    act = c.act if c.epi in (EPI_F16, EPI_F32) else 0
    if _c3_serves(c, cus):
        tm = 4 if (_cdiv(c.M, 256) * _cdiv(c.N, 256) >= 5 * cus // 8 or c.epi == EPI_PATCH) else 2
        # launch4w_c3_tm builds f32 / heads in both heights and patch with 256-row tiles: nothing falls back
        return f"gemm4w_kernel<{t}, {t}, {c.epi}, {act}, false, false, false, {tm}, true>"
    big, bm, bn, st = _choose_tile(c, cus)
    if big == 2:
        # launch4w128_dispatch: f16 (any activation), f32 without activation, heads, arena — what _gemm4w128_wanted admits
        return f"gemm4w_kernel<{t}, {t}, {c.epi}, {act}, false, false, false, 2, false>"
    if big == 1:
        # launch4w_dispatch builds every 16-bit epilogue: -1000 comes back for fp8 operands only
        if _prefer_4w(c, cus):
            return f"gemm4w_kernel<{t}, {t}, {c.epi}, {act}, false, false, false, 4, false>"
        return f"gemm256_kernel<{t}, {t}, {c.epi}, {act}, false, false, false>"
    return f"gemm_kernel<{t}, {bm}, {bn}, {st}, {c.epi}, {act}>"


def form_of(name):
    """The form (one of FORMS) of a kernel name."""
    base, args = name.split("<", 1)
    a = [x.strip() for x in args.rstrip(">").split(",")]
    if base == "gemm_kernel":
        return f"gemm_kernel<{a[1]},{a[2]},{a[3]}>"
    if base == "gemm256_kernel":
        return G256
    return f"gemm4w_kernel/{64 * int(a[-2])}" + ("/C3" if a[-1] == "true" else "")


# ================================================================================================================ the table
def _row_range(form, N):
    """Rows (lo, hi; hi None = unbounded) at which a problem of N columns that no 256-row kernel takes by itself runs on `form`
    (256 CUs): the thresholds of choose_tile / vidil_gemm256_eligible / vidil_gemm4w_c3_launch."""
    c64, c128, c256 = _cdiv(N, 64), _cdiv(N, 128), _cdiv(N, 256)
    need256 = (_cdiv(160, c256) - 1) * 256 + 1
    if form == S64:
        return 1, min((1280 // c64) * 64, (_cdiv(200, c128) - 1) * 128 if N <= 1024 else 10 ** 9)
    if form == S128x64:
        assert N > 1024
        return (1280 // c64) * 64 + 1, (2560 // c64) * 128
    if form == S128_3:
        assert N <= 1024
        return (_cdiv(200, c128) - 1) * 128 + 1, (256 // c128) * 128
    if form == S128_2:         # more than 256 tiles of 128 x 128 within N <= 1024, or choose_tile's last resort for wide problems
        return ((256 // c128) * 128 + 1 if N <= 1024 else (2560 // c64) * 128 + 1), None
    if form in (G256, W4, C3_256):
        return need256, None
    if form == C3_128:
        return 1, need256 - 1
    return 1, None


def _rows(form, N, mrem):
    """A row count on `form` whose last tile holds mrem rows: one tile above the lower end of the range (three tiles where the
    range starts at one row)."""
    lo, hi = _row_range(form, N)
    bm = TILE[form][0]
    tiles = 3 if lo == 1 else _cdiv(lo, bm) + 1
    M = (tiles - 1) * bm + mrem
    assert lo <= M and (hi is None or M <= hi), (form, N, M, lo, hi)
    return M


def _seqs(form, N, T):
    """Sequences of T tokens (at least 3) so that the rows land on `form`, more than one 64-row tile of them."""
    lo, hi = _row_range(form, N)
    B = max(3, _cdiv(70 if lo == 1 else lo + 64, T))
    assert hi is None or B * T <= hi, (form, N, T)
    return B


def _base_k(form):
    return 192 if form in (C3_256, C3_128) else 64 if form in SMALL else 128


def _cols(form):
    return {S64: 3, S128x64: 18, S128_3: 5, S128_2: 5, W4_128: 2, C3_128: 2}.get(form, 5)


def _cases():
    cs = []

    def add(name, form, **kw):
        kw.setdefault("K", _base_k(form))
        kw.setdefault("split_k", 1 if form in (C3_256, C3_128) else 0)
        cs.append(Case(name=f"{_short(form)}_{name}", kernel=form, env=dict(ENV.get(form, {})), **kw))

    for form in FORMS:
        bm, bn = TILE[form]
        ct = _cols(form)
        c3 = form in (C3_256, C3_128)
        epi16 = EPI_F32 if c3 else EPI_F16          # (the C3 form serves no 16-bit rows: its plain cases are all f32 rows)
        n_p8, n_m8, n_p24 = (ct - 1) * bn + 8, ct * bn - 8, (ct - 1) * bn + 24
        n_mid = (ct - 1) * bn + (72 if bn >= 128 else 40)
        # ---- row and column tails, ldo > N; plain 16-bit rows and the four f32 variants (resid alias / own / none, no bias)
        add("m1_n+8", form, epi=epi16, M=_rows(form, n_p8, 1), N=n_p8)
        add("m3_n-8_ldo+8_resid_alias", form, dtype="bf16", epi=EPI_F32, resid="alias", M=_rows(form, n_m8, 3), N=n_m8, ldo_pad=8)
        add("m-1_n+24", form, dtype="bf16", epi=epi16, M=_rows(form, n_p24, bm - 1), N=n_p24)
        add("mfull_nmid_ldo+16_resid_own", form, epi=EPI_F32, resid="own", M=_rows(form, n_mid, bm), N=n_mid, ldo_pad=16)
        add("m5_n+8_f32_nobias", form, epi=EPI_F32, bias=False, M=_rows(form, n_p8, 5), N=n_p8)
        add("m-1_n-8_f32", form, dtype="bf16", epi=EPI_F32, M=_rows(form, n_m8, bm - 1), N=n_m8, ldo_pad=4)
        add("m3_n+24_ldo+8", form, epi=epi16, M=_rows(form, n_p24, 3), N=n_p24, ldo_pad=8)
        # ---- M below one tile (<128,128,3> needs 200 .. 256 tiles within N <= 1024: at least 25 tile rows; <128,128,2> is also
        # choose_tile's last resort, for N > 1024 with more than 2,560 tiles of 128 x 64: one tile row of 2,562 column tiles)
        if form != S128_3:
            wide = {S128x64: 1281 * 64 + 8, S128_2: 2561 * 64 + 8, G256: 160 * 256 - 8, W4: 160 * 256 - 8, C3_256: 160 * 256 - 8, W4_128: 248, C3_128: 248}.get(form, n_p8)     # (248: one tile)
            add("M1", form, epi=epi16, M=1, N=wide, ldo_pad=8)
            add("M5", form, dtype="bf16", epi=EPI_F32, resid="alias", M=5, N=wide)
        if form == S128_2:                  # a row tail on the wide route as well: 2 x 1,282 tiles of 128 x 64
            add("wide_m3_n+8", form, M=_rows(form, 1281 * 64 + 8, 3), N=1281 * 64 + 8)
            add("wide_m-1_n+8_f32", form, dtype="bf16", epi=EPI_F32, resid="own", M=_rows(form, 1281 * 64 + 8, bm - 1), N=1281 * 64 + 8, ldo_pad=4)
        if form in SMALL:
            # ---- odd N, ldo no multiple of the vector width
            n_odd = 1097 if form == S128x64 else 1001 if form == S64 else 633
            add("n_odd_ldo+3", form, M=_rows(form, n_odd, 3), N=n_odd, ldo_pad=3)
            add("n_odd_f32_ldo+1", form, dtype="bf16", epi=EPI_F32, resid="own", M=_rows(form, n_odd, bm - 1), N=n_odd, ldo_pad=1)
            # ---- K / 64 = 2, 3, 5 against the ring depth (1: every other case), lda = K + 8 and K + 64
            for kt, pad, dt in ((1, 8, "bf16"), (2, 8, "f16"), (3, 64, "bf16"), (5, 0, "f16"), (5, 64, "bf16")):
                add(f"k{kt}_lda+{pad}", form, dtype=dt, epi=EPI_F32 if kt == 3 else EPI_F16, K=64 * kt, lda_pad=pad,
                    M=_rows(form, n_p8, 3), N=n_p8)
        else:
            add("lda+8", form, epi=epi16, lda_pad=8, M=_rows(form, n_m8, 1), N=n_m8)
        # ---- the persistent grid: 1 tile (M1 / M5 above), 9 tiles (16 workgroups), a count above the CUs that is no multiple of 8
        if form in (W4_128, C3_128):
            add("tiles9", form, epi=epi16, M=2 * bm + 3, N=2 * 256 + 8)
            add("tiles260", form, dtype="bf16", epi=EPI_F32, resid="alias", M=64 * bm + 5, N=3 * 256 + 24)
        if form in (G256, W4, C3_256):
            add("tiles261", form, dtype="bf16", epi=epi16, M=28 * 256 + 3, N=8 * 256 + 72)
        if c3:
            add("Kl128_resid_own", form, dtype="bf16", epi=EPI_F32, resid="own", K=384, M=_rows(form, n_p8, 3), N=n_p8, ldo_pad=4)
        # ---- activations on exact pre-activations (multiples of 1/8 in [-6, 6])
        acts = [("gelu16", epi16, ACT_GELU_ERF, "f16"), ("gelu16", epi16, ACT_GELU_ERF, "bf16"), ("quick16", epi16, ACT_QUICK_GELU, "bf16"),
                ("gelu32", EPI_F32, ACT_GELU_ERF, "f16"), ("gelu32", EPI_F32, ACT_GELU_ERF, "bf16"), ("quick32", EPI_F32, ACT_QUICK_GELU, "bf16")]
        for nm, epi, act, dt in acts:
            if (c3 and nm.endswith("16")) or (form == W4_128 and epi == EPI_F32):
                continue                    # (no 16-bit rows in the C3 form; the 128-row form is not built for f32 + activation)
            add(f"{nm}_{dt}", form, dtype=dt, epi=epi, act=act, M=_rows(form, n_p8, 3), N=n_p8, ldo_pad=8)

        # ---- heads: T x (H, parts) x V layout x t_off
        if True:
            big_h = form == S128x64                 # (N > 1024 there: 6 heads and more)
            variants = [  # (H, part0, parts, layout, t_off)
                (3, 0, 3, "vt", 5), (1, 0, 1, "row", 0), (3, 1, 2, "tiled", 3), (1, 0, 3, "row", 2),
                (3, 1, 2, "vt", 6), (3, 0, 3, "tiled", 7), (1, 1, 2, "row", 4)]
            for i, T in enumerate((1, 7, 8, 9, 17, 33, 300)):
                if T < 8 and form in (W4, W4_128, C3_256, C3_128):
                    continue                # (routed to the 8-wave / small-tile kernels: prefer_4w, vidil_gemm_c3_serves)
                H, part0, parts, layout, t_off = variants[i]
                if big_h:
                    H = {1: 17, 2: 9, 3: 6}[parts]
                _add_heads(add, form, T, H, part0, parts, layout, t_off, "bf16" if i % 2 else "f16")
            # every V layout and Q alone / K|V on every form, whatever T left out above
            _add_heads(add, form, 9, 17 if big_h else 1, 0, 1, "row", 0, "bf16", tag="_q_alone")
            _add_heads(add, form, 17, 9 if big_h else 3, 1, 2, "tiled", 3, "f16", tag="_kv")
            _add_heads(add, form, 33, 6 if big_h else 3, 0, 3, "row", 2, "bf16", tag="_qkv")
            _add_heads(add, form, 33, 6 if big_h else 3, 0, 3, "vt", 13, "f16", tag="_shifted")    # vt(t_off + t): blocks entered midway
        if not c3:
            # ---- arena: T = 1 / slot_stride 1 and T = 5 / slot_stride 3, spare arena rows, t_off > 0, part0 0 and 1
            for T, stride, part0, parts, dt in ((1, 1, 0, 3, "f16"), (5, 3, 0, 3, "bf16"), (5, 3, 1, 2, "f16"), (1, 1, 1, 2, "bf16")):
                H = ({3: 6, 2: 9}[parts]) if form == S128x64 else 3
                N = parts * H * 64
                B = _seqs(form, N, T)
                add(f"arena_T{T}_s{stride}_p{part0}", form, dtype=dt, epi=EPI_ARENA, M=B * T, N=N, T=T, H=H, part0=part0, t_off=2,
                    Tk_cap=2 + T + 2, arena_rows=(B - 1) * stride + 1 + 2, slot_stride=stride)
        if form not in (W4_128, C3_128):
            # ---- patch: many images start inside one tile; the class rows stay untouched
            for tpi, dt in ((1, "f16"), (4, "bf16"), (49, "f16")):
                N = (ct - 1) * bn + 8
                B = _seqs(form, N, tpi)
                add(f"patch_tpi{tpi}", form, dtype=dt, epi=EPI_PATCH, M=B * tpi, N=N, tpi=tpi, ldo_pad=8,
                    K=384 if (c3 and tpi == 4) else _base_k(form))
        if form == C3_256:
            # ---- the patch epilogue takes 256-row tiles at ANY size (vidil_gemm4w_c3_launch): the one way to this kernel's grid
            # below 8 workgroups, to 9 tiles on 16 workgroups and to M below one tile
            add("patch_tpi4_tiles1", form, epi=EPI_PATCH, M=3 * 4, N=248, tpi=4, ldo_pad=8)
            add("patch_tpi1_M5_tiles2", form, dtype="bf16", epi=EPI_PATCH, M=5, N=256 + 8, tpi=1, ldo_pad=4)
            add("patch_tpi49_tiles9", form, dtype="bf16", epi=EPI_PATCH, M=11 * 49, N=2 * 256 + 8, tpi=49, ldo_pad=8, K=384)
            add("patch_tpi4_tiles9", form, epi=EPI_PATCH, M=129 * 4 + 0, N=3 * 256 - 8, tpi=4, ldo_pad=4)
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def _short(form):
    return {S64: "s64", S128x64: "s128x64", S128_3: "s128x3", S128_2: "s128x2", G256: "g256", W4: "w4", W4_128: "w4h", C3_256: "c3",
            C3_128: "c3h"}[form]


def _add_heads(add, form, T, H, part0, parts, layout, t_off, dt, tag=""):
    N = parts * H * 64
    B = _seqs(form, N, T)
    span = t_off + T
    kw = dict(T=T, H=H, part0=part0, t_off=t_off if part0 + parts > 1 else 0, Tq_cap=T + T // 8 + 2)
    if layout == "tiled":
        kw.update(tiled=True, Tk_cap=_cdiv(span + span // 8 + 1, 32) * 32)
    elif layout == "vt":
        kw.update(Tk_cap=span + span // 8 + 2, NP=_cdiv(span + span // 8 + 1, 16) * 16)
    else:
        kw.update(Tk_cap=span + span // 8 + 2)
    add(f"heads_T{T}_H{H}_p{part0}x{parts}_{layout}{tag}", form, dtype=dt, epi=EPI_HEADS, M=B * T, N=N,
        q_scale=0.5 if T % 2 else 0.25, **kw)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ================================================================================================================ inputs
def _rng(c, stream):
    return np.random.default_rng([zlib.crc32(c.name.encode()), stream])


def _ints(c, stream, shape, lo, hi, density=1.0):
    g = _rng(c, stream)
    x = g.integers(lo, hi + 1, size=shape).astype(np.float64)
    if density < 1.0:
        x *= g.random(shape) < density
    return x


def inputs(c):
    """The operands of a case, float64 numpy arrays holding values exact in the case's types:
      A [M, K], W [N, K], bias [N] | None, resid [M, N] | None, pos [tpi + 1, N] | None.
    Exact cases: A in {-2 .. 2} (bf16: {-1, 0, 1} at density 1/4), W in {-2 .. 2}, bias / resid / pos integers.  C3 cases: A =
    [x_hi | x_lo | x_hi], W = [W_hi | W_hi | W_lo] of such integers.  Activation cases: one 1 per A row, W in eighths within
    [-5, 5], bias in {-1, 0, 1}: the pre-activation is W[n, k(m)] + bias[n], exact."""
    M, N, K = c.M, c.N, c.K
    d = {}
    if not c.exact:
        A = np.zeros((M, K))
        kk = _rng(c, 1).integers(0, K // 3 if c.split_k else K, size=M)
        A[np.arange(M), kk] = 1.0
        if c.split_k:
            A[:, 2 * (K // 3):] = A[:, :K // 3]
        W = _ints(c, 2, (N, K // 3 if c.split_k else K), -40, 40) / 8.0
        if c.split_k:
            W = np.concatenate([W, W, np.zeros_like(W)], axis=1)
    elif c.split_k:
        Kl = K // 3
        dens = 0.25 if c.dtype == "bf16" else 1.0
        amax = 1 if c.dtype == "bf16" else 2
        xh, xl = _ints(c, 1, (M, Kl), -amax, amax, dens), _ints(c, 3, (M, Kl), -1, 1, dens)
        wh, wl = _ints(c, 2, (N, Kl), -2, 2), _ints(c, 4, (N, Kl), -1, 1)
        A, W = np.concatenate([xh, xl, xh], axis=1), np.concatenate([wh, wh, wl], axis=1)
    else:
        if c.dtype == "bf16":
            A = _ints(c, 1, (M, K), -1, 1, 0.25)
        else:
            A = _ints(c, 1, (M, K), -2, 2)
        W = _ints(c, 2, (N, K), -2, 2)
    d["A"], d["W"] = A, W
    d["bias"] = (_ints(c, 5, (N,), -1, 1) if not c.exact else _ints(c, 5, (N,), -4, 4)) if c.bias else None
    d["resid"] = _ints(c, 6, (M, N), -8, 8) if c.resid != "none" else None
    d["pos"] = _ints(c, 7, (c.tpi + 1, N), -8, 8) if c.epi == EPI_PATCH else None
    return d


def operand_tensors(c, d):
    """(A16 [M + NAN_ROWS, lda], W16 [N + NAN_ROWS, K]) torch tensors of the case's type: NaN in A's padding columns and in the
    rows behind A and behind W — an over-read that reaches a result shows up as a NaN there."""
    dt = T16[c.dtype]
    A = torch.full((c.M + NAN_ROWS, c.lda), float("nan"), dtype=dt)
    A[:c.M, :c.K] = torch.from_numpy(d["A"]).to(dt)
    W = torch.full((c.N + NAN_ROWS, c.K), float("nan"), dtype=dt)
    W[:c.N] = torch.from_numpy(d["W"]).to(dt)
    return A, W


# ================================================================================================================ the reference
def vt_col(t):
    """Storage column of key t in a V^T row: every 16-key block holds its keys in the order 0-3, 8-11, 4-7, 12-15."""
    return t ^ (12 * (((t >> 2) ^ (t >> 3)) & 1))


def ktile_off(t, d):
    """K tile [d / 8][key % 32][d % 8], 2048 elements per 32 keys."""
    return (t // 32) * 2048 + ((d // 8) * 32 + t % 32) * 8 + d % 8


def vtile_off(t, d):
    """V tile [key % 32 / 16][d / 32][g % 2][d % 32][(g / 2) * 4 + key % 4], g = (key % 16) / 4."""
    key = t % 32
    g = (key % 16) // 4
    return (t // 32) * 2048 + ((((key // 16) * 2 + d // 32) * 2 + g % 2) * 32 + d % 32) * 8 + (g // 2) * 4 + key % 4


def dest_shapes(c):
    """name -> (shape, "t16" | "f32") of every destination view of a case."""
    if c.epi in (EPI_F16, EPI_F32, EPI_PATCH):
        return {"out": ((c.cap_rows, c.ldo), "t16" if c.epi == EPI_F16 else "f32")}
    parts = range(c.part0, c.part0 + c.nparts)
    s = {}
    if c.epi == EPI_ARENA:
        if 0 in parts:
            s["q"] = ((c.cap_rows, c.HD), "t16")
        if 1 in parts:
            s["k"] = ((c.Tk_cap, c.arena_rows, c.HD), "t16")
        if 2 in parts:
            s["vt"] = ((c.Tk_cap, c.arena_rows, c.HD), "t16")
        return s
    if 0 in parts:
        s["q"] = ((c.B, c.H, c.Tq_cap, 64), "t16")
    if 1 in parts:
        s["k"] = ((c.B, c.H, c.Tk_cap, 64), "t16")
    if 2 in parts:
        s["vt"] = ((c.B, c.H, 64, c.NP) if (c.NP and not c.tiled) else (c.B, c.H, c.Tk_cap, 64), "t16")
    return s


def dest_of(c, m, n):
    """Where source element (m, n) of the product goes: (destination name, flat element index in its view).  The formulas are
    per element; `expected` evaluates them on integer arrays of one shape whose columns all lie in one part (the first column
    then names the part; every other operation is elementwise).  tests/test_gemm_cases_cpu.py writes the maps a second time,
    element by element in plain loops, and compares."""
    if c.epi in (EPI_F16, EPI_F32):
        return "out", m * c.ldo + n
    if c.epi == EPI_PATCH:
        return "out", (m + m // c.tpi + 1) * c.ldo + n
    part = c.part0 + (n // c.HD if np.isscalar(n) else int(n.flat[0]) // c.HD)
    hcol = n % c.HD
    h, d = hcol // 64, hcol % 64
    b, t = m // c.T, m % c.T
    if c.epi == EPI_ARENA:
        if part == 0:
            return "q", m * c.HD + hcol
        return ("k", "vt")[part - 1], ((c.t_off + t) * c.arena_rows + b * c.slot_stride) * c.HD + hcol
    bh = b * c.H + h
    if part == 0:
        return "q", (bh * c.Tq_cap + t) * 64 + d
    if c.tiled:
        return ("k", "vt")[part - 1], bh * c.Tk_cap * 64 + (ktile_off(c.t_off + t, d) if part == 1 else vtile_off(c.t_off + t, d))
    if part == 1 or c.NP == 0:
        return ("k", "vt")[part - 1], (bh * c.Tk_cap + c.t_off + t) * 64 + d
    return "vt", (bh * 64 + d) * c.NP + vt_col(c.t_off + t)


def pre_activation(c, d):
    """A . W^T + bias in float64: exact (integers, or eighths in the activation cases)."""
    P = d["A"] @ d["W"].T
    if d["bias"] is not None:
        P = P + d["bias"][None, :]
    return P


def activation64(act, x):
    if act == ACT_GELU_ERF:
        return x * 0.5 * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())
    if act == ACT_QUICK_GELU:
        return x / (1.0 + np.exp(-1.702 * x))
    return x


def source_values(c, d):
    """float64 [M, N]: what the epilogue hands to the store for source element (m, n), before the rounding to the output type."""
    P = activation64(c.act, pre_activation(c, d))
    if c.epi == EPI_F32 and d["resid"] is not None:
        P = P + d["resid"]
    if c.epi == EPI_PATCH:
        P = P + d["pos"][np.arange(c.M) % c.tpi + 1, :]
    if c.epi in (EPI_HEADS, EPI_ARENA) and c.part0 == 0:
        P = P.copy()
        P[:, :c.HD] *= c.q_scale
    return P


def expected(c, d=None):
    """name -> (values float64 [numel of the view], written bool [numel], count int32 [numel]: sources per element) for every
    destination view of a case."""
    d = inputs(c) if d is None else d
    V = source_values(c, d)
    out = {}
    for name, (shape, _) in dest_shapes(c).items():
        n = int(np.prod(shape))
        out[name] = (np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int32))
    m = np.arange(c.M, dtype=np.int64)[:, None]
    width = c.HD if c.epi in (EPI_HEADS, EPI_ARENA) else c.N             # one part (or the whole row) at a time
    for n0 in range(0, c.N, width):
        n = np.arange(n0, n0 + width, dtype=np.int64)[None, :]
        name, idx = dest_of(c, m + 0 * n, n + 0 * m)
        vals, written, count = out[name]
        idx = idx.reshape(-1)
        assert idx.min() >= 0 and idx.max() < vals.size, (c.name, name)
        vals[idx] = V[:, n0:n0 + width].reshape(-1)
        written[idx] = True
        count += np.bincount(idx, minlength=vals.size).astype(np.int32)
    return out


def magnitude(c, d):
    """max over (m, n) of sum_k |a| |w| + |bias| + |resid| + |pos|: below 2^24 every f32 summation order is exact."""
    S = np.abs(d["A"]) @ np.abs(d["W"]).T
    if d["bias"] is not None:
        S = S + np.abs(d["bias"])[None, :]
    if d["resid"] is not None:
        S = S + np.abs(d["resid"])
    if d["pos"] is not None:
        S = S + np.abs(d["pos"]).max()
    return float(S.max())


# ================================================================================================================ activation bounds
# f32 rows: the error of torch's own f32 evaluation against float64 on the pre-activations of the activation cases (every
# multiple of 1/8 in [-6, 6]), times 4 for a different but equally legitimate f32 evaluation order.  name -> (bound, measurement).
# tests/test_gemm_cases_cpu.py recomputes the measurement.  16-bit rows: erf-GELU is the polynomial of csrc/common.h, held to the
# bounds of test_polynomial_gelu_of_16bit_outputs_vs_erf_gelu + half an ulp of the output; quick-GELU is evaluated in f32 and
# rounded once: the f32 bound + half an ulp.
GRID = np.arange(-48, 49) / 8.0
BOUNDS = {
    "gelu_erf_f32": (2.24e-06, 5.61e-07),
    "quick_gelu_f32": (1.85e-06, 4.63e-07),
}
GELU16_ABS = {"f16": 4.5e-5, "bf16": 2.0e-4}


def measure_f32_activation(act):
    """max |torch f32 activation - float64| over GRID."""
    x = torch.from_numpy(GRID).float()
    y = torch.nn.functional.gelu(x) if act == ACT_GELU_ERF else x * torch.sigmoid(1.702 * x)
    return float(np.abs(y.double().numpy() - activation64(act, GRID)).max())


def act_bound(c, ref):
    """Elementwise bound on |stored - float64| of an activation case (ref: the float64 expected values)."""
    f32 = BOUNDS["gelu_erf_f32" if c.act == ACT_GELU_ERF else "quick_gelu_f32"][0]
    if c.epi == EPI_F32:
        return np.full(ref.shape, f32)
    mant, emin = (10, -14) if c.dtype == "f16" else (7, -126)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** emin))) - mant)
    return (GELU16_ABS[c.dtype] if c.act == ACT_GELU_ERF else f32) + 0.5 * ulp


# ================================================================================================================ the verdict
def int_type(kind):
    return (np.int32, SENTINEL32) if kind == "f32" else (np.int16, SENTINEL16)


def float_type(c, kind):
    return torch.float32 if kind == "f32" else T16[c.dtype]


def bits_of(c, kind, vals):
    """The bit patterns of float64 values in a destination's type, as the integer type the allocations are compared in."""
    it = torch.int32 if kind == "f32" else torch.int16
    return torch.from_numpy(np.ascontiguousarray(vals)).to(float_type(c, kind)).view(it).numpy()


def verdict(c, dest, got, vals, written):
    """None, or what is wrong with `got` — the whole integer allocation of destination `dest` after the launch: GUARD elements,
    the view, GUARD elements — against the expected values and written mask of `expected`."""
    shape, kind = dest_shapes(c)[dest]
    _, sentinel = int_type(kind)
    n = vals.size
    if got.size != n + 2 * GUARD:
        return f"{dest}: allocation of {got.size} elements, expected {n + 2 * GUARD}"
    if (got[:GUARD] != sentinel).any():
        return f"{dest}: a store landed in the guard in front of the view"
    if (got[GUARD + n:] != sentinel).any():
        return f"{dest}: a store landed in the guard behind the view"
    inside = got[GUARD:GUARD + n]
    escaped = np.flatnonzero((inside != sentinel) & ~written)
    if escaped.size:
        return (f"{dest}: {escaped.size} elements outside the written region were overwritten, first at "
                f"{[tuple(int(i) for i in np.unravel_index(e, shape)) for e in escaped[:4]]}")
    ft = float_type(c, kind)
    if c.exact:
        bad = np.flatnonzero((inside != bits_of(c, kind, vals)) & written)
        if bad.size:
            return (f"{dest}: {bad.size} of {int(written.sum())} written elements differ from the exact result, first at "
                    f"{[tuple(int(i) for i in np.unravel_index(e, shape)) for e in bad[:4]]}: got "
                    f"{torch.from_numpy(inside[bad[:4]].copy()).view(ft).tolist()}, want {vals[bad[:4]].tolist()}")
        return None
    val = torch.from_numpy(inside.copy()).view(ft).double().numpy()[written]
    if not np.isfinite(val).all():
        return f"{dest}: {int((~np.isfinite(val)).sum())} written elements are not finite"
    err = np.abs(val - vals[written])
    worst = float((err / act_bound(c, vals[written])).max())
    if worst > 1.0:
        return f"{dest}: max |d| vs float64 {err.max():.3e}: {worst:.2f} of the bound"
    return None
