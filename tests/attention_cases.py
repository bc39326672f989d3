"""Cases, inputs and references for the form / edge tests of `vidil_attention`'s staged kernel (attn_lds_kernel) and direct kernel
(attn_direct1_kernel<T, false, 1, TILED>): tests/test_attention_forms_gpu.py; the preconditions are asserted without a GPU by
tests/test_attention_cases_cpu.py.  Everything here is numpy / torch on the CPU.

Every case names the kernel it is for (`Case.kernel`); `expected_kernel` is a pure-Python copy of the dispatch (attention.hip:
attention_dispatch, launch_any, launch_lds, stream_eligible) that must agree, and returns with the instantiation the two launch
properties the kernels branch on: `rb` and the store path.  Every dimension is the smallest that reaches its branch: H = 3 heads
and 2 K/V batches (six direct-kernel units: the second workgroup is half empty) unless a unit form needs more, at most 8 query
batches.

Random inputs come from numpy's PCG64 streams (bit-identical on every host).  Q is N(0, 1) / 8 (the callers scale it by
1 / sqrt(64)), K and V are N(0, 1), V holds no exact zero (a dropped key always shows), and everything a launch must not read is
NaN: K / V rows Nk .. Tk_cap - 1 (Tk_cap = Nk + 5), V^T columns up to NP = round16(Nk) + 16, the slots of a fragment tile past Nk,
Q rows Nq .. Tq_cap - 1 (Tq_cap = Nq + 3).

Bound (`bounds`), elementwise against fp64 of the same 16-bit operands — derived, not measured:
    |got - ref| <= 2 h (A + |ref|) + 1e-7,    A = sum_j p_j |v_j| in fp64,    h = 2^-11 (f16) or 2^-8 (bf16).
The kernels round every probability and the output once to the operand type: h (A + |ref|) to first order; the factor 2 is for
the f32 sums and exp2.  [hi | lo | hi] planes: hi takes that bound, hi + lo takes 2 h (A + h |ref|) + 1e-7.  e4m3 rows:
2 (2^-4 |ref| + 2^-10 + h A) (3 mantissa bits, subnormal spacing 2^-9).  `emulate` writes the kernels' arithmetic down in torch
(P rounded to the type, f32 sums, a reference up to kLazy stale, the rounded / split output); it is never the expected value of
a GPU assertion: the CPU test only shows with it that correct code stays within half of the bound.
"""
import zlib
from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

KLAZY = 5.0                     # attention.hip kLazy: the staged kernel moves a row's reference only when a tile outgrows it by this
LOG2E = 1.4426950408889634
SPIKE_Q = 0.5                   # every spiked query's component along u (queries arrive scaled: 4 / 8)
SPIKE_STEPS = (0.0, 14.0, 20.0, 34.0)     # added along u to the keys of four consecutive 32-key tiles: scores step by 7, 3, 7
SPIKE_REST = 0.5                # a spiked query's other components are scaled by this: scores N(0, 0.5^2) around the steps
SENTINEL = -80.0                # exact in f16, bf16 and e4m3; no output (a convex combination of N(0, 1) values) comes near it
T16 = {"f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
OLD_TOL = {"f16": 3e-3, "bf16": 2e-2}     # rtol = atol of tests/test_kernels_gpu.py::test_attention, all that stood behind these kernels
START_GROUPS = (1, 3, 3, 4)     # group_start of the `start` unit form: groups of 2, 0 and 1 query batches; batches 0 and 4 unnamed
CHUNK = 224                     # keys per staged chunk of the chunked form (attn_lds_kernel<T, 7, NW> over 225 .. 768 keys)

LDS, DIRECT, WAVE, STREAM = "attn_lds_kernel", "attn_direct1_kernel", "attn_wave_kernel", "attn_stream_kernel"
# kernel, 16-bit type, nkt (LDS: 1 .. 9 or "chunked"; DIRECT: "tiled" | "rows"), waves, rounds of row blocks, store path
Launch = namedtuple("Launch", "kernel dt nkt nw rb store")
# rows per unit -> (Nq, kv_group): 129 and 128 put several query batches into one wave
ROWS = {33: (33, 1), 128: (64, 2), 129: (43, 3), 256: (64, 4), 257: (257, 1), 384: (96, 4), 385: (385, 1), 1: (1, 1), 3: (3, 1),
        32: (8, 4)}


@dataclass(frozen=True)
class Case:
    name: str
    kernel: str                 # LDS | DIRECT
    dt: str = "f16"
    H: int = 3
    Bq: int = 2
    Nq: int = 33
    Nk: int = 51
    unit: str = "group"         # group (kv_group) | index (kv_index) | start (group_start = START_GROUPS)
    kv_group: int = 1
    max_group: int = 2          # `start` only: the bound on a group's query batches
    vt: bool = True             # V as V^T [64][NP] in vt_pos order; False: row-major V (NP = 0, staged kernel only)
    tiled: int = 0              # 1 / 2: K and V in 32-key fragment tiles (kv_tiled; direct kernel only)
    tk_extra: int = 0           # tiled: Tk_cap = round32(Nk) + tk_extra
    kv_len: tuple = None
    causal: bool = False
    causal_off: int = 0
    out: str = "plain"          # plain 16-bit rows | planes [hi | lo | hi] | fp8 (e4m3 rows)
    pad: int = 0                # spare columns behind H * 64 of every row / plane
    shift: int = 0              # the output pointer is moved by this many elements off its 16-byte alignment
    spiked: int = 0             # 1: every query batch; 2: the odd ones only (rows that keep their reference beside rows that move it)
    aimed: bool = False         # the "every key is read" construction (aimed_targets) instead of random operands

    @property
    def C(self):
        return self.H * 64

    @property
    def ldo(self):
        return (self.C + self.pad) * (3 if self.out == "planes" else 1)

    @property
    def Tq_cap(self):
        return self.Nq + 3

    @property
    def Tk_cap(self):
        return (self.Nk + 31) // 32 * 32 + self.tk_extra if self.tiled else self.Nk + 5

    @property
    def NP(self):
        return (self.Nk + 15) // 16 * 16 + 16 if self.vt and not self.tiled else 0


def unit_map(c):
    """(kv batch of every query batch, -1 where no unit names it; K/V batches; kv_index; group_start; max_group)."""
    if c.unit == "index":
        n_kv = c.Bq - 1
        idx = [n_kv - 1 - b for b in range(n_kv)] + [n_kv - 1]          # a permutation, then its first kv batch again
        return np.array(idx), n_kv, idx, None, 0
    if c.unit == "start":
        assert c.Bq == START_GROUPS[-1] + 1
        m = -np.ones(c.Bq, dtype=np.int64)
        for j in range(len(START_GROUPS) - 1):
            m[START_GROUPS[j]:START_GROUPS[j + 1]] = j
        return m, len(START_GROUPS) - 1, None, list(START_GROUPS), c.max_group
    assert c.Bq % c.kv_group == 0
    return np.arange(c.Bq) // c.kv_group, c.Bq // c.kv_group, None, None, 0


def max_rows(c):
    return {"index": c.Nq, "start": c.max_group * c.Nq}.get(c.unit, c.kv_group * c.Nq)


def lds_bytes(nkt):
    """K [32 nkt][72] + V^T [64][32 nkt + 8] of 16-bit elements: launch_lds's smem_kv."""
    return nkt * 32 * 72 * 2 + 64 * (nkt * 32 + 8) * 2


def expected_kernel(c, stream_env=None):
    """The dispatch of vidil_attention for Nk <= 768 (attention.hip: attention_dispatch, launch_any, launch_lds, stream_eligible),
    restated.  stream_env: the value of $VIDIL_ATTN_STREAM.  (torch allocations are 16-byte aligned: only `shift` breaks that.)"""
    assert c.Nk <= 768
    rows, nkt = max_rows(c), (c.Nk + 31) // 32
    branch = {"plain": "", "planes": "/planes", "fp8": "/fp8"}[c.out]
    aligned = c.shift == 0
    if nkt == 7 and not (stream_env or "1").startswith("0"):
        wide = c.ldo % 8 == 0 if c.out == "plain" else (c.out == "fp8" and c.ldo % 16 == 0)
        if (not c.vt and not c.tiled and c.kv_len is None and c.unit == "group" and c.kv_group == 1 and not c.causal
                and 128 < rows <= 224 and c.Nk > 192 and wide and aligned):
            return Launch(STREAM, c.dt, 7, 8, 1, "store_rows_stream" + branch)
    if rows <= 32:
        if nkt == 1 and not c.tiled:
            return Launch(WAVE, c.dt, 1, 1, 1, "store_rows_wave" + branch)
        return Launch(DIRECT, c.dt, "tiled" if c.tiled else "rows", 1, 1, "store_rows" + branch)
    nw = 8 if rows > 128 else 4
    t = nkt if nkt <= 9 else 7
    budget = 2 * (lds_bytes(t) + nw * 2048) <= 160 * 1024               # the output scratch beside two resident workgroups
    ostage = budget and c.ldo % 8 == 0 and aligned
    rb = 2 if c.Nk <= t * 32 and nw * 32 < rows <= nw * 48 else 1
    store = "store_rows_lds" if c.out == "plain" and ostage else "store_rows" + branch
    return Launch(LDS, c.dt, nkt if nkt <= 9 else "chunked", nw, rb, store)


def family(c, stream_env=None):
    """The kernels inside one family promise the same bits for a row (the streamed kernel is bit-compared with the staged one)."""
    k = expected_kernel(c, stream_env).kernel
    return LDS if k == STREAM else k


# ================================================================================================================ the table
LEN_POOL = lambda Nk: (0, 1, 31, 32, 33, Nk - 1, Nk, Nk + 3)
# the three shapes of the unit-form, mask and output-form cases (83 keys: NKT = 3, a partial last tile, a straddled 16-key block)
# and the chunked one: name -> (kernel, Nk, Nq, kv_group of the grouped / masked launches)
SHAPES = {"lds4": (LDS, 83, 40, 2), "lds8": (LDS, 83, 140, 2), "direct": (DIRECT, 83, 5, 4), "chunked": (LDS, 449, 40, 2)}


def _cases():
    cs = []

    def add(name, kernel, rows=None, **kw):
        if rows is not None:
            kw["Nq"], kw["kv_group"] = ROWS[rows]
            kw["Bq"] = 2 * kw["kv_group"]
        cs.append(Case(name=name, kernel=kernel, **kw))

    R4, R8 = (33, 128), (129, 256, 257, 384, 385)
    # ---- 1. staged kernel, one chunk: NKT 1 .. 9 x NW {4, 8} x {f16, bf16} x {V^T, row-major V} at Nk = 32 NKT - 13, the rows of
    # the table rotating through them; Nk = 32 NKT for NKT 1, 7, 9
    i = 0
    for nkt in range(1, 10):
        for Nk in (32 * nkt - 13,) + ((32 * nkt,) if nkt in (1, 7, 9) else ()):
            for di, dt in enumerate(("f16", "bf16")):
                for vt in (True, False):
                    for nw in (4, 8):
                        i += 1
                        rows = R4[(i // 2 + di) % 2] if nw == 4 else R8[(i // 2 + nkt + 2 * di) % 5]
                        if nkt == 7 and not vt and rows == 129:
                            rows = 257                  # (129 rows of one batch each on row-major V belong to the streamed kernel)
                        add(f"lds_k{Nk}_nw{nw}_{dt}_{'vt' if vt else 'vrow'}_r{rows}", LDS, rows=rows, dt=dt, Nk=Nk, vt=vt)
    # ---- 2. staged kernel, 224-key chunks
    i = 0
    for Nk in (289, 449, 577, 768):
        for dt in ("f16",) + (("bf16",) if Nk in (449, 768) else ()):
            for vt in (True, False):
                for nw in (4, 8):
                    i += 1
                    rows = R4[i % 2] if nw == 4 else R8[i % 5]
                    add(f"chunked_k{Nk}_nw{nw}_{dt}_{'vt' if vt else 'vrow'}_r{rows}", LDS, rows=rows, dt=dt, Nk=Nk, vt=vt)
    # ---- 3. direct kernel, plain rows + V^T: 33 keys (the smallest count the one-tile wave kernel does not take), 65 = three tiles,
    # 96 / 97 = the first wrap of the two-set register ring
    for Nk in (33, 64, 65, 96, 97, 197, 577, 768):
        for rows in (1, 3, 32):
            for dt in ("f16", "bf16"):
                add(f"direct_k{Nk}_r{rows}_{dt}", DIRECT, rows=rows, dt=dt, Nk=Nk)
    # ---- 4. direct kernel, fragment tiles (NaN in every slot past Nk, and in a whole spare tile with tk_extra)
    for i, Nk in enumerate((1, 17, 32, 33, 65, 197, 768)):
        for j, extra in enumerate((0, 32)):
            for di, dt in enumerate(("f16", "bf16")):
                add(f"tiled_k{Nk}_cap+{extra}_{dt}", DIRECT, rows=(1, 3, 32)[(i + j + di) % 3], dt=dt, Nk=Nk, tiled=1, tk_extra=extra)
    # ---- 5. unit forms
    for sh in ("lds4", "lds8", "direct"):
        k, Nk, Nq, g = SHAPES[sh]
        vt = sh != "lds8"
        add(f"{sh}_kv_group1", k, Bq=2, Nq=Nq, Nk=Nk, vt=vt)
        add(f"{sh}_kv_group{g}", k, Bq=2 * g, Nq=Nq, Nk=Nk, kv_group=g, vt=vt, dt="bf16")
        add(f"{sh}_kv_index", k, Bq=4, Nq=Nq, Nk=Nk, unit="index", vt=vt)
        add(f"{sh}_group_start", k, Bq=5, Nq=Nq, Nk=Nk, unit="start", vt=vt, dt="bf16")
        add(f"{sh}_group_start_bound3", k, Bq=5, Nq=Nq, Nk=Nk, unit="start", max_group=3, vt=vt)
    add("tiled_kv_index", DIRECT, Bq=4, Nq=5, Nk=83, unit="index", tiled=1)
    add("tiled_group_start", DIRECT, Bq=5, Nq=5, Nk=83, unit="start", tiled=2, tk_extra=32)
    # ---- 6. masks: 8 query batches, one kv_len each
    for si, sh in enumerate(("lds4", "lds8", "direct", "chunked")):
        k, Nk, Nq, g = SHAPES[sh]
        g = 4 if sh in ("lds8", "direct") else g            # lds8: 160 rows per unit from the 40-row batches
        Nq = 40 if sh == "lds8" else Nq
        vt = si % 2 == 0 or k == DIRECT
        pool = LEN_POOL(Nk)
        lens = tuple(pool[(3 * b + 1 + si) % 8] for b in range(8))          # neighbours in a wave differ
        add(f"{sh}_len", k, Bq=8, Nq=Nq, Nk=Nk, kv_group=g, kv_len=lens, vt=vt, dt=("f16", "bf16")[si % 2])
        Nc = {"lds8": 140, "chunked": 300}.get(sh, Nq)    # causal limits that pass Nk (lds8) and the first chunk (chunked)
        gc = 1 if sh in ("lds8", "chunked") else g
        for off in (0, 3, -2):
            add(f"{sh}_causal_off{off:+d}", k, Bq=2 * gc, Nq=Nc, Nk=Nk, kv_group=gc, causal=True, causal_off=off, vt=vt,
                dt=("f16", "bf16")[(si + off) % 2])
        add(f"{sh}_causal_len", k, Bq=2 * gc, Nq=Nc, Nk=Nk, kv_group=gc, causal=True, causal_off=3, vt=not vt or k == DIRECT,
            kv_len=tuple((0, 33, Nk, 1, 32, Nk - 1, 31, Nk + 3)[b] for b in range(2 * gc)))
    add("chunked_len_chunk_edges", LDS, Bq=8, Nq=40, Nk=449, kv_group=2, kv_len=(224, 0, 225, 100, 223, 449, 448, 226))
    add("chunked_len_chunk_edges_nw8_vrow", LDS, Bq=8, Nq=40, Nk=449, kv_group=4, kv_len=(100, 225, 0, 224, 449, 1, 224, 225),
        vt=False, dt="bf16")
    # ---- 7. output forms: planes, spare columns, a pointer off its alignment; fp8 rows from NKT 2, 7, 9 and the chunked form
    for sh in ("lds4", "lds8", "direct"):
        k, Nk, Nq, g = SHAPES[sh]
        i = 0
        for out in ("plain", "planes"):
            for pad in (0, 8):
                for shift in (0, 1):
                    i += 1
                    if (out, pad, shift) != ("plain", 0, 0):
                        add(f"{sh}_{out}_pad{pad}_shift{shift}", k, Bq=2 * g, Nq=Nq, Nk=Nk, kv_group=g, out=out, pad=pad, shift=shift,
                            vt=(sh != "lds8") or i % 2 == 0, dt=("f16", "bf16")[i % 2])
    add("tiled_planes_pad8_shift1", DIRECT, Bq=8, Nq=5, Nk=83, kv_group=4, tiled=1, out="planes", pad=8, shift=1)
    add("chunked_planes_pad8_shift1", LDS, rows=129, Nk=449, out="planes", pad=8, shift=1, vt=False)
    for i, Nk in enumerate((51, 211, 275, 449)):
        for j, pad in enumerate((0, 16)):
            rows = (33, 257, 128, 384)[(i + 2 * j) % 4]
            add(f"fp8_k{Nk}_pad{pad}_r{rows}", LDS, rows=rows, Nk=Nk, out="fp8", pad=pad, vt=(i + j) % 2 == 0, dt=("f16", "bf16")[(i + j) % 2])
    # ---- 8. spiked scores: 48 rows per unit of 12-row batches (a wave holds batches 0, 1 and part of 2) and 144 of 36-row ones
    for dt in ("f16", "bf16"):
        for sp in (1, 2):
            add(f"spiked{sp}_k179_{dt}", LDS, Bq=8, Nq=12, Nk=179, kv_group=4, spiked=sp, dt=dt, vt=sp == 1)
            add(f"spiked{sp}_k577_{dt}", LDS, Bq=8, Nq=36, Nk=577, kv_group=4, spiked=sp, dt=dt, vt=sp == 2)
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------- "every key is read"
def aimed_targets(Nk, every):
    """Keys that rows are aimed at.  every: all of them (the staged kernel's single-chunk forms, Nk <= 288).  Otherwise both sides of
    every 32-key tile edge and of every 224-key chunk edge, all 16 keys of the first and of the last 16-key block, the last key."""
    if every:
        return list(range(Nk))
    t = set(range(min(16, Nk))) | set(range((Nk - 1) // 16 * 16, Nk)) | {Nk - 1}
    for e in list(range(32, Nk, 32)) + list(range(CHUNK, Nk, CHUNK)):
        t |= {e - 1, e}
    return sorted(t)


def _aimed_cases():
    cs = []
    # staged, single chunk: every key, NKT 1 .. 9 x both types x both V forms; 4 waves (48 rows per unit) and 8 (130) alternate
    for nkt in range(1, 10):
        for di, dt in enumerate(("f16", "bf16")):
            for vt in (True, False):
                nw = (4, 8)[(nkt + di) % 2]
                Nq, g = ((24, 2), (65, 2))[nw == 8]
                cs.append(Case(name=f"aim_lds_k{32 * nkt - 13}_nw{nw}_{dt}_{'vt' if vt else 'vrow'}", kernel=LDS, dt=dt, Bq=2 * g, Nq=Nq,
                               kv_group=g, Nk=32 * nkt - 13, vt=vt, aimed=True))
    # chunked: the edges
    for i, (Nk, dt) in enumerate((("449", "f16"), ("449", "bf16"), ("768", "f16"), ("577", "bf16"))):
        for vt in (True, False):
            nw = (4, 8)[(i + vt) % 2]
            Nq, g = ((24, 2), (65, 2))[nw == 8]
            cs.append(Case(name=f"aim_chunked_k{Nk}_nw{nw}_{dt}_{'vt' if vt else 'vrow'}", kernel=LDS, dt=dt, Bq=2 * g, Nq=Nq, kv_group=g,
                           Nk=int(Nk), vt=vt, aimed=True))
    # direct: 32 rows per unit, both layouts
    for Nk in (97, 197, 768):
        for dt in ("f16", "bf16"):
            for tiled in (0, 1):
                cs.append(Case(name=f"aim_direct_k{Nk}_{dt}_{'tiled' if tiled else 'rows'}", kernel=DIRECT, dt=dt, Bq=8, Nq=8, kv_group=4,
                               Nk=Nk, tiled=tiled, aimed=True))
    return tuple(cs)


AIMED = _aimed_cases()

# ---------------------------------------------------------------------------------------------- "a row's bits" launches
# Two units of 2 x 60 rows (4 waves; wave 1 holds rows of both batches), a kv_len per batch, the odd batches spiked
BITS_LDS = tuple(Case(name=f"bits_lds_k{Nk}_{dt}_{'vt' if vt else 'vrow'}", kernel=LDS, dt=dt, Bq=4, Nq=60, kv_group=2, Nk=Nk, vt=vt,
                      spiked=2, kv_len=(Nk + 3, 33, 0, Nk - 1))
                 for Nk in (83, 449) for dt in ("f16", "bf16") for vt in (True, False))
# the towers' shape: the streamed kernel unless $VIDIL_ATTN_STREAM=0 or a kv_len table is passed
STREAM_CASE = Case(name="stream_tower", kernel=STREAM, Bq=3, Nq=197, Nk=197, vt=False)


def bits_variants(c):
    """The other launches that tests/test_attention_forms_gpu.py compares a BITS_LDS case with, as far as the dispatch sees them."""
    from dataclasses import replace
    return dict(alone=replace(c, Bq=c.kv_group), index=replace(c, unit="index", kv_group=1),
                start=replace(c, unit="start", max_group=c.kv_group), start_two_rounds=replace(c, unit="start", max_group=5),
                start_third_group=replace(c, unit="start", max_group=3))


def aimed_every(c):
    return c.kernel == LDS and c.Nk <= 288


def aimed_pos(c):
    """i64 [units, H, rows]: the key that row r of (unit, head) is aimed at — slot s takes target s mod (number of targets)."""
    tg = aimed_targets(c.Nk, aimed_every(c))
    units, rows = c.Bq // c.kv_group, c.kv_group * c.Nq
    slots = units * c.H * rows
    assert slots >= len(tg), (c.name, slots, len(tg))
    return torch.tensor([tg[s % len(tg)] for s in range(slots)]).view(units, c.H, rows)


def aimed_want(c):
    """fp64 [Bq * Nq, C]: the value row of every row's target."""
    d, pos = inputs(c), aimed_pos(c)
    units, H, rows = pos.shape
    want = d["v_vals"].double()[torch.arange(units)[:, None, None], torch.arange(H)[None, :, None], pos]       # [units, H, rows, 64]
    return want.view(units, H, c.kv_group, c.Nq, 64).permute(0, 2, 3, 1, 4).reshape(c.Bq * c.Nq, c.C)


# ================================================================================================================ inputs
def _rng(c, stream):
    return np.random.default_rng([zlib.crc32(c.name.encode()), stream])


def _randn(c, stream, *shape):
    return torch.from_numpy(_rng(c, stream).standard_normal(shape, dtype=np.float32))


def spike_tile0(Nk):
    """First of the four stepped tiles: the last four of a single chunk; 12 .. 15 of 577 keys (the steps straddle the chunk edge 448)."""
    return (Nk + 31) // 32 - 4 if Nk <= CHUNK else 12


def _spike(c, q, k):
    """q [Bq, H, Nq, 64], k [n_kv, H, Nk, 64] in place: per head a unit vector u; every spiked query's component along u becomes
    SPIKE_Q (its other components shrink by SPIKE_REST), every other query's becomes 0, and every key's component along u becomes
    SPIKE_STEPS[its tile - tile0]."""
    u = _randn(c, 9, c.H, 64).double()
    u = (u / u.norm(dim=-1, keepdim=True))[None, :, None, :]
    flat = q.double() - (q.double() * u).sum(-1, keepdim=True) * u
    sel = slice(None) if c.spiked == 1 else slice(1, None, 2)
    q[:] = flat.float()              # (spiked == 2: the even batches lose their component along u, so the steps pass them by)
    q[sel] = (SPIKE_REST * flat + SPIKE_Q * u).float()[sel]
    tile = (torch.arange(c.Nk) // 32 - spike_tile0(c.Nk)).clamp(min=0, max=len(SPIKE_STEPS) - 1)
    step = torch.tensor(SPIKE_STEPS, dtype=torch.float64)[tile]
    kd = k.double()
    k[:] = (kd - (kd * u).sum(-1, keepdim=True) * u + step[None, None, :, None] * u).float()


def pack_q(q_vals, Nq, dt):
    """[Bq, H, Nq, 64] values -> the Q buffer [Bq, H, Nq + 3, 64] (NaN rows behind Nq)."""
    Bq, H = q_vals.shape[:2]
    q = torch.full((Bq, H, Nq + 3, 64), float("nan"), dtype=dt)
    q[:, :, :Nq] = q_vals.to(dt)
    return q


def pack_kv(k_vals, v_vals, dt, vt=True, tiled=0, tk_extra=0):
    """[n_kv, H, Nk, 64] values -> (K buffer, V buffer, Tk_cap, NP) in the layout a launch reads, NaN wherever no key lives."""
    from vidil_amd.kernels import kv_tile_offsets, vt_columns

    n_kv, H, Nk, _ = k_vals.shape
    k16, v16 = k_vals.to(dt), v_vals.to(dt)
    if tiled:
        cap = (Nk + 31) // 32 * 32 + tk_extra
        ko, vo = kv_tile_offsets(Nk)
        kt = torch.full((n_kv, H, cap * 64), float("nan"), dtype=dt)
        vtl = torch.full((n_kv, H, cap * 64), float("nan"), dtype=dt)
        kt[:, :, ko.reshape(-1)] = k16.reshape(n_kv, H, -1)
        vtl[:, :, vo.reshape(-1)] = v16.reshape(n_kv, H, -1)
        return kt.view(n_kv, H, cap, 64), vtl.view(n_kv, H, cap, 64), cap, 0
    cap = Nk + 5
    kp = torch.full((n_kv, H, cap, 64), float("nan"), dtype=dt)
    kp[:, :, :Nk] = k16
    if vt:
        NP = (Nk + 15) // 16 * 16 + 16
        vp = torch.full((n_kv, H, 64, NP), float("nan"), dtype=dt)
        vp[..., vt_columns(Nk)] = v16.transpose(-1, -2)
    else:
        NP = 0
        vp = torch.full((n_kv, H, cap, 64), float("nan"), dtype=dt)
        vp[:, :, :Nk] = v16
    return kp, vp, cap, NP


def _aimed_values(c):
    """Row r of (unit, head) is aligned with ONE key (raw score 100, every other at least 25 below: asserted by the CPU test) whose
    value row is a pattern unique to that key, so the row's output is that pattern."""
    units, H = c.Bq // c.kv_group, c.H
    tg, pos = aimed_targets(c.Nk, aimed_every(c)), aimed_pos(c)
    k = _randn(c, 2, units, H, c.Nk, 64)
    k[:, :, tg] *= 10.0 / k[:, :, tg].norm(dim=-1, keepdim=True)
    k = k.to(T16[c.dt]).float()
    v = _randn(c, 3, units, H, c.Nk, 64)
    key, d = torch.tensor(tg), torch.arange(64)
    pat = ((key[None, None, :, None] * 7 + d * 3 + 5 * torch.arange(units)[:, None, None, None] + 11 * torch.arange(H)[None, :, None, None]) % 61 - 30) / 16
    v[:, :, tg] = pat.float()
    kt = k[torch.arange(units)[:, None, None], torch.arange(H)[None, :, None], pos]                               # [units, H, rows, 64]
    q = kt / kt.norm(dim=-1, keepdim=True) * 10.0
    q = q.view(units, H, c.kv_group, c.Nq, 64).permute(0, 2, 1, 3, 4).reshape(c.Bq, H, c.Nq, 64)
    return q, k, v


@lru_cache(maxsize=None)
def inputs(c):
    """The operands of a case on the CPU: q_vals [Bq, H, Nq, 64], k_vals / v_vals [n_kv, H, Nk, 64] (f32 tensors that hold the 16-bit
    values), and q, k, v: the buffers in the layout the launch reads (pack_q, pack_kv), with Tk_cap and NP."""
    dt = T16[c.dt]
    _, n_kv, kv_index, group_start, max_group = unit_map(c)
    if c.aimed:
        q, k, v = _aimed_values(c)
    else:
        q = _randn(c, 1, c.Bq, c.H, c.Nq, 64) * 0.125
        k = _randn(c, 2, n_kv, c.H, c.Nk, 64)
        v = _randn(c, 3, n_kv, c.H, c.Nk, 64) * (3.0 if c.out == "fp8" else 1.0)     # (fp8: outputs above e4m3's subnormals)
        if c.spiked:
            _spike(c, q, k)
    q, k, v = q.to(dt).float(), k.to(dt).float(), v.to(dt).float()
    if not c.aimed:
        v[v == 0] = 2.0 ** -6
    kb, vb, cap, NP = pack_kv(k, v, dt, c.vt, c.tiled, c.tk_extra)
    assert cap == c.Tk_cap and NP == c.NP
    return dict(q_vals=q, k_vals=k, v_vals=v, q=pack_q(q, c.Nq, dt), k=kb, v=vb, n_kv=n_kv, kv_index=kv_index, group_start=group_start,
                max_group=max_group)


def key_limits(c):
    """i64 [Bq, Nq]: min(Nk, kv_len[b], t + causal_off + 1); a row with a limit <= 0 has no key."""
    lim = torch.full((c.Bq, c.Nq), c.Nk, dtype=torch.int64)
    if c.kv_len is not None:
        lim = torch.minimum(lim, torch.tensor(c.kv_len, dtype=torch.int64)[:, None])
    if c.causal:
        lim = torch.minimum(lim, (torch.arange(c.Nq) + c.causal_off + 1)[None, :])
    return lim


def _operands(c, wt):
    d = inputs(c)
    kvb = torch.from_numpy(unit_map(c)[0]).clamp(min=0)          # (an unnamed batch borrows kv batch 0; its rows are dropped later)
    return d["q_vals"].to(wt), d["k_vals"][kvb].to(wt), d["v_vals"][kvb].to(wt)


def _masked(c, s):
    keys = torch.arange(c.Nk)
    return s.masked_fill(keys[None, None, None, :] >= key_limits(c)[:, None, :, None], float("-inf"))


def scores64(c):
    """fp64 scores [Bq, H, Nq, Nk], -inf at excluded keys."""
    q, k, _ = _operands(c, torch.float64)
    return _masked(c, q @ k.transpose(-1, -2))


def _live(c):
    return ((key_limits(c) > 0) & torch.from_numpy(unit_map(c)[0] >= 0)[:, None])[:, None, :, None]      # [Bq, 1, Nq, 1]


def _rows(c, x):
    return x.permute(0, 2, 1, 3).reshape(c.Bq * c.Nq, c.C)


@lru_cache(maxsize=None)
def reference(c):
    """(ref fp64 [Bq * Nq, C]: softmax(q k^T) v of the 16-bit operands, 0 in rows without a key and in unnamed batches;
    A = sum_j p_j |v_j| alike; written [Bq * Nq] bool: rows of query batches that a unit names; nokey [Bq * Nq] bool: written rows
    whose key limit is <= 0)."""
    _, _, v = _operands(c, torch.float64)
    s, live = scores64(c), _live(c)
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = e.sum(-1, keepdim=True)
    p = torch.where(live, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))
    written = torch.from_numpy(np.repeat(unit_map(c)[0] >= 0, c.Nq))
    nokey = (key_limits(c) <= 0).reshape(-1) & written
    return _rows(c, p @ v), _rows(c, p @ v.abs()), written, nokey


def bounds(c):
    """Bound (a), one tensor [Bq * Nq, C] per stored quantity: (plain rows,), (hi, hi + lo) or (e4m3 rows,)."""
    ref, A, _, _ = reference(c)
    h = HALF_ULP[c.dt]
    if c.out == "fp8":
        return (2.0 * (2.0 ** -4 * ref.abs() + 2.0 ** -10 + h * A),)
    first = 2.0 * h * (A + ref.abs()) + 1e-7
    return (first, 2.0 * h * (A + h * ref.abs()) + 1e-7) if c.out == "planes" else (first,)


def stored(c, o):
    """What the case's output form holds for the f32 result o, as float64: matches `bounds` entry by entry."""
    dt = T16[c.dt]
    if c.out == "fp8":
        return (o.to(torch.float8_e4m3fn).double(),)
    hi = o.to(dt).float()
    if c.out == "planes":
        return hi.double(), hi.double() + (o - hi).to(dt).double()
    return (hi.double(),)


def emulate(c, stale):
    """The kernels' arithmetic in torch: f32 scores of the 16-bit operands, p = 2^((s - m) log2 e) in f32 with the reference m the
    row maximum minus `stale` (0, or up to kLazy for the staged kernel's lazy reference), the row sum l of the UNROUNDED p in f32,
    P rounded to the type, f32 sums of P.V, times 1 / l, stored as the output form stores it."""
    q, k, v = _operands(c, torch.float32)
    s, live = _masked(c, q @ k.transpose(-1, -2)), _live(c)
    m = s.max(-1, keepdim=True).values
    m = torch.where(live, m - stale, torch.zeros_like(m))
    e = torch.exp2(s * LOG2E - m * LOG2E)
    l = e.sum(-1, keepdim=True)
    o = (e.to(T16[c.dt]).float() @ v) * torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return stored(c, _rows(c, torch.where(live, o, torch.zeros_like(o))))
