"""Cases, inputs and references for the form / edge tests of `vidil_attention_f32` (tests/test_attention_f32_forms_gpu.py; the
preconditions are asserted without a GPU by tests/test_attention_f32_cases_cpu.py).  Everything here is numpy / torch on the CPU.

The entry point dispatches to seven kernels of csrc/attention.hip; every case names the one it is for (`Case.kernel`) and
`expected_kernel` is a pure-Python copy of the dispatcher's decision that must agree.  Every dimension is the smallest that
reaches its branch: H = 2 or 3 heads (3 makes the unit counts of the wave-per-unit kernels no multiple of 4), at most 8 query
batches.

Random inputs come from numpy's PCG64 streams (bit-identical on every host; torch's seeded CPU normal sampler is not).

Tolerances (`tolerance`):
  * N(0, 1) operands, f32 rows 3e-6, f16 [hi | lo | hi] rows 5e-6: the bounds of tests/test_parity_mode_gpu.py.
  * bf16 [hi | lo | hi] rows from f32 arithmetic (arith 0, the arena form): 3e-6 + 2^-17 |ref| elementwise.  hi keeps 8 significant
    bits and lo keeps 8 bits of a remainder of at most 2^-9 |v|: the pair represents v to 2^-18 |v|; the bound is twice that.
  * MEASURED bounds (`BOUNDS`): arith 1 / 2 / kv16 with bf16 operands, and every spiked case.  Measured on the CPU: 4 x the larger
    of (a) the error of `emulate` — the split arithmetic written down below — and (b) the error of a plain torch f32 computation,
    both against fp64 and both on the values as the output format stores them.  The factor 4 is for the kernels' other summation
    order.  The emulation is never the expected value of a GPU assertion: it only shows that correct code reaches the bound.
"""
import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

SCALE = 0.125
KLAZY = 5.0                     # attention.hip kLazy: attn_split_kernel moves its reference only when a tile outgrows it by this
                                # (the other kernels of the family keep the exact running maximum)
SPIKE_Q = 4.0                   # every spiked query's component along u
SPIKE_STEPS = (0.0, 14.0, 20.0, 34.0)     # added along u to the keys of tile 0, 1, 2, 3: scores step by 7, 3, 7
SPIKE_REST = 0.5                # a spiked query's other components are scaled by this: scores N(0, 0.5^2) around the steps, so
                                # that a tile's maximum is within ~1 of its step and every row takes the steps alike
SENTINEL = -77.0                # exact in f32, f16 and bf16; no output (a convex combination of N(0, 1) values) comes near it
T16 = {"f16": torch.float16, "bf16": torch.bfloat16}
START_GROUPS = (1, 3, 3, 4)     # group_start of the `start` unit form: groups of 2, 0 and 1 query batches; batches 0 and 4 unnamed

VALU, MFMA, SPLIT, RELB, ROW1 = "attn_f32_kernel", "attn_f32_mfma_kernel", "attn_split_kernel", "attn_split_kernel/RELB", "attn_split_row1_kernel"
KV16, ARENA, GATHER = "attn_direct1_kernel/QS", "attn_f32_arena_kernel", "attn_f32_arena_gather_kernel"
KERNELS = (VALU, MFMA, SPLIT, RELB, ROW1, KV16, ARENA, GATHER)
KEY_TILE = {VALU: 64, ROW1: 64, MFMA: 32, SPLIT: 32, RELB: 32, KV16: 32}


@dataclass(frozen=True)
class Case:
    name: str
    kernel: str                 # the kernel this case is for, without its <T16>
    form: str = "dense"         # dense | kv16 | arena
    arith: int = 0
    H: int = 2
    Bq: int = 2
    Nq: int = 1
    Nk: int = 1
    kv_pad: int = 0             # kv_rows - Nk (kv16: on top of the round-up to 32)
    unit: str = "group"         # group (kv_group) | index (kv_index) | start (group_start = START_GROUPS)
    kv_group: int = 1
    kv_len: tuple = None
    causal: bool = False
    causal_off: int = 0
    out: str = "f32"            # f32 rows | f16 | bf16 [hi | lo | hi] rows
    planes: int = 3
    pad: int = 0                # columns behind H*64 in every output plane (f32: in every row)
    spiked: int = 0             # 1: every query batch; 2: the odd ones only (rows that keep their reference while others move it)
    arena_extra: int = 2        # arena_rows - Bq

    @property
    def C(self):
        return self.H * 64

    @property
    def t16(self):
        return "bf16" if self.out == "bf16" else "f16"      # (f32 rows: the wrapper passes dtype16 = f16)

    @property
    def ldo(self):
        return (self.C + self.pad) * (1 if self.out == "f32" else 3)

    @property
    def kv_rows(self):
        return ((self.Nk + 31) // 32 * 32 if self.form == "kv16" else self.Nk) + self.kv_pad

    @property
    def measured(self):
        return bool(self.spiked) or (self.out == "bf16" and (self.arith in (1, 2)))


def unit_map(c):
    """(kv batch of every query batch, -1 where no unit names it; n_kv; kv_index; group_start; max_group)."""
    if c.unit == "index":
        n_kv = c.Bq - 1
        idx = [n_kv - 1 - b for b in range(n_kv)] + [n_kv - 1]          # a permutation, then its first kv batch again
        return np.array(idx), n_kv, idx, None, 0
    if c.unit == "start":
        assert c.Bq == START_GROUPS[-1] + 1
        m = -np.ones(c.Bq, dtype=np.int64)
        for j in range(len(START_GROUPS) - 1):
            m[START_GROUPS[j]:START_GROUPS[j + 1]] = j
        return m, len(START_GROUPS) - 1, None, list(START_GROUPS), 2
    assert c.Bq % c.kv_group == 0
    n_kv = c.Bq // c.kv_group
    return np.arange(c.Bq) // c.kv_group, n_kv, None, None, 0


def max_rows(c):
    return {"index": c.Nq, "start": 2 * c.Nq}.get(c.unit, c.kv_group * c.Nq)


def expected_kernel(c):
    """The dispatcher of vidil_attention_f32 (attention.hip), restated: the kernel instantiation a case launches."""
    t = f"<{c.t16}>"
    if c.form == "arena":
        return (GATHER if c.Nk <= 32 else ARENA) + t
    if c.arith == 1 and c.form == "kv16":
        return KV16 + t
    if c.arith == 1 and max_rows(c) == 1 and c.unit != "start":
        return ROW1 + t
    if c.arith in (1, 2):
        return (RELB if c.arith == 2 else SPLIT) + t
    wide = c.ldo % 12 == 0 if c.out != "f32" else c.ldo % 4 == 0          # (torch allocations are 16-byte aligned)
    return (MFMA if max_rows(c) > 8 and wide else VALU) + t


# ================================================================================================================ the table
def _cases():
    cs = []
    outs = (("f32", 3), ("f16", 3), ("bf16", 3), ("f16", 2), ("bf16", 2))

    def add(name, kernel, o=None, **kw):
        if o is not None:
            kw["out"], kw["planes"] = outs[o % len(outs)]
        cs.append(Case(name=name, kernel=kernel, **kw))

    fam = {VALU: ("valu", 0), MFMA: ("mfma", 0), SPLIT: ("split", 1), RELB: ("relb", 2), ROW1: ("row1", 1)}
    # ---- rows per unit x keys.  MFMA / split: 9, 33, 129 rows (129: a second workgroup with one row and three dead waves) over
    # 1, 31, 32, 33, 65 keys; VALU: 8 rows (both row groups of wave 0) and row1 over 1, 63, 64, 65, 130 keys
    for fi, k in enumerate((MFMA, SPLIT, RELB)):
        n, a = fam[k]
        for i, (Nq, Nk, kvp) in enumerate([(9, 1, 0), (9, 31, 3), (33, 32, 0), (33, 33, 0), (129, 65, 0)]):
            add(f"{n}_q{Nq}_k{Nk}", k, o=i + fi, arith=a, Bq=2, Nq=Nq, Nk=Nk, kv_pad=kvp)
    for i, Nk in enumerate((1, 63, 64, 65, 130)):
        add(f"valu_q8_k{Nk}", VALU, o=i, Bq=4, kv_group=2, Nq=4, Nk=Nk, kv_pad=3 if Nk == 63 else 0)
        add(f"row1_k{Nk}", ROW1, o=i + 1, arith=1, H=3, Bq=5, Nq=1, Nk=Nk, kv_pad=3 if Nk == 63 else 0)
    # ---- the VALU kernel as the fallback for outputs without wide stores: 45 rows per unit = two workgroups, waves 1 - 3, base > 0
    add("valu_fallback_f32_ldo_C+2", VALU, Bq=2, Nq=45, Nk=65, out="f32", pad=2)
    add("valu_fallback_f16_plane_C+1", VALU, Bq=2, Nq=45, Nk=65, out="f16", pad=1)
    add("valu_fallback_bf16_plane_C+1", VALU, Bq=2, Nq=45, Nk=65, out="bf16", pad=1, planes=2)
    # ---- masks
    for fi, k in enumerate((VALU, MFMA, SPLIT, RELB)):
        n, a = fam[k]
        Nq, Nk = (8, 70) if k == VALU else (33, 40)
        add(f"{n}_len_Nk_1_0", k, o=fi, arith=a, Bq=3, Nq=Nq, Nk=Nk, kv_len=(Nk, 1, 0))
        add(f"{n}_causal_off+3", k, o=fi + 1, arith=a, Bq=2, Nq=Nq, Nk=Nk, causal=True, causal_off=3)
        add(f"{n}_causal_off-2", k, o=fi + 2, arith=a, Bq=2, Nq=Nq, Nk=Nk, causal=True, causal_off=-2)
        add(f"{n}_causal_len", k, o=fi + 3, arith=a, Bq=3, Nq=Nq, Nk=Nk, causal=True, kv_len=(Nk, 5, 0))
    add("row1_len", ROW1, o=1, arith=1, H=3, Bq=5, Nk=70, kv_len=(70, 1, 0, 64, 65))
    add("row1_causal_off+3", ROW1, o=2, arith=1, H=3, Bq=5, Nk=70, causal=True, causal_off=3)
    add("row1_causal_off-2", ROW1, o=0, arith=1, H=3, Bq=5, Nk=70, causal=True, causal_off=-2)
    # ---- unit forms
    for fi, k in enumerate((VALU, MFMA, SPLIT, RELB)):
        n, a = fam[k]
        Nq = 4 if k == VALU else 9
        add(f"{n}_kv_index", k, o=fi + 1, arith=a, Bq=4, Nq=Nq, Nk=33, unit="index", kv_pad=3)
        add(f"{n}_group_start", k, o=fi + 2, arith=a, Bq=5, Nq=Nq, Nk=33, unit="start")
    add("row1_kv_index_len", ROW1, o=2, arith=1, H=3, Bq=5, Nk=70, unit="index", kv_len=(70, 3, 65, 0, 64))
    # ---- every output form on every kernel
    for k in (VALU, MFMA, SPLIT, RELB, ROW1):
        n, a = fam[k]
        shape = dict(Bq=4, kv_group=2, Nq=4) if k == VALU else dict(Bq=5, H=3) if k == ROW1 else dict(Bq=2, Nq=33)
        for o, (out, planes) in enumerate(outs):
            add(f"{n}_out_{out}_p{planes}", k, arith=a, Nk=65, out=out, planes=planes, pad=4 * (o % 2), **shape)
    # ---- spiked scores: the running maximum of every row moves late, once by more than kLazy and once by less
    add("valu_spiked", VALU, Bq=4, kv_group=2, Nq=4, Nk=197, spiked=1)
    add("mfma_spiked", MFMA, Bq=2, Nq=33, Nk=97, spiked=1)
    add("mfma_spiked_bf16", MFMA, Bq=2, Nq=33, Nk=97, spiked=1, out="bf16")
    for k in (SPLIT, RELB):
        n, a = fam[k]
        for out in ("f32", "f16", "bf16"):
            add(f"{n}_spiked_{out}", k, arith=a, Bq=2, Nq=33, Nk=97, spiked=1, out=out)
    for out in ("f32", "f16", "bf16"):
        add(f"row1_spiked_{out}", ROW1, arith=1, H=3, Bq=5, Nk=197, spiked=1, out=out)
    # ---- one mapping that kv_group, kv_index and group_start can all describe, on one kernel each (12 rows per query batch), with
    # spikes in every other query batch: the cases of the equal-bits test
    for k in (MFMA, SPLIT, RELB):
        n, a = fam[k]
        for out in ("f16", "bf16"):
            add(f"{n}_mixed_spikes_{out}", k, arith=a, Bq=4, kv_group=2, Nq=12, Nk=97, spiked=2, out=out)
    # ---- kv16: f32 queries against 16-bit K / V fragment tiles (one wave per (kv batch, head))
    for Nk in (1, 31, 32, 33, 768):
        add(f"kv16_k{Nk}", KV16, form="kv16", arith=1, Bq=2, kv_group=2, Nq=3, Nk=Nk, out="f16")
    add("kv16_rows32", KV16, form="kv16", arith=1, Bq=8, kv_group=8, Nq=4, Nk=40, out="f16")
    add("kv16_kv_index", KV16, form="kv16", arith=1, H=3, Bq=4, Nq=3, Nk=40, unit="index", out="f16")
    add("kv16_group_start", KV16, form="kv16", arith=1, H=3, Bq=5, Nq=3, Nk=40, unit="start", out="f16")
    add("kv16_bf16", KV16, form="kv16", arith=1, H=3, Bq=2, kv_group=2, Nq=3, Nk=33, out="bf16")
    add("kv16_planes2", KV16, form="kv16", arith=1, H=3, Bq=2, kv_group=2, Nq=3, Nk=40, out="f16", planes=2, pad=8)
    add("kv16_kv_rows96", KV16, form="kv16", arith=1, Bq=2, kv_group=2, Nq=3, Nk=33, kv_pad=32, out="f16")
    add("kv16_spiked", KV16, form="kv16", arith=1, Bq=2, kv_group=2, Nq=3, Nk=97, spiked=1, out="f16")
    add("kv16_spiked_bf16", KV16, form="kv16", arith=1, Bq=2, kv_group=2, Nq=3, Nk=97, spiked=1, out="bf16")
    # ---- arena: 9 units, anc_ld = Nk + 5, arena_rows = Bq + 2
    for i, Nk in enumerate((1, 8, 9, 31, 32)):
        add(f"arena_gather_k{Nk}", GATHER, o=i, form="arena", H=3, Bq=3, Nk=Nk)
    for i, Nk in enumerate((33, 40, 40, 33, 40)):
        add(f"arena_k{Nk}_{outs[i][0]}_p{outs[i][1]}", ARENA, o=i, form="arena", H=3, Bq=3, Nk=Nk, pad=4 * (i % 2))
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


CASES = _cases()


# ================================================================================================================ inputs
def _rng(c, stream):
    return np.random.default_rng([zlib.crc32(c.name.encode()), stream])


def _randn(c, stream, *shape):
    return torch.from_numpy(_rng(c, stream).standard_normal(shape, dtype=np.float32))


def _spike(c, q, k):
    """q [Bq, Nq, H, 64], k [n_kv, Nk, H, 64] in place: per head a unit vector u; every spiked query's component along u becomes
    SPIKE_Q (its other
    components shrink by SPIKE_REST) and every key's component along u becomes SPIKE_STEPS[its tile of the case's kernel]."""
    u = _randn(c, 9, c.H, 64).double()
    u = (u / u.norm(dim=-1, keepdim=True))
    qd = q.double()
    qd = SPIKE_REST * (qd - (qd * u).sum(-1, keepdim=True) * u) + SPIKE_Q * u
    sel = slice(None) if c.spiked == 1 else slice(1, None, 2)
    q[sel] = qd.float()[sel]
    tile = torch.arange(c.Nk) // KEY_TILE[c.kernel]
    step = torch.tensor(SPIKE_STEPS, dtype=torch.float64)[tile.clamp(max=len(SPIKE_STEPS) - 1)]
    kd = k.double()
    k[:] = (kd - (kd * u).sum(-1, keepdim=True) * u + step[None, :, None, None] * u).float()


@lru_cache(maxsize=None)
def inputs(c):
    """The operands of a case as CPU tensors, laid out as the launch reads them.
      q        f32 [Bq * Nq, C]: columns C .. 2C - 1 of the [.., 3C] matrix qw
      dense    k, v f32 [n_kv * kv_rows, C]: the column halves of the [.., 2C] matrix kvw; rows Nk .. kv_rows - 1 of a kv batch are NaN
      kv16     k, v 16-bit fragment tiles [n_kv, H, kv_rows, 64] (NaN wherever no key lives); k_vals, v_vals: the stored values
      arena    k, v f32 [Nk + 2, arena_rows, C]; anc i32 [Bq, Nk + 5]
      rel_bias f32 [H, ld] (arith 2): N(0, 0.5^2) inside the window a launch may read, NaN outside; rel_off"""
    C, H = c.C, c.H
    _, n_kv, kv_index, group_start, max_group = unit_map(c)
    d = dict(n_kv=n_kv, kv_index=kv_index, group_start=group_start, max_group=max_group)
    qw = _randn(c, 1, c.Bq * c.Nq, 3 * C)
    d["qw"] = qw
    q = qw[:, C:2 * C]
    if c.form == "arena":
        rows = c.Bq + c.arena_extra
        d["k"], d["v"] = _randn(c, 2, c.Nk + 2, rows, C), _randn(c, 3, c.Nk + 2, rows, C)
        d["anc"] = torch.from_numpy(_rng(c, 4).integers(0, rows, (c.Bq, c.Nk + 5)).astype(np.int32))
        d["arena_rows"] = rows
        d["q"] = q
        return d
    kf, vf = _randn(c, 2, n_kv, c.Nk, H, 64), _randn(c, 3, n_kv, c.Nk, H, 64)
    if c.spiked:
        q4 = q.reshape(c.Bq, c.Nq, H, 64).clone()
        _spike(c, q4, kf)
        qw[:, C:2 * C] = q4.reshape(c.Bq * c.Nq, C)
    d["q"] = q
    if c.form == "kv16":
        from vidil_amd.kernels import kv_tile_offsets
        dt = T16[c.t16]
        k16, v16 = kf.to(dt).permute(0, 2, 1, 3).contiguous(), vf.to(dt).permute(0, 2, 1, 3).contiguous()       # [n_kv, H, Nk, 64]
        ko, vo = kv_tile_offsets(c.Nk)
        kt = torch.full((n_kv, H, c.kv_rows * 64), float("nan"), dtype=dt)
        vt = torch.full((n_kv, H, c.kv_rows * 64), float("nan"), dtype=dt)
        kt[:, :, ko.reshape(-1)] = k16.reshape(n_kv, H, -1)
        vt[:, :, vo.reshape(-1)] = v16.reshape(n_kv, H, -1)
        d["k"], d["v"] = kt.view(n_kv, H, c.kv_rows, 64), vt.view(n_kv, H, c.kv_rows, 64)
        d["k_vals"], d["v_vals"] = k16.permute(0, 2, 1, 3).float(), v16.permute(0, 2, 1, 3).float()              # [n_kv, Nk, H, 64]
        return d
    kvw = torch.full((n_kv, c.kv_rows, 2 * C), float("nan"))
    kvw[:, :c.Nk, :C] = kf.reshape(n_kv, c.Nk, C)
    kvw[:, :c.Nk, C:] = vf.reshape(n_kv, c.Nk, C)
    kvw = kvw.view(n_kv * c.kv_rows, 2 * C)
    d["kvw"] = kvw
    d["k"], d["v"] = kvw[:, :C], kvw[:, C:]
    d["k_vals"], d["v_vals"] = kf, vf
    if c.arith == 2:
        rel_off = c.Nq - 1 + 5
        t = torch.full((H, rel_off + c.Nk + 7), float("nan"))
        t[:, rel_off - (c.Nq - 1):rel_off + c.Nk] = 0.5 * _randn(c, 5, H, c.Nq + c.Nk - 1)
        d["rel_bias"], d["rel_off"] = t, rel_off
    return d


def key_limits(c):
    """i64 [Bq, Nq]: min(Nk, kv_len[b], t + causal_off + 1); a row with a limit <= 0 has no key."""
    lim = torch.full((c.Bq, c.Nq), c.Nk, dtype=torch.int64)
    if c.kv_len is not None:
        lim = torch.minimum(lim, torch.tensor(c.kv_len, dtype=torch.int64)[:, None])
    if c.causal:
        lim = torch.minimum(lim, (torch.arange(c.Nq) + c.causal_off + 1)[None, :])
    return lim


def _keys(c):
    """K, V [Bq, H, Nk, 64] f32: every query batch's keys (an unnamed batch borrows kv batch 0; its rows are dropped later)."""
    d = inputs(c)
    if c.form == "arena":
        a, j = d["anc"][:, :c.Nk].long(), torch.arange(c.Nk)[None, :]
        k, v = d["k"][j, a], d["v"][j, a]                                              # [Bq, Nk, C]
    else:
        kvb = torch.from_numpy(unit_map(c)[0]).clamp(min=0)
        k, v = d["k_vals"][kvb].reshape(c.Bq, c.Nk, c.C), d["v_vals"][kvb].reshape(c.Bq, c.Nk, c.C)
    return k.reshape(c.Bq, c.Nk, c.H, 64).permute(0, 2, 1, 3), v.reshape(c.Bq, c.Nk, c.H, 64).permute(0, 2, 1, 3)


def _split(x, dt):
    hi = x.to(dt).float()
    return hi, (x - hi).to(dt).float()


def _dot(a, b):
    """a [.., M, K] . b [.., N, K]^T -> [.., M, N].  In f32 the sum runs over K in order, one rounded product and one rounded add
    per step: elementwise IEEE operations, so every host computes the same bits (a BLAS product's summation order is the
    host's), and the recorded measurements below can be recomputed exactly."""
    if a.dtype == torch.float64:
        return a @ b.transpose(-1, -2)
    acc = torch.zeros(a.shape[:-1] + b.shape[-2:-1], dtype=torch.float32)
    for j in range(a.shape[-1]):
        acc = acc + a[..., :, j, None] * b[..., None, :, j]
    return acc


def _exp(x):
    return torch.exp(x) if x.dtype == torch.float64 else torch.exp(x.double()).float()      # (f32: the correctly rounded value)


@lru_cache(maxsize=None)
def _scores(c, kind):
    """Masked scores [Bq, H, Nq, Nk] (-inf at excluded keys) in "fp64", "f32" or "emu" arithmetic (see _attend)."""
    d = inputs(c)
    wt = torch.float64 if kind == "fp64" else torch.float32
    q = d["q"].reshape(c.Bq, c.Nq, c.H, 64).permute(0, 2, 1, 3)
    k = _keys(c)[0]
    if kind == "emu":
        qh, ql = _split(q * SCALE, T16[c.t16])
        kh, kl = _split(k, T16[c.t16])
        s = _dot(ql, kh) + _dot(qh, kl) + _dot(qh, kh)
    else:
        s = _dot(q.to(wt) * SCALE, k.to(wt))
    keys = torch.arange(c.Nk)
    if c.arith == 2:
        idx = d["rel_off"] + keys[None, :] - torch.arange(c.Nq)[:, None]
        s = s + d["rel_bias"][:, idx].to(wt)
    return s.masked_fill(keys[None, None, None, :] >= key_limits(c)[:, None, :, None], float("-inf"))


def _attend(c, mode):
    """softmax(q k^T * scale [+ bias]) v of a case -> [Bq * Nq, C] float64 (rows of unnamed query batches and rows without a key: 0).
    mode: "fp64"; "f32" (plain f32 arithmetic); "emu0" / "emu5": the split-operand arithmetic of arith 1 / 2 / kv16 — operands
    hi = T16(x), lo = T16(x - hi), products lo.hi + hi.lo + hi.hi in f32, the probabilities split alike — with the exact row
    maximum as the softmax's reference, or a reference KLAZY below it (the stalest one the lazy kernels keep)."""
    emu = mode.startswith("emu")
    s = _scores(c, "emu" if emu else mode)
    live = ((key_limits(c) > 0) & torch.from_numpy(unit_map(c)[0] >= 0)[:, None])[:, None, :, None]      # [Bq, 1, Nq, 1]
    m = s.max(-1, keepdim=True).values
    m = torch.where(live, m, torch.zeros_like(m))
    if mode == "emu5":
        m = m - KLAZY
    e = _exp(s - m)
    l = _dot(e, torch.ones(1, 1, 1, c.Nk, dtype=s.dtype))
    vt = _keys(c)[1].transpose(-1, -2)
    if emu:
        eh, el = _split(e, T16[c.t16])
        vh, vl = _split(vt, T16[c.t16])
        o = _dot(eh, vl) + _dot(el, vh) + _dot(eh, vh)
    else:
        o = _dot(e, vt.to(s.dtype))
    o = torch.where(live, o / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(o))
    return o.permute(0, 2, 1, 3).double().reshape(c.Bq * c.Nq, c.C)


@lru_cache(maxsize=None)
def reference(c):
    """(fp64 [Bq * Nq, C]; written [Bq * Nq] bool: rows of query batches that a unit names; nokey [Bq * Nq] bool: written rows
    whose key limit is <= 0 — they are zeros)."""
    ref = _attend(c, "fp64")
    written = torch.from_numpy(np.repeat(unit_map(c)[0] >= 0, c.Nq))
    nokey = (key_limits(c) <= 0).reshape(-1) & written
    return ref, written, nokey


def scores64(c):
    """fp64 scores [Bq, H, Nq, Nk], -inf at excluded keys."""
    return _scores(c, "fp64")


def stored(c, x):
    """The value a row of the case's output format holds for the f32 result x: f32, or hi + lo of the 16-bit type."""
    x = x.float()
    if c.out == "f32":
        return x.double()
    hi, lo = _split(x, T16[c.out])
    return hi.double() + lo.double()


def emulation_applies(c):
    return c.form != "arena" and c.arith in (1, 2)


def emulate(c, lazy):
    """What the split-operand arithmetic gives on a case, as its output format stores it (float64): `_attend`'s "emu" modes, the
    arithmetic tests/probes/probe_precision_design.py injects into the fp32 oracle.  lazy: the stale reference instead of the maximum."""
    assert emulation_applies(c)
    return stored(c, _attend(c, "emu5" if lazy else "emu0"))


@lru_cache(maxsize=None)
def cpu_errors(c):
    """max |x - fp64| over the written rows for x = (the emulation with the exact maximum, with the stale reference, plain f32
    arithmetic); None where the emulation does not apply."""
    ref, written, _ = reference(c)
    err = lambda x: (x - ref)[written].abs().max().item()
    emu = (err(emulate(c, False)), err(emulate(c, True))) if emulation_applies(c) else (None, None)
    return emu + (err(stored(c, _attend(c, "f32"))),)


def measured_error(c):
    return max(e for e in cpu_errors(c) if e is not None)


# Measured bounds: name -> (bound, the CPU measurement it was taken from: the larger of the emulation's and the f32 computation's
# error against fp64).  bound <= 4 x measurement: tests/test_attention_f32_cases_cpu.py recomputes the measurement (the f32 sums of
# `_dot` run in a fixed order, so it is the same on every host) and asserts it; recorded at 3.8 x.
BOUNDS = {
    "split_q9_k31": (8.64e-05, 2.27e-05),
    "split_q33_k33": (6.05e-05, 1.59e-05),
    "relb_q9_k1": (1.58e-04, 4.15e-05),
    "relb_q33_k32": (7.72e-05, 2.03e-05),
    "row1_k63": (2.04e-05, 5.36e-06),
    "row1_k65": (4.18e-05, 1.10e-05),
    "split_len_Nk_1_0": (8.43e-05, 2.22e-05),
    "split_causal_off-2": (1.68e-04, 4.41e-05),
    "relb_causal_off+3": (1.54e-04, 4.06e-05),
    "row1_causal_off+3": (1.05e-04, 2.77e-05),
    "split_group_start": (8.32e-05, 2.19e-05),
    "relb_kv_index": (6.53e-05, 1.72e-05),
    "row1_kv_index_len": (6.03e-05, 1.59e-05),
    "split_out_bf16_p3": (4.60e-05, 1.21e-05),
    "split_out_bf16_p2": (5.00e-05, 1.31e-05),
    "relb_out_bf16_p3": (7.42e-05, 1.95e-05),
    "relb_out_bf16_p2": (5.22e-05, 1.37e-05),
    "row1_out_bf16_p3": (1.98e-05, 5.22e-06),
    "row1_out_bf16_p2": (3.25e-05, 8.56e-06),
    "valu_spiked": (1.40e-05, 3.69e-06),
    "mfma_spiked": (3.85e-06, 1.01e-06),
    "mfma_spiked_bf16": (5.82e-05, 1.53e-05),
    "split_spiked_f32": (3.39e-06, 8.93e-07),
    "split_spiked_f16": (6.09e-06, 1.60e-06),
    "split_spiked_bf16": (1.56e-04, 4.12e-05),
    "relb_spiked_f32": (7.64e-06, 2.01e-06),
    "relb_spiked_f16": (6.78e-06, 1.78e-06),
    "relb_spiked_bf16": (1.92e-04, 5.06e-05),
    "row1_spiked_f32": (1.36e-05, 3.59e-06),
    "row1_spiked_f16": (1.27e-05, 3.34e-06),
    "row1_spiked_bf16": (1.12e-04, 2.94e-05),
    "mfma_mixed_spikes_f16": (3.52e-06, 9.27e-07),
    "mfma_mixed_spikes_bf16": (5.76e-05, 1.52e-05),
    "split_mixed_spikes_f16": (3.53e-06, 9.28e-07),
    "split_mixed_spikes_bf16": (1.57e-04, 4.13e-05),
    "relb_mixed_spikes_f16": (1.21e-05, 3.18e-06),
    "relb_mixed_spikes_bf16": (1.16e-04, 3.06e-05),
    "kv16_bf16": (2.49e-05, 6.54e-06),
    "kv16_spiked": (3.31e-06, 8.71e-07),
    "kv16_spiked_bf16": (1.12e-04, 2.96e-05),
}


def tolerance(c, ref):
    """Bound on |stored output - fp64| for the GPU test: a float, or an elementwise array for bf16 rows of f32 arithmetic."""
    if c.measured:
        return BOUNDS[c.name][0]
    if c.out == "f32":
        return 3e-6
    if c.out == "f16":
        return 5e-6
    return 3e-6 + 2.0 ** -17 * ref.abs()
