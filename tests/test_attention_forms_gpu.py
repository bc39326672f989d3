"""The staged kernel (attn_lds_kernel<T, NKT, NW>, single chunk and 224-key chunks) and the direct kernel (attn_direct1_kernel<T,
false, 1, TILED>) of `vidil_attention` in every instantiation, unit form, mask edge and output form, against fp64 of the same
16-bit operands (tests/attention_cases.py has the case table, the reference and the bound with its derivation; its preconditions
are asserted by tests/test_attention_cases_cpu.py).

(a) every case, element by element: |got - ref| <= 2 h (A + |ref|) + 1e-7 (planes and e4m3 rows: see attention_cases.bounds).  Every
    output buffer starts as a sentinel: after the launch the spare columns of a row or plane, the rows of query batches that no
    group names and the rows behind Bq * Nq still hold it; a row without an admissible key is exactly zero, hi and lo alike.
(b) every key is read: rows aimed at one key each, whose value row is a pattern unique to the key.
(c) a row's bits do not depend on the launch around it, within one kernel family.

Worst |got - ref| / bound over the cases of a kernel, measured on an MI355X (printed per case by `_check`; 355 tests, 4.2 s):
    attn_lds_kernel, single chunk    16-bit rows 0.38 (f16), 0.38 (bf16); planes 0.30, 0.28; e4m3 rows 0.46, 0.44
    attn_lds_kernel, 224-key chunks  16-bit rows 0.32 (f16), 0.34 (bf16); planes 0.15 (f16); e4m3 rows 0.45, 0.38
    attn_direct1_kernel, plain rows  16-bit rows 0.40 (f16), 0.33 (bf16); planes 0.20, 0.21
    attn_direct1_kernel, tiles       16-bit rows 0.29 (f16), 0.30 (bf16); planes 0.17 (f16)
    attn_stream_kernel               0.21 (f16, the one comparison launch)
Every bit comparison of (c) held.
"""
import pytest
import torch

import attention_cases as ac
from attention_cases import Case, DIRECT, LDS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _i32(x):
    return None if x is None else torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _sentinel_buffer(n, out, dt):
    if out == "fp8":
        byte = torch.tensor([ac.SENTINEL]).to(torch.float8_e4m3fn).view(torch.uint8).item()
        return torch.full((n,), byte, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    return torch.full((n,), ac.SENTINEL, dtype=dt, device=DEV)


def _run(q, k, v, *, dt, Bq, H, Nq, Nk, Tk_cap, NP, tiled=0, out="plain", pad=0, shift=0, kv_group=1, kv_index=None, group_start=None,
         max_group=0, kv_len=None, causal=False, causal_off=0):
    """One launch on packed operands (attention_cases.pack_q / pack_kv) into a sentinel-filled buffer of Bq * Nq + 2 rows whose
    first element lies `shift` elements behind a 16-byte boundary.  Returns the buffer on the CPU, [Bq * Nq + 2, ldo]."""
    from vidil_amd import kernels as K

    ldo = (H * 64 + pad) * (3 if out == "planes" else 1)
    rows = Bq * Nq + 2
    flat = _sentinel_buffer(shift + rows * ldo + 8, out, dt)
    o = flat[shift:shift + rows * ldo].view(rows, ldo)
    K.attention(q.to(DEV), k.to(DEV), v.to(DEV), o, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq + 3, Tk_cap=Tk_cap, NP=NP, kv_group=kv_group,
                causal=causal, causal_off=causal_off, kv_len=_i32(kv_len), kv_index=_i32(kv_index), group_start=_i32(group_start),
                max_group=max_group, ldo=ldo, kv_tiled=tiled, split3=out == "planes")
    torch.cuda.synchronize()
    return o.cpu()


def _launch(c, **over):
    """The launch a case describes.  over: tiled / vt for the same values in another K / V layout."""
    d = ac.inputs(c)
    k, v, cap, NP = d["k"], d["v"], c.Tk_cap, c.NP
    tiled = over.get("tiled", c.tiled)
    if over:
        k, v, cap, NP = ac.pack_kv(d["k_vals"], d["v_vals"], ac.T16[c.dt], over.get("vt", c.vt), tiled, c.tk_extra)
    grouped = d["kv_index"] is None and d["group_start"] is None
    return _run(d["q"], k, v, dt=ac.T16[c.dt], Bq=c.Bq, H=c.H, Nq=c.Nq, Nk=c.Nk, Tk_cap=cap, NP=NP, tiled=tiled, out=c.out, pad=c.pad,
                shift=c.shift, kv_group=c.kv_group if grouped else 1, kv_index=d["kv_index"], group_start=d["group_start"],
                max_group=d["max_group"], kv_len=c.kv_len, causal=c.causal, causal_off=c.causal_off)


def _bits(o):
    return o.view(torch.uint8 if o.dtype == torch.float8_e4m3fn else torch.int16)


def _check(c, o):
    ref, A, written, nokey = ac.reference(c)
    C, rows = c.C, c.Bq * c.Nq
    sent = _bits(_sentinel_buffer(1, c.out, ac.T16[c.dt]).cpu())[0]
    b = _bits(o)
    assert (b[rows:] == sent).all(), "rows behind Bq * Nq were written"
    assert (b[:rows][~written] == sent).all(), "rows of query batches that no unit names were written"
    if c.out == "planes":
        p = o[:rows].view(rows, 3, C + c.pad)
        assert (_bits(p)[:, :, C:] == sent).all(), "columns behind H * 64 of a plane were written"
        hi, lo, third = p[:, 0, :C], p[:, 1, :C], p[:, 2, :C]
        assert torch.equal(_bits(third)[written], _bits(hi)[written]), "plane 2 is not plane 0"
        assert not hi[nokey].any() and not lo[nokey].any()
        got = (hi.double(), hi.double() + lo.double())
    else:
        assert (b[:rows, C:] == sent).all(), "columns behind H * 64 were written"
        got = (o[:rows, :C].double(),)
        assert not got[0][nokey].any()
    worst = 0.0
    for g, bound in zip(got, ac.bounds(c)):
        assert torch.isfinite(g[written]).all()
        worst = max(worst, ((g - ref).abs() / bound)[written].max().item())
    ek = ac.expected_kernel(c)
    print(f"BOUND {c.name}: {ek.kernel}<{ek.dt}, {ek.nkt}, {ek.nw}> rb={ek.rb} {ek.store}: worst |got - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0, (c.name, worst)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("c", ac.CASES, ids=[c.name for c in ac.CASES])
def test_attention_case_vs_float64(c):
    _check(c, _launch(c))


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("c", ac.AIMED, ids=[c.name for c in ac.AIMED])
def test_every_key_is_read(c):
    """Row r of a (unit, head) is aligned with ONE key (score margin >= 25: asserted by the CPU test) whose value row is a pattern
    unique to that key, so the row's output is that pattern: a key that is not read, or read from the wrong place, shows.  Every key
    of the staged kernel's single-chunk forms is a target; over 288 keys and in the direct kernel the tile and chunk edges are."""
    o = _launch(c)
    _check(c, o)
    rows = c.Bq * c.Nq
    assert ((o[:rows].double() - ac.aimed_want(c)).abs() <= ac.bounds(c)[0]).all()


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("c", ac.BITS_LDS, ids=[c.name for c in ac.BITS_LDS])
def test_a_staged_rows_bits_do_not_depend_on_the_launch(c):
    """Units of 2 x 60 rows (kv_len per batch, every other batch spiked) in a batched launch, against: each unit launched alone;
    with its query batches in reversed order; as kv_index batches of 60 rows; named by group_start in a 4-wave launch, in an 8-wave
    launch of two rounds (bound 5: 300 rows) and in an 8-wave launch beside a third, unrelated group of 3 batches (180 rows)."""
    d = ac.inputs(c)
    g, Nq, n_kv = c.kv_group, c.Nq, c.Bq // c.kv_group
    base = _launch(c)
    _check(c, base)
    base = _bits(base)[:c.Bq * Nq].view(c.Bq, Nq, -1)
    kw = dict(dt=ac.T16[c.dt], H=c.H, Nq=Nq, Nk=c.Nk, NP=c.NP, Tk_cap=c.Tk_cap)
    for u in range(n_kv):
        b0 = u * g
        q, k, v, lens = d["q"][b0:b0 + g], d["k"][u:u + 1], d["v"][u:u + 1], c.kv_len[b0:b0 + g]
        alone = _bits(_run(q, k, v, Bq=g, kv_group=g, kv_len=lens, **kw))[:g * Nq].view(g, Nq, -1)
        assert torch.equal(alone, base[b0:b0 + g]), ("alone", u)
        rev = _bits(_run(q.flip(0), k, v, Bq=g, kv_group=g, kv_len=lens[::-1], **kw))[:g * Nq].view(g, Nq, -1)
        assert torch.equal(rev.flip(0), base[b0:b0 + g]), ("reversed", u)
        idx = _bits(_run(q, k, v, Bq=g, kv_index=[0] * g, kv_len=lens, **kw))[:g * Nq].view(g, Nq, -1)
        assert torch.equal(idx, base[b0:b0 + g]), ("kv_index", u)
    starts = [j * g for j in range(n_kv + 1)]
    for max_group in (g, 5):
        o = _bits(_run(d["q"], d["k"], d["v"], Bq=c.Bq, group_start=starts, max_group=max_group, kv_len=c.kv_len, **kw))
        assert torch.equal(o[:c.Bq * Nq].view(c.Bq, Nq, -1), base), ("group_start", max_group)
    # a third group of 3 batches (the first three query batches again, on the K / V of unit 0)
    q7 = torch.cat([d["q"], d["q"][:3]])
    k3, v3 = torch.cat([d["k"], d["k"][:1]]), torch.cat([d["v"], d["v"][:1]])
    o = _bits(_run(q7, k3, v3, Bq=c.Bq + 3, group_start=starts + [c.Bq + 3], max_group=3, kv_len=c.kv_len + c.kv_len[:3], **kw))
    assert torch.equal(o[:c.Bq * Nq].view(c.Bq, Nq, -1), base), "group_start, 8 waves"


TILED = [c for c in ac.CASES if c.tiled and c.Nk > 32 and c.unit == "group" and c.out == "plain"]


@pytest.mark.parametrize("c", TILED, ids=[c.name for c in TILED])
def test_a_direct_rows_bits_do_not_depend_on_the_layout_or_the_launch(c):
    """kv_tiled = 1, kv_tiled = 2 and plain rows + V^T of the same operands; a unit launched alone."""
    d = ac.inputs(c)
    base = _bits(_launch(c))
    assert torch.equal(_bits(_launch(c, tiled=2)), base), "kv_tiled = 2"
    assert torch.equal(_bits(_launch(c, tiled=0, vt=True)), base), "row-major K, V^T"
    g, Nq = c.kv_group, c.Nq
    for u in range(c.Bq // g):
        alone = _run(d["q"][u * g:(u + 1) * g], d["k"][u:u + 1], d["v"][u:u + 1], dt=ac.T16[c.dt], Bq=g, H=c.H, Nq=Nq, Nk=c.Nk,
                     Tk_cap=c.Tk_cap, NP=c.NP, tiled=c.tiled, kv_group=g)
        assert torch.equal(_bits(alone)[:g * Nq], base[u * g * Nq:(u + 1) * g * Nq]), ("alone", u)


def test_the_streamed_kernel_and_the_staged_kernel_give_the_same_bits(monkeypatch):
    """The tower shape on the streamed kernel, on the staged kernel ($VIDIL_ATTN_STREAM=0), and with a kv_len table of full
    lengths — not stream-eligible, so the staged kernel whatever the switch says."""
    c = ac.STREAM_CASE
    outs = []
    for env, lens in (("1", None), ("0", None), ("1", (c.Nk,) * c.Bq)):
        monkeypatch.setenv("VIDIL_ATTN_STREAM", env)
        d = ac.inputs(c)
        o = _run(d["q"], d["k"], d["v"], dt=ac.T16[c.dt], Bq=c.Bq, H=c.H, Nq=c.Nq, Nk=c.Nk, Tk_cap=c.Tk_cap, NP=c.NP, kv_len=lens)
        outs.append(o)
    _check(c, outs[0])
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
