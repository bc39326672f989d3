"""vidil_attention_f32, arith = 2: the split-operand attention with a relative-position bias (csrc/attention.hip, attn_split_kernel
<.., RELB = true>) against float64, against arith = 1, and at the edges of its contract."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _k():
    from vidil_amd import kernels
    return kernels


def _rand(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _join(x3, planes=3):
    D = x3.shape[-1] // 3
    if planes == 3:
        assert torch.equal(x3[..., :D], x3[..., 2 * D:])
    return x3[..., :D].float() + x3[..., D:2 * D].float()


def _table(H, Nq, Nk, seed, slack_lo=5, slack_hi=7):
    """[H, ld] table: N(0, 1) inside the window [rel_off - (Nq - 1), rel_off + Nk - 1], NaN everywhere else."""
    rel_off = Nq - 1 + slack_lo
    ld = rel_off + Nk + slack_hi
    t = torch.full((H, ld), float("nan"))
    t[:, rel_off - (Nq - 1):rel_off + Nk] = _rand(H, Nq + Nk - 1, seed=seed)
    return t, rel_off


def _operands(Bq, H, Nq, Nk, kv_group):
    C = H * 64
    Bk = Bq // kv_group
    if Nq == Nk and kv_group == 1:
        qkv = _rand(Bq * Nq, 3 * C, seed=60).to(DEV)
        return qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    q = _rand(Bq * Nq, C, seed=61).to(DEV)
    kv = _rand(Bk, Nk, 2 * C, seed=62).to(DEV)
    return q, kv[..., :C], kv[..., C:]


def _ref64(q, kk, v, table, rel_off, Bq, H, Nq, Nk, kv_group, causal, kv_len):
    C = H * 64
    Bk = Bq // kv_group
    qd = q.double().cpu().view(Bq, Nq, H, 64).permute(0, 2, 1, 3)
    kd = kk.double().cpu().reshape(Bk, Nk, H, 64).permute(0, 2, 1, 3).repeat_interleave(kv_group, 0)
    vd = v.double().cpu().reshape(Bk, Nk, H, 64).permute(0, 2, 1, 3).repeat_interleave(kv_group, 0)
    keys, rows = torch.arange(Nk), torch.arange(Nq)
    bias = table.double()[:, rel_off + keys[None, :] - rows[:, None]]          # [H, Nq, Nk]
    assert not torch.isnan(bias).any()
    s = (qd @ kd.transpose(-1, -2)) * 0.125 + bias[None]
    if causal:
        s = s.masked_fill(keys[None, :] > rows[:, None], float("-inf"))
    if kv_len is not None:
        s = s.masked_fill(keys[None, None, None, :] >= kv_len.long()[:, None, None, None], float("-inf"))
    return (torch.softmax(s, -1) @ vd).permute(0, 2, 1, 3).reshape(Bq * Nq, C)


@pytest.mark.parametrize("Bq,H,Nq,Nk,kv_group,causal,lens", [
    (3, 2, 33, 33, 1, False, [33, 5, 1]),       # one row and one key past a 32 tile; a batch of one key
    (2, 2, 200, 200, 1, False, None),           # several workgroups per unit
    (2, 12, 384, 384, 1, False, [384, 130]),    # the sentence encoder's bound
    (4, 2, 1, 70, 1, False, None),              # one row per unit: the general kernel, not the one-row form of arith 1
    (4, 2, 3, 70, 2, False, None),              # t restarts in each batch of a shared K / V
    (2, 2, 40, 77, 1, True, None),              # causal
])
def test_relbias_attention_vs_float64(Bq, H, Nq, Nk, kv_group, causal, lens):
    k = _k()
    C = H * 64
    q, kk, v = _operands(Bq, H, Nq, Nk, kv_group)
    table, rel_off = _table(H, Nq, Nk, seed=63)
    kv_len = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    args = dict(Bq=Bq, H=H, Nq=Nq, Nk=Nk, kv_group=kv_group, causal=causal, kv_len=None if kv_len is None else kv_len.to(DEV),
                rel_bias=table.to(DEV), rel_off=rel_off)
    out32 = torch.zeros(Bq * Nq, C, dtype=torch.float32, device=DEV)
    out3 = torch.zeros(Bq * Nq, 3 * C, dtype=torch.float16, device=DEV)
    out2 = torch.zeros(Bq * Nq, 3 * C, dtype=torch.float16, device=DEV)
    k.attention_f32(q, kk, v, out32, **args)
    k.attention_f32(q, kk, v, out3, **args)
    k.attention_f32(q, kk, v, out2, planes=2, **args)
    ref = _ref64(q, kk, v, table, rel_off, Bq, H, Nq, Nk, kv_group, causal, kv_len)
    e32 = (out32.cpu().double() - ref).abs().max().item()
    e3 = (_join(out3.cpu()).double() - ref).abs().max().item()
    print(f"attention_f32 arith=2 {Bq}x{H}x{Nq}x{Nk}: max|d| vs float64 {e32:.2e} (f32 rows) {e3:.2e} ([hi | lo | hi] rows)")
    assert e32 < 3e-6 and e3 < 5e-6, (e32, e3)
    # two planes: hi | lo as in the three-plane rows, the third plane untouched
    assert torch.equal(out2[:, :2 * C], out3[:, :2 * C]) and not out2[:, 2 * C:].any()
    # the bias took part: without it the result is far away
    out1 = torch.zeros_like(out32)
    k.attention_f32(q, kk, v, out1, Bq=Bq, H=H, Nq=Nq, Nk=Nk, kv_group=kv_group, causal=causal, kv_len=args["kv_len"], arith=1)
    if Nk > 1:
        assert (out1.cpu().double() - ref).abs().max().item() > 1e-2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_zero_table_gives_the_bits_of_arith_1(dtype):
    k = _k()
    Bq, H, Nq, Nk = 3, 2, 70, 70
    C = H * 64
    q, kk, v = _operands(Bq, H, Nq, Nk, 1)
    kv_len = torch.tensor([70, 33, 2], dtype=torch.int32, device=DEV)
    zero = torch.zeros(H, Nq + Nk - 1, device=DEV)
    for causal in (False, True):
        a = dict(Bq=Bq, H=H, Nq=Nq, Nk=Nk, kv_len=kv_len, causal=causal)
        o1 = torch.zeros(Bq * Nq, 3 * C, dtype=dtype, device=DEV)
        o2 = torch.zeros_like(o1)
        k.attention_f32(q, kk, v, o1, arith=1, **a)
        k.attention_f32(q, kk, v, o2, rel_bias=zero, rel_off=Nq - 1, **a)
        assert o1.any() and torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    if dtype == torch.float16:
        f1 = torch.zeros(Bq * Nq, C, device=DEV)
        f2 = torch.zeros_like(f1)
        k.attention_f32(q, kk, v, f1, arith=1, Bq=Bq, H=H, Nq=Nq, Nk=Nk, kv_len=kv_len)
        k.attention_f32(q, kk, v, f2, rel_bias=zero, rel_off=Nq - 1, Bq=Bq, H=H, Nq=Nq, Nk=Nk, kv_len=kv_len)
        assert torch.equal(f1.view(torch.int32), f2.view(torch.int32))


def test_a_batch_alone_or_among_others_same_bits():
    k = _k()
    Bq, H, Nq, Nk = 5, 2, 96, 96
    C = H * 64
    q, kk, v = _operands(Bq, H, Nq, Nk, 1)
    table, rel_off = _table(H, Nq, Nk, seed=64)
    table = table.to(DEV)
    kv_len = torch.tensor([96, 40, 77, 3, 96], dtype=torch.int32, device=DEV)
    out = torch.zeros(Bq * Nq, 3 * C, dtype=torch.float16, device=DEV)
    k.attention_f32(q, kk, v, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, kv_len=kv_len, rel_bias=table, rel_off=rel_off)
    for b in (0, 2, 3):
        rows = slice(b * Nq, (b + 1) * Nq)
        alone = torch.zeros(Nq, 3 * C, dtype=torch.float16, device=DEV)
        k.attention_f32(q[rows], kk[rows], v[rows], alone, Bq=1, H=H, Nq=Nq, Nk=Nk, kv_len=kv_len[b:b + 1].clone(), rel_bias=table,
                        rel_off=rel_off)
        assert torch.equal(alone.view(torch.int16), out[rows].view(torch.int16)), b


def test_contract_edges_raise_before_any_launch(monkeypatch):
    from vidil_amd import _lib
    from vidil_amd._lib import VidilHipError
    k = _k()
    Bq, H, Nq, Nk = 2, 2, 8, 12
    C = H * 64
    q, kk, v = _operands(Bq, H, Nq, Nk, 1)
    table = torch.zeros(H, 32, device=DEV)
    pattern = torch.full((Bq * Nq, C), 7.25, device=DEV)
    out = pattern.clone()
    base = dict(Bq=Bq, H=H, Nq=Nq, Nk=Nk)

    def refused(match, **kw):
        with pytest.raises(VidilHipError, match=match):
            k.attention_f32(q, kk, v, out, **base, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out, pattern)

    refused("rel_bias is NULL", arith=2)                                             # no table
    refused("rel_off=6 < Nq - 1", rel_bias=table, rel_off=Nq - 2)                    # a row's window would start before the table
    refused("> rel_bias_ld", rel_bias=table, rel_off=32 - Nk + 1)                    # ... or end behind it
    k.attention_f32(q, kk, v, out.clone(), **base, rel_bias=table, rel_off=32 - Nk)  # (the last admissible offset runs)
    k.attention_f32(q, kk, v, out.clone(), **base, rel_bias=table, rel_off=Nq - 1)   # (and the first)
    # the arena form
    anc = torch.zeros(Bq * Nq, Nk, dtype=torch.int32, device=DEV)
    with pytest.raises(VidilHipError, match="anc must be NULL"):
        k.attention_f32(q, kk, v, out, Bq=Bq * Nq, H=H, Nq=1, Nk=Nk, anc=anc, arena_rows=Bq * Nq, rel_bias=table, rel_off=0)
    assert torch.equal(out, pattern)
    # kv16 and a table that is not 4-byte aligned: no tensor view expresses them, so the struct is edited on its way to the library
    lib = _lib.load()
    real = lib.vidil_attention_f32

    def edited(edit):
        def call(ref, stream):
            edit(ref._obj)
            return real(ref, stream)
        return call

    monkeypatch.setattr(lib, "vidil_attention_f32", edited(lambda a: setattr(a, "kv16", 1)))
    refused("kv16 must be 0", rel_bias=table, rel_off=Nq - 1)
    monkeypatch.setattr(lib, "vidil_attention_f32", edited(lambda a: setattr(a, "rel_bias", a.rel_bias + 2)))
    refused("not 4-byte aligned", rel_bias=table, rel_off=Nq - 1)
    monkeypatch.setattr(lib, "vidil_attention_f32", real)
    # and the third value is named where an unknown one is refused
    refused("2: split-operand \\+ relative-position bias", arith=3)
