"""The key-split form of vidil_attention (kv_tiled = 2: at most 32 query rows per unit over 768 < Nk <= 16384 keys in fragment
tiles — attn_dsplit_kernel, the decode cross-attention of a caption search over a video) against an fp64 softmax of the same
16-bit operands: every key is read (targets on both sides of every boundary between the waves' slices), the merge of the
slices' partials, masks and the three unit forms, the [hi | lo | hi] output, bit-for-bit independence of a row from the launch
around it, and the contract's edges.  Tolerances are those of tests/test_attention_long_gpu.py: averages over keys do not grow
with Nk.  Fragment tiles are built with kernels.kv_tile_offsets, as tests/test_kernels_gpu.py reads them back."""
import pytest
import torch

import attention_decode_long_cases as A
from common import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}


def _k():
    from vidil_amd import kernels
    return kernels


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _tile_kv(kk, v, Nk, dt, spare_tiles=1):
    """Fragment tiles [Bk, H, Tk_cap * 64] of K / V [Bk, H, Nk, 64] with NaN in every tile position past Nk — the rest of the last
    tile and ``spare_tiles`` whole tiles behind it.  Returns (k tiles, v tiles, Tk_cap) on the device."""
    k = _k()
    Bk, H = kk.shape[:2]
    Tk_cap = (Nk + 31) // 32 * 32 + 32 * spare_tiles
    k_off, v_off = k.kv_tile_offsets(Nk)
    kt = torch.full((Bk, H, Tk_cap * 64), float("nan"), dtype=dt)
    vt = torch.full((Bk, H, Tk_cap * 64), float("nan"), dtype=dt)
    kt[:, :, k_off] = kk.to(dt)
    vt[:, :, v_off] = v.to(dt)
    return kt.to(DEV), vt.to(DEV), Tk_cap


def _ref64(q16, k16, v16, unit_of_batch, kv_len=None):
    """fp64 softmax(q k^T) v of 16-bit operands: q16 [Bq,H,Nq,64], k16 / v16 [Bk,H,Nk,64] -> [Bq*Nq, H*64]; rows whose every key is
    masked are zero (l > 0 ? 1/l : 0)."""
    Bq, H, Nq, _ = q16.shape
    kk = k16.double()[unit_of_batch]
    vv = v16.double()[unit_of_batch]
    s = q16.double() @ kk.transpose(-1, -2)
    if kv_len is not None:
        keys = torch.arange(kk.shape[2])
        s = s.masked_fill(keys[None, None, None, :] >= kv_len.long()[:, None, None, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    return (p @ vv).permute(0, 2, 1, 3).reshape(Bq * Nq, H * 64)


def _attend(q16, kt, vt, Tk_cap, Nk, *, dt, kv_tiled=2, split3=False, **kw):
    k = _k()
    Bq, H, Nq, _ = q16.shape
    out = torch.full((Bq * Nq, (3 if split3 else 1) * H * 64), float("nan"), dtype=dt, device=DEV)
    k.attention(q16.to(DEV), kt, vt, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Tk_cap, NP=0, kv_tiled=kv_tiled, split3=split3, **kw)
    return out


@pytest.mark.parametrize("Nk,H,units,rows,dt", [
    (769, 2, 2, 1, torch.float16), (800, 2, 2, 3, torch.float16), (1025, 2, 2, 4, torch.float16),
    (1576, 2, 2, 32, torch.float16), (1576, 2, 2, 3, torch.bfloat16), (4616, 2, 2, 32, torch.float16),
    (9232, 2, 2, 4, torch.float16), (9232, 2, 2, 3, torch.bfloat16),
    (16384, 1, 1, 32, torch.float16)])                       # the bound itself, once: one unit, one head
def test_every_key_is_read(Nk, H, units, rows, dt):
    """The construction of test_attention_long_gpu.test_every_key_is_read: row r is aligned with ONE key pos[r] (raw score >= 25
    above every other) whose value row is a pattern unique to r, so its output is that pattern.  `rows` rows per unit — one
    (a sampling step), three (a beam step: kv_group = 3), four (the shared prompt pass: Nq = 4) or 32 —, all targets walked
    `rows` at a time per (unit, head)."""
    tg = A.targets(Nk)
    Nq = 4 if rows == 4 else 1
    per_unit = rows // Nq
    Bq = units * per_unit
    kk = _rand(units, H, Nk, 64, seed=41)
    kk[:, :, tg] *= 10.0 / kk[:, :, tg].norm(dim=-1, keepdim=True)     # target keys stand out: own score ~100, every other < 60
    kk = kk.to(dt)
    slots = units * H * rows
    unit_of_batch = torch.arange(Bq) // per_unit
    d = torch.arange(64)
    tol = TOL[dt]
    for r0 in range(0, len(tg), slots):
        part = tg[r0:r0 + slots]
        pos = torch.tensor([part[s % len(part)] for s in range(slots)]).view(units, H, rows)
        v = _rand(units, H, Nk, 64, seed=42).to(dt)
        q = torch.empty(units, H, rows, 64)
        for u in range(units):
            for h in range(H):
                for r in range(rows):
                    key = kk[u, h, pos[u, h, r]].float()
                    q[u, h, r] = key / key.norm() * 10.0
                    v[u, h, pos[u, h, r]] = (((r * 7 + d * 3 + 5 * u + 11 * h) % 61) - 30).to(dt) / 16
        q16 = q.view(units, H, per_unit, Nq, 64).permute(0, 2, 1, 3, 4).reshape(Bq, H, Nq, 64).to(dt).contiguous()
        s = q16.double() @ kk.double()[unit_of_batch].transpose(-1, -2)
        top2 = s.topk(2, dim=-1).values
        assert (top2[..., 0] - top2[..., 1]).min().item() >= 25.0            # the construction holds
        kt, vt, Tk_cap = _tile_kv(kk, v, Nk, dt, spare_tiles=0 if Nk == A.MAX_KEYS else 1)
        got = _attend(q16, kt, vt, Tk_cap, Nk, dt=dt, kv_group=per_unit).double().cpu()
        assert torch.isfinite(got).all()
        ref = _ref64(q16, kk, v, unit_of_batch)
        assert torch.allclose(got, ref, rtol=tol, atol=tol), (Nk, r0, (got - ref).abs().max())
        want = v.double()[torch.arange(units)[:, None, None], torch.arange(H)[None, :, None], pos]    # [units, H, rows, 64]
        want = want.view(units, H, per_unit, Nq, 64).permute(0, 2, 3, 1, 4).reshape(Bq * Nq, H * 64)
        assert torch.allclose(got, want, rtol=tol, atol=tol), (Nk, r0, (got - want).abs().max())


@pytest.mark.parametrize("Bq,Nq,kv_group", [(2, 4, 1), (6, 4, 3), (6, 1, 3)])
@pytest.mark.parametrize("where", ["last_tile", "first_slice", "short_limit"])
def test_merge_across_slices(where, Bq, Nq, kv_group):
    """Nk = 1,576 (slices of 12 / 13 / 12 / 13 tiles).  last_tile: a score spike in the last tile with ramps every 32 keys (every
    partial's maximum differs; the last wave's dominates the merge).  first_slice: the mirror image — the spike at key 5, so
    the later partials are rescaled to almost nothing.  short_limit: kv_len = 100 for every row, inside the first slice: three
    of the four partials are empty (m = -inf, l = 0) and must merge with weight 0, not NaN."""
    H, Nk = 4, 1576
    Bk = Bq // kv_group
    q = _rand(Bq, H, Nq, 64, seed=30) * 0.125
    kk = _rand(Bk, H, Nk, 64, seed=31)
    v = _rand(Bk, H, Nk, 64, seed=32)
    spike = 5 if where != "last_tile" else Nk - 7
    for b in range(Bq):
        for t in range(0, Nq, 3):
            kk[b // kv_group, :, spike] = q[b, :, t] / q[b, :, t].norm(dim=-1, keepdim=True) * (25.0 + 10.0 * (t % 4)) / 0.125 / 8
    kk[:, :, ::32] *= torch.linspace(0.2, 2.5, kk[:, :, ::32].shape[2])[None, None, :, None]
    q16, k16, v16 = q.half(), kk.half(), v.half()
    unit_of_batch = torch.arange(Bq) // kv_group
    kv_len = torch.full((Bq,), 100, dtype=torch.int32) if where == "short_limit" else None
    s = q16.double() @ k16.double()[unit_of_batch].transpose(-1, -2)
    assert s.max().item() > 15.0
    ref = _ref64(q16, k16, v16, unit_of_batch, kv_len)
    kt, vt, Tk_cap = _tile_kv(k16, v16, Nk, torch.float16)
    kw = {} if kv_len is None else dict(kv_len=kv_len.to(DEV))
    got = _attend(q16, kt, vt, Tk_cap, Nk, dt=torch.float16, kv_group=kv_group, **kw).double().cpu()
    assert torch.isfinite(got).all()
    assert torch.allclose(got, ref, rtol=3e-3, atol=3e-3), (where, (got - ref).abs().max())


NK_MASK = 1000                                         # 32 tiles: slices of 8, boundaries at keys 256 / 512 / 768
LEN_POOL = [0, 1, 768, 769, 255, 257, NK_MASK - 1, NK_MASK]


def _lens(Bq):
    return torch.tensor([LEN_POOL[(3 * b + 1) % len(LEN_POOL)] for b in range(Bq)], dtype=torch.int32)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("form", ["kv_group", "kv_index", "group_start"])
def test_masks_and_unit_forms(form, dt):
    """kv_group = 3 (a beam step: 8 units x 3 one-row batches), kv_index (8 batches of 4 rows over 2 units) and group_start with
    counts [0, 1, 3, 32] of one-row batches (an empty unit, one row, three, a full wave); kv_len per query batch from {0, 1, 768,
    769, a slice boundary -+ 1, Nk-1, Nk}: slices masked as a whole for some rows of a unit and for all of them.  kv_len = 0
    rows are exactly zero."""
    Nk, H = NK_MASK, 2
    assert A.slice_keys(Nk) == [256, 512, 768]
    if form == "group_start":
        counts = torch.tensor([0, 1, 3, 32])
        Nq, Bq, Bk = 1, int(counts.sum()), 4
        gs = torch.zeros(5, dtype=torch.int32)
        gs[1:] = counts.cumsum(0)
        unit_of_batch = torch.repeat_interleave(torch.arange(4), counts)
        kw = dict(group_start=gs.to(DEV), max_group=32)
    elif form == "kv_index":
        Nq, Bq, Bk = 4, 8, 2
        unit_of_batch = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0])
        kw = dict(kv_index=unit_of_batch.to(torch.int32).to(DEV))
    else:
        Nq, Bq, Bk = 1, 24, 8
        unit_of_batch = torch.arange(Bq) // 3
        kw = dict(kv_group=3)
    q16 = (_rand(Bq, H, Nq, 64, seed=50) * 0.125).to(dt)
    k16 = _rand(Bk, H, Nk, 64, seed=51).to(dt)
    v16 = _rand(Bk, H, Nk, 64, seed=52).to(dt)
    kv_len = _lens(Bq)
    assert set(kv_len.tolist()) == set(LEN_POOL)
    kt, vt, Tk_cap = _tile_kv(k16, v16, Nk, dt)
    got = _attend(q16, kt, vt, Tk_cap, Nk, dt=dt, kv_len=kv_len.to(DEV), **kw).double().cpu()
    assert torch.isfinite(got).all()
    zero_rows = (kv_len == 0).repeat_interleave(Nq)
    assert zero_rows.any() and (got[zero_rows] == 0).all()
    ref = _ref64(q16, k16, v16, unit_of_batch, kv_len)
    assert torch.allclose(got, ref, rtol=TOL[dt], atol=TOL[dt]), (got - ref).abs().max()


def _join(o3):
    C = o3.shape[1] // 3
    return o3[:, :C].float() + o3[:, C:2 * C].float()


def test_split3_output_carries_the_f32_result():
    """tests/test_parity_mode_gpu.py's relation between the [hi | lo | hi] planes and the plain launch, at 1,576 keys: planes 0 and
    2 are equal, hi is the plain row to one unit in the last place, hi + lo is closer to the exact attention than hi alone."""
    Bq, H, Nq, Nk, kv_group = 6, 4, 1, 1576, 3
    Bk, C = Bq // kv_group, H * 64
    q = (_rand(Bq, H, Nq, 64, seed=30) * 0.125).half()
    kk = _rand(Bk, H, Nk, 64, seed=31).half()
    v = _rand(Bk, H, Nk, 64, seed=32).half()
    kt, vt, Tk_cap = _tile_kv(kk, v, Nk, torch.float16)
    o16 = _attend(q, kt, vt, Tk_cap, Nk, dt=torch.float16, kv_group=kv_group)
    o3 = _attend(q, kt, vt, Tk_cap, Nk, dt=torch.float16, kv_group=kv_group, split3=True)
    assert torch.isfinite(o3).all()
    assert torch.equal(o3[:, :C], o3[:, 2 * C:])
    assert torch.allclose(o3[:, :C].float(), o16.float(), rtol=1.1e-3, atol=1e-7)
    ref = _ref64(q, kk, v, torch.arange(Bq) // kv_group)
    e_hi = (o16.cpu().double() - ref).abs().max().item()
    e_split = (_join(o3.cpu()).double() - ref).abs().max().item()
    assert e_split < 4e-4 and e_split <= e_hi + 5e-5, (e_split, e_hi)
    assert (o3[:, C:2 * C] != 0).any()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_a_rows_bits_do_not_depend_on_the_launch(dt):
    """The same three Q rows with the same key limit on the same unit — alone (group_start, three one-row batches); as rows 5, 17
    and 30 of a 32-row unit among other rows with other limits (kv_group = 32); in a launch of 40 units (kv_index: every row a
    unit of its own, over two K/V batches): identical output bits."""
    Nk, H, L = 1576, 2, 1001
    k16 = _rand(2, H, Nk, 64, seed=61).to(dt)
    v16 = _rand(2, H, Nk, 64, seed=62).to(dt)
    kt, vt, Tk_cap = _tile_kv(k16, v16, Nk, dt)
    probes = (_rand(3, H, 1, 64, seed=60) * 0.3).to(dt)                 # three query rows [3, H, 1, 64]

    def bits(out):
        return out.cpu().view(torch.int16)

    alone = bits(_attend(probes, kt[:1], vt[:1], Tk_cap, Nk, dt=dt, kv_len=torch.full((3,), L, dtype=torch.int32, device=DEV),
                         group_start=torch.tensor([0, 3], dtype=torch.int32, device=DEV), max_group=3))
    # a 32-row unit
    q32 = (_rand(32, H, 1, 64, seed=63) * 0.3).to(dt)
    l32 = torch.tensor([(97 * b) % (Nk + 1) for b in range(32)], dtype=torch.int32)
    at = [5, 17, 30]
    q32[at] = probes
    l32[at] = L
    assert len(set(l32.tolist())) > 20 and 0 in l32.tolist()
    full = bits(_attend(q32, kt[:1], vt[:1], Tk_cap, Nk, dt=dt, kv_len=l32.to(DEV), kv_group=32))
    assert torch.equal(full[at], alone)
    # 40 units
    q40 = (_rand(40, H, 1, 64, seed=64) * 0.3).to(dt)
    l40 = torch.tensor([(131 * b) % (Nk + 1) for b in range(40)], dtype=torch.int32)
    idx = torch.tensor([(b * 7) % 2 for b in range(40)], dtype=torch.int32)
    at = [5, 18, 31]
    q40[at] = probes
    l40[at] = L
    idx[at] = 0
    many = bits(_attend(q40, kt, vt, Tk_cap, Nk, dt=dt, kv_len=l40.to(DEV), kv_index=idx.to(DEV)))
    assert torch.equal(many[at], alone)
    # (and the value is right)
    ref = _ref64(probes, k16[:1], v16[:1], torch.zeros(3, dtype=torch.long), torch.full((3,), L))
    assert torch.allclose(alone.view(dt).double(), ref, rtol=TOL[dt], atol=TOL[dt])


def test_contract_edges():
    k = _k()
    H = 2
    # up to 768 keys kv_tiled = 2 is kv_tiled = 1: the same kernels, the same bits
    for Nk, Bq, Nq, kv_group in [(768, 6, 1, 3), (577, 6, 1, 3), (768, 2, 4, 1), (20, 4, 1, 1)]:
        q = (_rand(Bq, H, Nq, 64, seed=70) * 0.125).half()
        kk, v = _rand(Bq // kv_group, H, Nk, 64, seed=71).half(), _rand(Bq // kv_group, H, Nk, 64, seed=72).half()
        kt, vt, Tk_cap = _tile_kv(kk, v, Nk, torch.float16)
        one = _attend(q, kt, vt, Tk_cap, Nk, dt=torch.float16, kv_tiled=True, kv_group=kv_group)
        two = _attend(q, kt, vt, Tk_cap, Nk, dt=torch.float16, kv_tiled=2, kv_group=kv_group)
        assert torch.isfinite(one).all() and torch.equal(one.view(torch.int16), two.view(torch.int16)), Nk

    def launch(Nk, Bq, Nq, dt=torch.float16, out_dt=None, **kw):
        q = torch.zeros(Bq, H, Nq, 64, dtype=dt, device=DEV)
        Tc = (Nk + 31) // 32 * 32
        kv = torch.zeros(1, H, Tc, 64, dtype=dt, device=DEV)
        out = torch.zeros(Bq * Nq, H * 64, dtype=out_dt or dt, device=DEV)
        kw.setdefault("kv_tiled", 2)
        k.attention(q, kv, kv, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Tc, NP=0, kv_group=Bq, **kw)
        return out

    with pytest.raises(k.VidilHipError, match="at most 32 query rows"):
        launch(800, 33, 1)
    with pytest.raises(k.VidilHipError, match="at most 32 query rows"):
        launch(800, 3, 11)
    with pytest.raises(k.VidilHipError, match="not supported"):          # past the bound
        launch(16385, 3, 1)
    with pytest.raises(k.VidilHipError, match="not supported"):          # causal masks stay with the short kernels
        launch(800, 1, 4, causal=True)
    with pytest.raises(k.VidilHipError, match="not supported"):          # kv_tiled = 1 keeps refusing more than 768 keys
        launch(800, 3, 1, kv_tiled=True)
    with pytest.raises(k.VidilHipError, match="fp8"):                    # e4m3 rows need more than 32 query rows per unit
        launch(800, 3, 1, out_dt=torch.float8_e4m3fn)
    with pytest.raises(k.VidilHipError, match="multiple of 32"):
        q = torch.zeros(3, H, 1, 64, dtype=torch.float16, device=DEV)
        kv = torch.zeros(1, H, 832, 64, dtype=torch.float16, device=DEV)
        k.attention(q, kv, kv, torch.zeros(3, H * 64, dtype=torch.float16, device=DEV), Bq=3, H=H, Nq=1, Nk=800, Tq_cap=1, Tk_cap=801,
                    NP=0, kv_group=3, kv_tiled=2)
    with pytest.raises(k.VidilHipError, match="kv_tiled"):
        from vidil_amd import _lib
        q = torch.zeros(3, H, 1, 64, dtype=torch.float16, device=DEV)
        kv = torch.zeros(1, H, 832, 64, dtype=torch.float16, device=DEV)
        out = torch.zeros(3, H * 64, dtype=torch.float16, device=DEV)
        k.check(_lib.load().vidil_attention(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), out.data_ptr(), None, None, None, 0, 0, 3, H, 1,
                                            800, 1, 832, 0, 3, 0, 0, H * 64, 3, _lib.DT_F16, _lib.DT_F16, None), "attention")
    assert (launch(16384, 32, 1) == 0).all() and (launch(769, 1, 1, dt=torch.bfloat16) == 0).all()     # both ends are served
    torch.cuda.synchronize()


def test_tiled_heads_epilogue_at_16384_keys():
    """project_cross_kv(tiled=True)'s GEMM epilogue at the bound: T = Tk_cap = 16,384 keys of one sequence — every slot of the
    fragment tiles written once, with the bits of the row-major epilogue of the same GEMM — and a decode step over all of them."""
    k = _k()
    H, T = 2, 16384
    C = H * 64
    a = (_rand(T, C, seed=93) * 1.0).half().to(DEV)
    w = (_rand(2 * C, C, seed=94) * 0.05).half().to(DEV)
    bias = _rand(2 * C, seed=95).to(DEV)
    kt = torch.full((1, H, T * 64), float("nan"), dtype=torch.float16, device=DEV)
    vt = torch.full((1, H, T * 64), float("nan"), dtype=torch.float16, device=DEV)
    k.gemm(a, w, bias, heads=dict(k=kt, vt=vt, T=T, H=H, part0=1, t_off=0, Tk_cap=T, tiled=True))
    k_rm = torch.empty(1, H, T, 64, dtype=torch.float16, device=DEV)
    v_rm = torch.empty(1, H, T, 64, dtype=torch.float16, device=DEV)
    k.gemm(a, w, bias, heads=dict(k=k_rm, vt=v_rm, T=T, H=H, part0=1, t_off=0, Tk_cap=T, NP=0))
    k_off, v_off = (o.to(DEV) for o in k.kv_tile_offsets(T))
    assert torch.isfinite(kt).all() and torch.isfinite(vt).all()
    assert torch.equal(kt[:, :, k_off], k_rm) and torch.equal(vt[:, :, v_off], v_rm)
    # the tiles serve a decode step over all 16,384 keys
    q = (_rand(3, H, 1, 64, seed=96) * 0.125).half()
    got = _attend(q, kt, vt, T, T, dt=torch.float16, kv_group=3).double().cpu()
    ref = _ref64(q, k_rm.cpu(), v_rm.cpu(), torch.zeros(3, dtype=torch.long))
    assert torch.allclose(got, ref, rtol=3e-3, atol=3e-3), (got - ref).abs().max()
