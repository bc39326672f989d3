"""The long-key form of vidil_attention (768 < Nk <= 16384, more than 32 query rows per unit: attn_long_kernel) against an
fp64 softmax of the same 16-bit operands: every key is read (targets at every chunk boundary), the online softmax across
chunks, masks and the three unit forms, bit-for-bit independence of a row from the launch around it, and the contract's edges.
Tolerances are those of the short kernels (tests/test_kernels_gpu.py): averages over keys do not grow with Nk."""
import ctypes
import os

import pytest
import torch

from common import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu
DEV = "cuda"

CH = 128                      # attn_long_kernel's chunk (LONG_NKEY in csrc/attention.hip): two LDS buffers of 128 keys
TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}


def _k():
    from vidil_amd import kernels
    return kernels


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _pad_kv(kk, v, Nk, vt_form, dt, pad=5):
    """K [Bk,H,Nk+pad,64] and V (row-major, or V^T [Bk,H,64,NP] in vt_columns order) with NaN in everything past Nk."""
    k = _k()
    Bk, H = kk.shape[:2]
    Tk_cap = Nk + pad
    kp = torch.full((Bk, H, Tk_cap, 64), float("nan"), dtype=dt)
    kp[:, :, :Nk] = kk
    if vt_form:
        NP = (Nk + 15) // 16 * 16 + 16
        vp = torch.full((Bk, H, 64, NP), float("nan"), dtype=dt)
        vp[..., k.vt_columns(Nk)] = v.transpose(-1, -2)
    else:
        NP = 0
        vp = torch.full((Bk, H, Tk_cap, 64), float("nan"), dtype=dt)
        vp[:, :, :Nk] = v
    return kp.to(DEV), vp.to(DEV), Tk_cap, NP


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


def _targets(Nk):
    """Keys a row is aimed at: both ends, 767 / 768 (where the short kernels end), the last partial 16-key block and both sides
    of EVERY boundary between the kernel's 128-key chunks."""
    t = {0, Nk - 1, (Nk - 1) // 16 * 16, max(0, Nk - 2)}
    t |= {x for x in (767, 768) if x < Nk}
    for c in range(1, (Nk + CH - 1) // CH):
        t |= {x for x in (c * CH - 1, c * CH, c * CH + 1) if x < Nk}
    return sorted(t)


def test_targets_are_the_chunk_boundaries_of_128_key_chunks():
    # CH = 128: the boundaries of Nk = 800 spelled out
    assert _targets(800) == [0, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 639, 640, 641, 767, 768, 769, 784,
                             798, 799]
    assert _targets(257) == [0, 127, 128, 129, 255, 256]                 # 2 * CH + 1


@pytest.mark.parametrize("vt_form", [False, True], ids=["vrow", "vt"])
@pytest.mark.parametrize("Nk,H,units,rows,dt", [
    (769, 2, 2, 48, torch.float16), (800, 2, 2, 48, torch.float16), (1025, 2, 2, 48, torch.float16),
    (1576, 2, 2, 48, torch.float16), (1576, 2, 2, 48, torch.bfloat16),
    (2 * CH + 1, 2, 2, 48, torch.float16),          # 257 keys: at CH = 128 this one is served by the short staged kernel
    (4616, 1, 1, 40, torch.float16), (9232, 1, 1, 40, torch.float16)])
def test_every_key_is_read(Nk, H, units, rows, dt, vt_form):
    """Row r is aligned with ONE key pos[r] (raw score >= 25 above every other) whose value row is a pattern unique to r, so
    its output is that pattern: a key that is not read, or read from the wrong place, shows.  Grouped form, `rows` query rows
    per unit (6 or 5 batches of 8); all targets are walked, `rows` at a time per (unit, head)."""
    k = _k()
    Nq = 8
    per_unit = rows // Nq
    Bq = units * per_unit
    tg = _targets(Nk)
    kk = _rand(units, H, Nk, 64, seed=41)
    kk[:, :, tg] *= 10.0 / kk[:, :, tg].norm(dim=-1, keepdim=True)     # target keys stand out: own score ~100, every other < 60
    kk = kk.to(dt)
    slots = units * H * rows
    gs = torch.arange(units + 1, dtype=torch.int32) * per_unit
    unit_of_batch = torch.arange(Bq) // per_unit
    for r0 in range(0, len(tg), slots):
        part = tg[r0:r0 + slots]
        # slot s = (unit, head, row) -> target part[s % len(part)] (every slot has one; every target at least one slot)
        pos = torch.tensor([part[s % len(part)] for s in range(slots)]).view(units, H, rows)
        v = _rand(units, H, Nk, 64, seed=42).to(dt)
        q = torch.empty(units, H, rows, 64)
        d = torch.arange(64)
        for u in range(units):
            for h in range(H):
                for r in range(rows):
                    key = kk[u, h, pos[u, h, r]].float()
                    q[u, h, r] = key / key.norm() * 10.0
                    v[u, h, pos[u, h, r]] = (((r * 7 + d * 3 + 5 * u + 11 * h) % 61) - 30).to(dt) / 16
        # [units, H, rows, 64] -> query batches [Bq, H, Nq, 64]
        q16 = q.view(units, H, per_unit, Nq, 64).permute(0, 2, 1, 3, 4).reshape(Bq, H, Nq, 64).to(dt).contiguous()
        s = q16.double() @ kk.double()[unit_of_batch].transpose(-1, -2)
        top2 = s.topk(2, dim=-1).values
        assert (top2[..., 0] - top2[..., 1]).min().item() >= 25.0            # the construction holds
        kp, vp, Tk_cap, NP = _pad_kv(kk, v, Nk, vt_form, dt)
        out = torch.full((Bq * Nq, H * 64), float("nan"), dtype=dt, device=DEV)
        k.attention(q16.to(DEV), kp, vp, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Tk_cap, NP=NP,
                    group_start=gs.to(DEV), max_group=per_unit)
        got = out.double().cpu()
        assert torch.isfinite(got).all()
        ref = _ref64(q16, kk, v, unit_of_batch)
        tol = TOL[dt]
        assert torch.allclose(got, ref, rtol=tol, atol=tol), (Nk, r0, (got - ref).abs().max())
        # ... and the output IS the target's pattern (the reference is not fooled either)
        want = v.double()[torch.arange(units)[:, None, None], torch.arange(H)[None, :, None], pos]    # [units, H, rows, 64]
        want = want.view(units, H, per_unit, Nq, 64).permute(0, 2, 3, 1, 4).reshape(Bq * Nq, H * 64)
        assert torch.allclose(got, want, rtol=tol, atol=tol), (Nk, r0, (got - want).abs().max())


@pytest.mark.parametrize("Bq,H,Nq,Nk,kv_group", [(2, 4, 35, 1576, 1), (6, 4, 35, 1576, 3)])
def test_online_softmax_across_chunks_on_spiked_scores(Bq, H, Nq, Nk, kv_group):
    """The construction of test_attention_online_softmax_on_spiked_scores at 13 chunks: a spike in the last tile, ramps every 32
    keys (the reference value moves late and often, across chunk boundaries) — 35 rows (4-wave form) and 105 rows per unit."""
    k = _k()
    Bk = Bq // kv_group
    q = _rand(Bq, H, Nq, 64, seed=30) * 0.125
    kk = _rand(Bk, H, Nk, 64, seed=31)
    v = _rand(Bk, H, Nk, 64, seed=32)
    for b in range(Bq):
        for t in range(0, Nq, 3):
            kk[b // kv_group, :, Nk - 7] = q[b, :, t] / q[b, :, t].norm(dim=-1, keepdim=True) * (25.0 + 10.0 * (t % 4)) / 0.125 / 8
    kk[:, :, ::32] *= torch.linspace(0.2, 2.5, kk[:, :, ::32].shape[2])[None, None, :, None]
    q16, k16, v16 = q.half(), kk.half(), v.half()
    unit_of_batch = torch.arange(Bq) // kv_group
    s = q16.double() @ k16.double()[unit_of_batch].transpose(-1, -2)
    assert s.max().item() > 15.0
    ref = _ref64(q16, k16, v16, unit_of_batch)
    for vt_form in (False, True):
        kp, vp, Tk_cap, NP = _pad_kv(k16, v16, Nk, vt_form, torch.float16)
        out = torch.full((Bq * Nq, H * 64), float("nan"), dtype=torch.float16, device=DEV)
        k.attention(q16.to(DEV), kp, vp, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Tk_cap, NP=NP, kv_group=kv_group)
        got = out.double().cpu()
        assert torch.isfinite(got).all()
        assert torch.allclose(got, ref, rtol=3e-3, atol=3e-3), (vt_form, (got - ref).abs().max())


def _lens(Bq, Nk):
    pool = [0, 1, 768, 769, CH, CH + 1, Nk - 1, Nk]
    return torch.tensor([pool[(3 * b + 1) % len(pool)] for b in range(Bq)], dtype=torch.int32)


@pytest.mark.parametrize("vt_form", [False, True], ids=["vrow", "vt"])
@pytest.mark.parametrize("form", ["group_start", "kv_index", "kv_group"])
def test_masks_and_unit_forms(form, vt_form):
    """group_start with counts [0, 1, 40, 3] x 8 rows (an empty unit, 8 rows inside a launch bounded by 40 x 8, 320 rows over two
    row blocks), kv_index and kv_group = 2 with 35 rows per batch; kv_len per query batch from {0, 1, 768, 769, CH, CH+1, Nk-1,
    Nk}: chunks that are masked as a whole, for some rows of a wave and for all of them.  kv_len = 0 rows are zeros."""
    k = _k()
    Nk, H = 1000, 2
    kw = {}
    if form == "group_start":
        counts = torch.tensor([0, 1, 40, 3])
        Nq, Bq, Bk = 8, int(counts.sum()), 4
        gs = torch.zeros(5, dtype=torch.int32)
        gs[1:] = counts.cumsum(0)
        unit_of_batch = torch.repeat_interleave(torch.arange(4), counts)
        kw = dict(group_start=gs.to(DEV), max_group=40)
    elif form == "kv_index":
        Nq, Bq, Bk = 35, 8, 2
        unit_of_batch = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0])
        kw = dict(kv_index=unit_of_batch.to(torch.int32).to(DEV))
    else:
        Nq, Bq, Bk = 35, 8, 4
        unit_of_batch = torch.arange(Bq) // 2
        kw = dict(kv_group=2)
    q16 = (_rand(Bq, H, Nq, 64, seed=50) * 0.125).half()
    k16 = _rand(Bk, H, Nk, 64, seed=51).half()
    v16 = _rand(Bk, H, Nk, 64, seed=52).half()
    kv_len = _lens(Bq, Nk)
    assert set(kv_len.tolist()) == {0, 1, 768, 769, CH, CH + 1, Nk - 1, Nk}
    kp, vp, Tk_cap, NP = _pad_kv(k16, v16, Nk, vt_form, torch.float16)
    out = torch.full((Bq * Nq, H * 64), float("nan"), dtype=torch.float16, device=DEV)
    k.attention(q16.to(DEV), kp, vp, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Tk_cap, NP=NP, kv_len=kv_len.to(DEV), **kw)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    zero_rows = (kv_len == 0).repeat_interleave(Nq)
    assert zero_rows.any() and (got[zero_rows] == 0).all()
    ref = _ref64(q16, k16, v16, unit_of_batch, kv_len)
    assert torch.allclose(got, ref, rtol=3e-3, atol=3e-3), (got - ref).abs().max()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("vt_form", [False, True], ids=["vrow", "vt"])
def test_a_rows_bits_do_not_depend_on_the_launch(vt_form, dt):
    """The same three Q rows against the same unit with the same key limit — alone (one row, the bound rounded up to 33),
    inside a group of 40 x 1 rows (4-wave form), inside 9 x 35 rows (8-wave form, second row block): identical output bits."""
    k = _k()
    Nk, H, L = 1576, 2, 1001                          # L: the rows' key limit (masks the tail: chunks 8.. are never needed)
    k16 = _rand(1, H, Nk, 64, seed=61).to(dt)
    v16 = _rand(1, H, Nk, 64, seed=62).to(dt)
    kp, vp, Tk_cap, NP = _pad_kv(k16, v16, Nk, vt_form, dt)
    probes = (_rand(3, H, 64, seed=60) * 0.3).to(dt)               # three query rows [3, H, 64]

    def run(q16, Bq, Nq, lens, max_group):
        out = torch.full((Bq * Nq, H * 64), float("nan"), dtype=dt, device=DEV)
        k.attention(q16.to(DEV), kp, vp, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Tk_cap, NP=NP, kv_len=lens.to(DEV),
                    group_start=torch.tensor([0, Bq], dtype=torch.int32, device=DEV), max_group=max_group)
        return out.cpu().view(torch.int16)

    for i in range(3):
        alone = run(probes[i].view(1, H, 1, 64), 1, 1, torch.tensor([L], dtype=torch.int32), 33)[0]
        # 40 batches of one row, the probe at batch 5 + 13 * i; the others are other rows with other limits
        q40 = (_rand(40, H, 1, 64, seed=63) * 0.3).to(dt)
        l40 = torch.tensor([(97 * b) % (Nk + 1) for b in range(40)], dtype=torch.int32)
        b = 5 + 13 * i
        q40[b, :, 0] = probes[i]
        l40[b] = L
        assert torch.equal(run(q40, 40, 1, l40, 40)[b], alone)
        # 9 batches of 35 rows (315 rows: 8 waves), the probe in batch 2 + 3 * i at token 4 + 10 * i (rows 74 / 189 / 304)
        q9 = (_rand(9, H, 35, 64, seed=64) * 0.3).to(dt)
        l9 = torch.tensor([Nk, 0, 300, Nk - 1, 769, 100, CH, Nk, 1200], dtype=torch.int32)
        b, t = 2 + 3 * i, 4 + 10 * i
        q9[b, :, t] = probes[i]
        l9[b] = L
        assert torch.equal(run(q9, 9, 35, l9, 9)[b * 35 + t], alone)
    # (and the value is right)
    ref = _ref64(probes[0].view(1, H, 1, 64), k16, v16, torch.zeros(1, dtype=torch.long), torch.tensor([L]))
    got = run(probes[0].view(1, H, 1, 64), 1, 1, torch.tensor([L], dtype=torch.int32), 33).view(dt).double()
    assert torch.allclose(got, ref, rtol=TOL[dt], atol=TOL[dt])


def test_contract_edges():
    k = _k()
    H = 2

    def launch(Nk, Bq, Nq, **kw):
        q = torch.zeros(Bq, H, Nq, 64, dtype=torch.float16, device=DEV)
        kv = torch.zeros(Bq, H, (Nk + 31) // 32 * 32, 64, dtype=torch.float16, device=DEV)
        out = torch.zeros(Bq * Nq, H * 64, dtype=torch.float16, device=DEV)
        k.attention(q, kv, kv, out, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=kv.shape[2], NP=0, **kw)
        return out

    with pytest.raises(k.VidilHipError, match="not supported"):          # 32 rows per unit: no kernel over 768 keys
        q = torch.zeros(1, H, 32, 64, dtype=torch.float16, device=DEV)
        vt = torch.zeros(1, H, 64, 784, dtype=torch.float16, device=DEV)
        kk = torch.zeros(1, H, 769, 64, dtype=torch.float16, device=DEV)
        k.attention(q, kk, vt, torch.zeros(32, H * 64, dtype=torch.float16, device=DEV), Bq=1, H=H, Nq=32, Nk=769, Tq_cap=32,
                    Tk_cap=769, NP=784)
    with pytest.raises(k.VidilHipError):                                 # fragment-tiled K / V
        launch(800, 1, 40, kv_tiled=True)
    with pytest.raises(k.VidilHipError):
        launch(800, 1, 4, kv_tiled=True)
    with pytest.raises(k.VidilHipError, match="not supported"):          # past the builder's bound (16384)
        launch(16385, 1, 40)
    with pytest.raises(k.VidilHipError, match="not supported"):          # causal masks stay with the short kernels
        launch(800, 1, 40, causal=True)
    launch(16384, 1, 40)                                                 # the bound itself is served
    torch.cuda.synchronize()


def test_nk_768_bits_equal_a_parent_build():
    """Launches with Nk <= 768 dispatch exactly as before: the same launches through a library built from the parent commit
    ($VIDIL_HIP_LIB_PARENT: its libvidil_hip.so, same ABI) give the same bits."""
    path = os.environ.get("VIDIL_HIP_LIB_PARENT")
    if not path or not os.path.exists(path):
        pytest.skip("no parent build to compare with: set VIDIL_HIP_LIB_PARENT to a libvidil_hip.so built from the parent commit")
    from vidil_amd import _lib
    k = _k()
    parent = ctypes.CDLL(path)
    res, args = _lib.SIGNATURES["vidil_attention"]
    parent.vidil_attention.restype, parent.vidil_attention.argtypes = res, args
    assert parent.vidil_abi_version() == _lib.ABI_VERSION
    for Bq, Nq, Nk, kv_group, NP in [(2, 40, 768, 1, 0), (2, 40, 768, 1, 768), (6, 35, 577, 3, 0), (4, 300, 768, 1, 0),
                                     (2, 4, 768, 1, 768)]:
        H = 2
        Bk = Bq // kv_group
        q = (_rand(Bq, H, Nq, 64, seed=70) * 0.125).half().to(DEV)
        kk = _rand(Bk, H, Nk, 64, seed=71).half().to(DEV)
        v = _rand(Bk, H, Nk, 64, seed=72).half()
        if NP:
            vt = torch.zeros(Bk, H, 64, NP, dtype=torch.float16)
            vt[..., k.vt_columns(Nk)] = v.transpose(-1, -2)
            v = vt
        v = v.to(DEV)
        a = torch.zeros(Bq * Nq, H * 64, dtype=torch.float16, device=DEV)
        b = torch.zeros_like(a)
        k.attention(q, kk, v, a, Bq=Bq, H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Nk, NP=NP, kv_group=kv_group)
        torch.cuda.synchronize()
        rc = parent.vidil_attention(q.data_ptr(), kk.data_ptr(), v.data_ptr(), b.data_ptr(), None, None, None, 0, 0, Bq, H, Nq, Nk,
                                    Nq, Nk, NP, kv_group, 0, 0, H * 64, 0, _lib.DT_F16, _lib.DT_F16, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (Bq, Nq, Nk, kv_group, NP)
