"""The two small-unit attention kernels against float64, and every unit against itself launched alone.

`beam_attention` (decode self-attention over the KV arena: one wave serves a group of heads of a beam row and executes
only the 8-key blocks that hold a key) and `attention` on its one-tile path (at most 32 query rows and 32 keys per unit:
four units per workgroup, output rows through LDS).  Every case checks the batched launch against a float64 softmax of
the same 16-bit operands, with the tolerances tests/test_kernels_gpu.py applies to the two entry points, and asserts that
the same units launched one at a time give the same bits: a unit's result must not depend on its neighbours, on the
grouping of heads or on its place in a workgroup.  V holds no exact zero (a skipped key block and an executed one may
differ in the sign of an exact zero only)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
# (rtol, atol).  beam_attention: tests/test_kernels_gpu.py applies 2e-3 / 2e-3 to it, in f16.  Its arithmetic is f32 on exact
# products, so what separates a result from float64 is the rounding of the output: at most half an ulp, which is 2^-11 of the
# value in f16 (11 significant bits) and 2^-8 = 3.9e-3 of it in bf16 (8 significant bits) — so bf16 takes rtol 4e-3, the
# smallest round figure that admits a correctly rounded result, with the same atol.
# attention: the file applies 3e-3 in f16 and 2e-2 in bf16 (the probabilities are rounded to the 16-bit type before P.V).
BEAM_TOL = {"f16": (2e-3, 2e-3), "bf16": (4e-3, 2e-3)}
ATTN_TOL = {"f16": (3e-3, 3e-3), "bf16": (2e-2, 2e-2)}


def _k():
    from vidil_amd import kernels
    return kernels


def _rand(*shape, seed, dtype):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*shape, generator=g).to(dtype)
    return torch.where(x == 0, torch.ones_like(x), x)


def _bits(t):
    return t.view(torch.int16)


def _check_planes(out, ref, C, split3, tol, fill):
    """out [rows, ldo] on the device: plane 0 (and hi + lo, and plane 2 == plane 0) against ref [rows, C]; the columns
    between the planes keep the fill value."""
    o = out.cpu()
    pl = o.shape[1] // 3 if split3 else o.shape[1]
    hi = o[:, :C].double()
    assert torch.isfinite(hi).all()
    assert torch.allclose(hi, ref, rtol=tol[0], atol=tol[1]), (hi - ref).abs().max()
    for p in range(3 if split3 else 1):
        assert (o[:, p * pl + C:(p + 1) * pl].float() == fill).all()
    if split3:
        assert torch.equal(_bits(o[:, 2 * pl:2 * pl + C].contiguous()), _bits(o[:, :C].contiguous()))
        both = hi + o[:, pl:pl + C].double()
        assert torch.allclose(both, ref, rtol=tol[0], atol=tol[1]), (both - ref).abs().max()


# ----------------------------------------------------------------------------------------------- beam_attention
N_KEYS = [1, 7, 8, 9, 16, 17, 31, 32, 33, 64]     # every 8-key block edge and the edges between the kernel instances
TCAP = 70


@pytest.mark.parametrize("split3", [False, True])
@pytest.mark.parametrize("anc_kind", ["repeated", "permutation"])
@pytest.mark.parametrize("H", [5, 12])             # 5: a head group with a tail
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_beam_attention_vs_fp64_and_row_by_row(dt, rows, H, anc_kind, split3):
    k = _k()
    tdt, C, arena_rows = DT[dt], H * 64, rows + 3
    g = torch.Generator().manual_seed(1000 + rows * 16 + H)
    q = _rand(rows, C, seed=201, dtype=tdt)
    ka = _rand(TCAP, arena_rows, C, seed=202, dtype=tdt)
    va = _rand(TCAP, arena_rows, C, seed=203, dtype=tdt)
    if anc_kind == "repeated":      # beams that share ancestors: slots repeat inside a position
        anc = torch.randint(0, arena_rows, (rows, TCAP), generator=g, dtype=torch.int32)
        if rows > 1:
            anc[1] = anc[0]
    else:                           # every position: distinct slots, in an order of its own
        anc = torch.stack([torch.randperm(arena_rows, generator=g)[:rows] for _ in range(TCAP)], 1).to(torch.int32)
    qd, ancd = q.to(DEV), anc.to(DEV)
    ldo = 3 * C if split3 else C
    for n_keys in N_KEYS:
        kn, vn = ka.clone(), va.clone()
        kn[n_keys:] = float("nan")      # positions past n_keys must never be read into a result
        vn[n_keys:] = float("nan")
        t = torch.arange(n_keys)
        kg = kn[t[None, :], anc[:, :n_keys].long()].double().view(rows, n_keys, H, 64)     # [r, t, h, d]
        vg = vn[t[None, :], anc[:, :n_keys].long()].double().view(rows, n_keys, H, 64)
        s = torch.einsum("rhd,rthd->rht", q.double().view(rows, H, 64), kg)
        ref = torch.einsum("rht,rthd->rhd", torch.softmax(s, dim=-1), vg).reshape(rows, C)
        kd, vd = kn.to(DEV), vn.to(DEV)
        out = torch.full((rows, ldo), 7.0, dtype=tdt, device=DEV)
        k.beam_attention(qd, kd, vd, ancd, out, rows=rows, H=H, n_keys=n_keys, split3=split3)
        _check_planes(out, ref, C, split3, BEAM_TOL[dt], 7.0)
        one = torch.full((rows, ldo), 7.0, dtype=tdt, device=DEV)
        for r in range(rows):
            k.beam_attention(qd[r:r + 1], kd, vd, ancd[r:r + 1], one[r:r + 1], rows=1, H=H, n_keys=n_keys, split3=split3)
        assert torch.equal(_bits(out), _bits(one)), n_keys


# ------------------------------------------------------------------------------- attention, one tile per unit
# (form, K/V batches, H, Nq, Nk, use kv_len, causal_off or None, query batches per K/V batch for the table form)
CASES = [
    ("plain", 1, 1, 1, 1, False, None, None),
    ("plain", 3, 12, 18, 18, True, None, None),
    ("plain", 5, 12, 32, 32, False, None, None),            # full units: no row and no key is masked
    ("plain", 9, 12, 18, 18, True, None, None),
    ("plain", 5, 1, 4, 31, True, None, None),
    ("plain", 9, 12, 4, 4, False, 0, None),
    ("plain", 3, 12, 18, 32, True, 3, None),
    ("plain", 5, 12, 32, 31, False, 0, None),
    ("group3", 1, 12, 4, 18, False, None, None),
    ("group3", 5, 12, 4, 31, True, None, None),
    ("group3", 9, 1, 1, 32, False, 3, None),
    ("group3", 3, 12, 4, 4, False, 0, None),
    ("index", 3, 12, 18, 18, True, None, None),
    ("index", 9, 12, 1, 32, False, None, None),
    ("index", 5, 1, 32, 4, False, None, None),
    ("table", 5, 12, 4, 18, True, None, [3, 0, 8, 1, 5]),
    ("table", 9, 12, 1, 31, False, None, [1, 4, 0, 32, 2, 7, 1, 1, 3]),
    ("table", 3, 1, 18, 1, False, None, [1, 1, 1]),
    ("table", 1, 12, 4, 32, False, 3, [8]),
]
# (split3, columns per plane beyond H*64, element offset of the output pointer): the planes form, an output view wider
# than the rows written, and a pointer that is only 2-byte aligned (the kernel's 8-byte stores instead of 16-byte ones)
OUT_FORMS = [(False, 0, 0), (True, 0, 0), (False, 8, 0), (True, 8, 0), (False, 0, 1), (True, 8, 1)]


def _out(rows, C, split3, pad, shift, tdt):
    ldo = (3 if split3 else 1) * (C + pad)
    buf = torch.full((rows * ldo + 8,), 7.0, dtype=tdt, device=DEV)
    return buf[shift:shift + rows * ldo].view(rows, ldo)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:5]) + ("-len" if c[5] else "")
                         + ("" if c[6] is None else f"-causal{c[6]}"))
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_one_tile_attention_vs_fp64_and_unit_by_unit(dt, case):
    form, n_kv, H, Nq, Nk, use_len, causal_off, counts = case
    k = _k()
    tdt, C = DT[dt], H * 64
    g = torch.Generator().manual_seed(77 + n_kv)
    if form == "plain":
        kv_of = torch.arange(n_kv)
    elif form == "group3":
        kv_of = torch.arange(n_kv).repeat_interleave(3)
    elif form == "index":
        kv_of = torch.randint(0, n_kv, (n_kv + 2,), generator=g)
    else:
        kv_of = torch.repeat_interleave(torch.arange(n_kv), torch.tensor(counts))
    Bq = kv_of.numel()
    NP = (Nk + 15) // 16 * 16
    q = (_rand(Bq, H, Nq, 64, seed=211, dtype=torch.float32) * 0.125).to(tdt)
    kk = _rand(n_kv, H, Nk, 64, seed=212, dtype=tdt)
    v = _rand(n_kv, H, Nk, 64, seed=213, dtype=tdt)
    vt = torch.full((n_kv, H, 64, NP), float("nan"), dtype=tdt)           # padding must never leak
    vt[..., k.vt_columns(Nk)] = v.transpose(-1, -2)
    kv_len = None
    if use_len:
        kv_len = torch.tensor([(7 * i) % Nk + 1 for i in range(Bq)], dtype=torch.int32)     # (batch 0: one key)
    # float64 reference from the same 16-bit operands
    s = q.double() @ kk.double()[kv_of].transpose(-1, -2)
    keys = torch.arange(Nk)
    mask = torch.zeros(Bq, 1, Nq, Nk, dtype=torch.bool)
    if kv_len is not None:
        mask |= keys[None, None, None, :] >= kv_len[:, None, None, None]
    if causal_off is not None:
        mask |= keys[None, None, None, :] > (torch.arange(Nq)[None, None, :, None] + causal_off)
    ref = (torch.softmax(s.masked_fill(mask, float("-inf")), -1) @ v.double()[kv_of]).permute(0, 2, 1, 3).reshape(Bq * Nq, C)

    qd, kd, vd = q.to(DEV), kk.to(DEV), vt.to(DEV)
    ld = None if kv_len is None else kv_len.to(DEV)
    shape = dict(H=H, Nq=Nq, Nk=Nk, Tq_cap=Nq, Tk_cap=Nk, NP=NP, causal=causal_off is not None, causal_off=causal_off or 0)
    if form == "index":
        batched = dict(Bq=Bq, kv_index=kv_of.to(torch.int32).to(DEV))
    elif form == "table":
        gs = torch.zeros(n_kv + 1, dtype=torch.int32)
        gs[1:] = torch.cumsum(torch.tensor(counts), 0)
        batched = dict(Bq=Bq, group_start=gs.to(DEV), max_group=max(counts))
    else:
        batched = dict(Bq=Bq, kv_group=3 if form == "group3" else 1)
    # the units: (first query batch, query batches, K/V batch)
    if form == "index":
        units = [(b, 1, int(kv_of[b])) for b in range(Bq)]
    else:
        units = [(int((kv_of < z).sum()), int((kv_of == z).sum()), z) for z in range(n_kv)]

    for split3, pad, shift in OUT_FORMS:
        out = _out(Bq * Nq, C, split3, pad, shift, tdt)
        ldo = out.shape[1]
        k.attention(qd, kd, vd, out, kv_len=ld, ldo=ldo, split3=split3, **shape, **batched)
        _check_planes(out, ref, C, split3, ATTN_TOL[dt], 7.0)
        one = _out(Bq * Nq, C, split3, pad, shift, tdt)
        for b0, nb, z in units:
            if nb == 0:
                continue
            k.attention(qd[b0:b0 + nb], kd[z:z + 1], vd[z:z + 1], one[b0 * Nq:(b0 + nb) * Nq], Bq=nb, kv_group=nb,
                        kv_len=None if ld is None else ld[b0:b0 + nb], ldo=ldo, split3=split3, **shape)
        assert torch.equal(_bits(out.contiguous()), _bits(one.contiguous())), (split3, pad, shift)
