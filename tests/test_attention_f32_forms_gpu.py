"""vidil_attention_f32 on every kernel it dispatches to, in every unit form and at the key / row / mask edges, against fp64
(tests/attention_f32_cases.py has the case table, the reference and the tolerances with their derivations; its preconditions
are asserted by tests/test_attention_f32_cases_cpu.py).

Every output buffer starts as a sentinel: after the launch everything outside the written region still holds it — the columns
behind H * 64 of a wide row or plane, the third plane with planes = 2, the rows of query batches that no group names — and a
row without an admissible key is exactly zero in hi and in lo."""
from dataclasses import replace

import pytest
import torch

import attention_f32_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"
BY_NAME = {c.name: c for c in ac.CASES}


def _i32(x):
    return None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)


def _launch(c, kv_index=None, group_start=None, max_group=0):
    """One launch of a case into a sentinel-filled buffer [Bq * Nq, ldo].  kv_index / group_start: another description of the
    case's kv_group mapping (the equal-bits test)."""
    from vidil_amd import kernels as K

    d = ac.inputs(c)
    C = c.C
    q = d["qw"].to(DEV)[:, C:2 * C]
    kw = dict(Bq=c.Bq, H=c.H, Nq=c.Nq, Nk=c.Nk, planes=c.planes)
    if c.form == "arena":
        kk, v = d["k"].to(DEV), d["v"].to(DEV)
        kw.update(anc=d["anc"].to(DEV), arena_rows=d["arena_rows"])
    else:
        if c.form == "kv16":
            kk, v = d["k"].to(DEV), d["v"].to(DEV)
            kw.update(kv16=True)
        else:
            kvw = d["kvw"].to(DEV)
            kk, v = kvw[:, :C], kvw[:, C:]
        if kv_index is None and group_start is None:
            kv_index, group_start, max_group = d["kv_index"], d["group_start"], d["max_group"]
        grouped = kv_index is None and group_start is None
        kw.update(kv_rows=c.kv_rows, kv_group=c.kv_group if grouped else 1, kv_index=_i32(kv_index), group_start=_i32(group_start),
                  max_group=max_group, causal=c.causal, causal_off=c.causal_off, kv_len=_i32(c.kv_len), arith=c.arith)
        if c.arith == 2:
            kw.update(rel_bias=d["rel_bias"].to(DEV), rel_off=d["rel_off"])
    out = torch.full((c.Bq * c.Nq, c.ldo), ac.SENTINEL, dtype=torch.float32 if c.out == "f32" else ac.T16[c.out], device=DEV)
    K.attention_f32(q, kk, v, out, **kw)
    return out


def _check(c, out):
    ref, written, nokey = ac.reference(c)
    o = out.cpu()
    C, rows = c.C, c.Bq * c.Nq
    assert (o[~written] == ac.SENTINEL).all(), "rows of query batches that no unit names were written"
    if c.out == "f32":
        val = o[:, :C].double()
        assert (o[:, C:] == ac.SENTINEL).all(), "columns behind H * 64 were written"
        assert not o[nokey][:, :C].any()
    else:
        p = o.view(rows, 3, C + c.pad)
        assert (p[:, :, C:] == ac.SENTINEL).all(), "columns behind H * 64 of a plane were written"
        hi, lo, third = p[:, 0, :C], p[:, 1, :C], p[:, 2, :C]
        if c.planes == 2:
            assert (third == ac.SENTINEL).all(), "planes = 2 wrote the third plane"
        else:
            assert torch.equal(third[written].view(torch.int16), hi[written].view(torch.int16))
        assert not hi[nokey].any() and not lo[nokey].any()
        val = hi.double() + lo.double()
    assert torch.isfinite(val[written]).all()
    err = (val - ref).abs()
    tol = ac.tolerance(c, ref)
    worst = (err / tol)[written].max().item()
    print(f"{c.name}: {ac.expected_kernel(c)}: max|d| vs fp64 {err[written].max().item():.2e}, "
          f"{worst:.2f} of the bound ({'measured' if c.measured else 'fixed'}: {tol if isinstance(tol, float) else '3e-6 + 2^-17 |ref|'})")
    assert worst <= 1.0, (c.name, err[written].max().item())


@pytest.mark.parametrize("c", ac.CASES, ids=[c.name for c in ac.CASES])
def test_attention_f32_case_vs_float64(c):
    _check(c, _launch(c))


@pytest.mark.parametrize("out", ["f16", "bf16"])
@pytest.mark.parametrize("fam", ["mfma", "split", "relb"])
def test_kv_group_kv_index_and_group_start_describe_one_mapping_with_the_same_bits(fam, out):
    """In the f32-MFMA and split-operand kernels a lane's arithmetic involves its own row only, and the ballot-driven rescale of
    the split kernel multiplies the rows that keep their reference by exactly 2^0 — every other query batch of these cases has
    no spike, so such rows sit beside rows that move theirs.  Nq = 12 keeps kv_index (12 rows per unit) on the kernel that
    kv_group and group_start (24 rows per unit) run."""
    c = BY_NAME[f"{fam}_mixed_spikes_{out}"]
    g, n_kv = c.kv_group, c.Bq // c.kv_group
    assert ac.expected_kernel(c) == ac.expected_kernel(replace(c, unit="index")) and c.Nq > 8 and g == 2       # (start: 2 Nq rows)
    grouped = _launch(c)
    _check(c, grouped)
    indexed = _launch(c, kv_index=[b // g for b in range(c.Bq)])
    started = _launch(c, group_start=[j * g for j in range(n_kv + 1)], max_group=g)
    assert torch.equal(grouped.view(torch.int16), indexed.view(torch.int16))
    assert torch.equal(grouped.view(torch.int16), started.view(torch.int16))
