"""vidil_gemm on every kernel body it dispatches to, with every epilogue each serves, at the tile, ring, grid and scatter edges,
against the exact integer product (tests/gemm_cases.py has the case table, the inputs and the reference; its preconditions are
asserted by tests/test_gemm_cases_cpu.py).

Per case: the name vidil_gemm_kernel_name reports is the one the table expects (a table that no longer reaches its kernel is
a hole, so a mismatch fails); one launch; every written element equals the reference BIT FOR BIT (activation cases: within the
bound of gemm_cases.act_bound); every other element of every destination allocation — capacity rows and columns, other
sequences' token rows, unused arena slots, the guards on both sides — still holds the NaN sentinel it was filled with."""
import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _alloc(shape, kind, dt):
    """(flat integer allocation filled with the sentinel, the destination view inside it behind GUARD elements)."""
    n = int(np.prod(shape))
    if kind == "f32":
        flat = torch.full((n + 2 * gc.GUARD,), gc.SENTINEL32, dtype=torch.int32, device=DEV)
        view = flat[gc.GUARD:gc.GUARD + n].view(torch.float32)
    else:
        flat = torch.full((n + 2 * gc.GUARD,), gc.SENTINEL16, dtype=torch.int16, device=DEV)
        view = flat[gc.GUARD:gc.GUARD + n].view(dt)
    assert view.data_ptr() % 16 == 0
    return flat, view.view(shape)


def _launch_args(c, d, views):
    """(a, w, bias, keyword arguments) of kernels.gemm / kernels.gemm_kernel_name for a case."""
    A, W = gc.operand_tensors(c, d)
    A, W = A.to(DEV), W.to(DEV)
    bias = None if d["bias"] is None else torch.from_numpy(d["bias"]).float().to(DEV)
    kw = dict(M=c.M, lda=c.lda, split_k=bool(c.split_k))
    if c.epi in (gc.EPI_F16, gc.EPI_F32):
        out = views["out"][:c.M]
        kw.update(out=out, act=c.act)
        if c.resid != "none":
            r = torch.from_numpy(d["resid"]).float().to(DEV)
            if c.resid == "alias":
                out[:, :c.N] = r
                kw.update(resid=out)
            else:
                own = torch.full((c.M, c.ldo), float("nan"), device=DEV)
                own[:, :c.N] = r
                kw.update(resid=own)
    elif c.epi == gc.EPI_PATCH:
        kw.update(patch=dict(out=views["out"][:c.out_rows], pos=torch.from_numpy(d["pos"]).float().to(DEV), tpi=c.tpi))
    elif c.epi == gc.EPI_HEADS:
        kw.update(heads=dict(q=views.get("q"), k=views.get("k"), vt=views.get("vt"), T=c.T, H=c.H, part0=c.part0, t_off=c.t_off,
                             Tq_cap=c.Tq_cap, Tk_cap=c.Tk_cap, NP=c.NP, q_scale=c.q_scale, tiled=c.tiled))
    else:
        q = views.get("q")
        kw.update(arena=dict(q=None if q is None else q[:c.M], k=views.get("k"), v=views.get("vt"), T=c.T, H=c.H, part0=c.part0,
                             t_off=c.t_off, arena_rows=c.arena_rows, slot_stride=c.slot_stride, Tcap=c.Tk_cap, q_scale=c.q_scale))
    return A[:c.M + gc.NAN_ROWS], W[:c.N], bias, kw


@pytest.mark.parametrize("c", gc.CASES, ids=[c.name for c in gc.CASES])
def test_gemm_case_is_exact_and_confined(c, monkeypatch):
    from vidil_amd import kernels as K

    for key in gc.ENV_KEYS:
        monkeypatch.delenv(key, raising=False)
    for key, val in c.env.items():
        monkeypatch.setenv(key, val)
    d = gc.inputs(c)
    dt = gc.T16[c.dtype]
    shapes = gc.dest_shapes(c)
    flats, views = {}, {}
    for name, (shape, kind) in shapes.items():
        flats[name], views[name] = _alloc(shape, kind, dt)
    a, w, bias, kw = _launch_args(c, d, views)
    name = K.gemm_kernel_name(a, w, bias, **kw)
    assert name == gc.expected_kernel(c, cus=torch.cuda.get_device_properties(0).multi_processor_count), c.name
    assert gc.form_of(name) == c.kernel, (c.name, name)
    if c.split_k:
        assert K.split_k_serves(a, w, bias, **kw)
    K.gemm(a, w, bias, **kw)
    torch.cuda.synchronize()
    exp = gc.expected(c, d)
    counts = []
    for dest, (vals, written, _) in exp.items():
        got = flats[dest].cpu().numpy()
        if not c.exact:
            _, kind = shapes[dest]
            val = torch.from_numpy(got[gc.GUARD:gc.GUARD + vals.size].copy()).view(gc.float_type(c, kind)).double().numpy()[written]
            err = np.abs(val - vals[written])
            print(f"{c.name}: {dest}: max |d| vs float64 {np.nanmax(err):.3e}, {np.nanmax(err / gc.act_bound(c, vals[written])):.2f} of the bound")
        wrong = gc.verdict(c, dest, got, vals, written)
        assert wrong is None, f"{c.name}: {name}: {wrong}"
        counts.append(f"{dest}: {int(written.sum())} written, {got.size - int(written.sum())} sentinel")
    print(f"{c.name}: {name}: M={c.M} N={c.N} K={c.K}: " + "; ".join(counts))
