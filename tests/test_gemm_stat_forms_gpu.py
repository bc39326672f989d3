"""The epilogue features of vidil_gemm that tests/test_gemm_forms_gpu.py does not reach — the LayerNorm-fold consumer, the
row-partials producer and the 16-bit copy, the residual LayerNorm, out16_split3 = 1 / 2 and fp8 operands — on BOTH 256-row kernel
bodies (gemm256_kernel with VIDIL_GEMM4W=0, gemm4w_kernel with VIDIL_GEMM4W=1; the compensated producer on its 128-row form), at
the tile, group, part and column edges, against exact / float64 references (tests/gemm_stat_cases.py has the table, the inputs,
the references and the bounds; its preconditions are asserted by tests/test_gemm_stat_cases_cpu.py).

Per case and body: the name vidil_gemm_kernel_name reports is the one the table expects; one launch (split3: a second one
without `out`); every written element of every destination equals the reference BIT FOR BIT (bound tier and activations: within
the derived bound; the 16-bit copy, the planes and the row partials are then checked against the f32 rows the SAME launch wrote,
the copy and the planes bit for bit); everything else in every destination allocation — rows >= M of out / out16 / the partials,
columns >= N, plane 2 when out16_split3 == 2, the padding between planes, the f32 rows when `out` is NULL, the guards — still
holds its NaN sentinel.  The bodies of a case are compared with each other bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_cases as gc
import gemm_stat_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}


def _alloc(shape, kind, dt):
    """(flat integer allocation filled with the sentinel, the destination view inside it behind GUARD elements)."""
    n = int(np.prod(shape))
    it = {"f32": torch.int32, "t16": torch.int16, "f8": torch.int8}[kind]
    flat = torch.full((n + 2 * gc.GUARD,), sc.int_type(kind)[1], dtype=it, device=DEV)
    view = flat[gc.GUARD:gc.GUARD + n].view({"f32": torch.float32, "t16": dt, "f8": sc.F8}[kind])
    assert view.data_ptr() % 16 == 0
    return flat, view.view(shape)


def _f32(x, rows=0):
    """An f32 device tensor of a float64 array, followed by `rows` rows of NaN that nothing may read into a result."""
    t = torch.from_numpy(np.ascontiguousarray(x)).float()
    if rows:
        t = torch.cat([t, torch.full((rows,) + tuple(t.shape[1:]), float("nan"))])
    return t.to(DEV)


def _launch_args(c, d, views, out_null):
    """(a, w, bias, keyword arguments of kernels.gemm, struct fields the wrapper cannot express) for one launch of a case."""
    A, W = sc.operand_tensors(c, d)
    A, W = A.to(DEV), W.to(DEV)
    bias = None if d["bias"] is None else _f32(d["bias"])
    kw = dict(M=c.M, lda=c.lda, split_k=bool(c.split_k))
    patch = {}
    if c.fp8:
        kw.update(w_scale=_f32(d["w_scale"]), dtype16=gc.T16[c.dtype])
    if c.fold:
        kw.update(ln=(_f32(d["colsum"]), c.eps, _f32(d["stats_in"], 32)[:c.M]))
    if c.epi in (gc.EPI_F16, gc.EPI_F32, sc.EPI_F8):
        out = views["out"][:c.M]
        if not out_null:                # (split3 alone may leave `out` NULL: the f32 rows are then not written)
            kw.update(out=out)
        kw.update(act=c.act)
        if c.resid != "none":
            r = _f32(d["resid"])
            if c.resid == "alias":
                out[:, :c.N] = r
                kw.update(resid=out)
            else:
                own = torch.full((c.M, c.ldo), float("nan"), device=DEV)
                own[:, :c.N] = r
                kw.update(resid=own)
        if c.split3:
            # the wrapper takes dense planes [M, 3 N]; planes of N + pad columns are set in the struct
            flat = views["out16"].reshape(-1)
            kw.update(split3_out=flat[:c.M * 3 * c.N].view(c.M, 3 * c.N), split3_planes=c.split3)
            if c.ldo16_pad:
                patch["ldo16"] = c.ldo16
        elif c.out16:
            kw.update(out16=views["out16"][:c.M])
            if c.stats:
                kw.update(ln_stats_out=views["stats"][:c.M])
        if c.rln:
            kw.update(rln=(_f32(d["gamma"]), _f32(d["beta"]), c.eps, _f32(d["stats_in"], 32)[:c.M]))
    elif c.epi == gc.EPI_PATCH:
        kw.update(patch=dict(out=views["out"][:c.out_rows], pos=_f32(d["pos"]), tpi=c.tpi))
    elif c.epi == gc.EPI_HEADS:
        kw.update(heads=dict(q=views.get("q"), k=views.get("k"), vt=views.get("vt"), T=c.T, H=c.H, part0=c.part0, t_off=c.t_off,
                             Tq_cap=c.Tq_cap, Tk_cap=c.Tk_cap, NP=c.NP, q_scale=c.q_scale, tiled=c.tiled))
    else:
        q = views.get("q")
        kw.update(arena=dict(q=None if q is None else q[:c.M], k=views.get("k"), v=views.get("vt"), T=c.T, H=c.H, part0=c.part0,
                             t_off=c.t_off, arena_rows=c.arena_rows, slot_stride=c.slot_stride, Tcap=c.Tk_cap, q_scale=c.q_scale))
    return A[:c.M + gc.NAN_ROWS], W[:c.N], bias, kw, patch


def _run(K, a, w, bias, kw, patch):
    """(kernel name, launch) — through kernels.gemm, or through the struct where a field has to be set by hand."""
    from vidil_amd import _lib

    if not patch:
        name = K.gemm_kernel_name(a, w, bias, **kw)
        K.gemm(a, w, bias, **kw)
        return name
    g, _ = K._gemm_build(a, w, bias, **kw)
    for f, v in patch.items():
        setattr(g, f, v)
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.load().vidil_gemm_kernel_name(ctypes.byref(g), buf, 128), "gemm_kernel_name")
    _lib.check(_lib.load().vidil_gemm(ctypes.byref(g), torch.cuda.current_stream().cuda_stream), "gemm")
    return buf.value.decode()


def _one_launch(K, c, d, out_null):
    """name, {destination: integer allocation on the host} of one launch."""
    dt = gc.T16[c.dtype]
    flats, views = {}, {}
    for dest, (shape, kind) in sc.dest_shapes(c).items():
        flats[dest], views[dest] = _alloc(shape, kind, dt)
    a, w, bias, kw, patch = _launch_args(c, d, views, out_null)
    if c.split_k:
        assert K.split_k_serves(a, w, bias, **kw)
    name = _run(K, a, w, bias, kw, patch)
    torch.cuda.synchronize()
    return name, {k: v.cpu().numpy() for k, v in flats.items()}


@pytest.mark.parametrize("c", sc.CASES, ids=[c.name for c in sc.CASES])
def test_gemm_feature_case_is_exact_or_within_its_bound_and_confined(c, monkeypatch):
    from vidil_amd import kernels as K

    d = sc.inputs(c)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    first = None
    for body in c.bodies:
        cb = sc.with_body(c, body)
        for key in gc.ENV_KEYS:
            monkeypatch.delenv(key, raising=False)
        for key, val in cb.env.items():
            monkeypatch.setenv(key, val)
        results = {}
        for out_null in ((False, True) if c.split3 else (False,)):
            name, got = _one_launch(K, cb, d, out_null)
            assert name == sc.expected_kernel(cb, cus=cus), (c.name, body)
            assert gc.form_of(name) == body, (c.name, name)
            results[out_null] = got
            rows = None
            if not c.exact and c.epi == gc.EPI_F32 and (c.out16 or c.stats) and not out_null:
                rows = sc.written_rows(c, got["out"])
            for dest, (vals, written, bound) in sc.expected(c, d, out_rows=rows, out_null=out_null).items():
                wrong, worst = sc.verdict(c, dest, got[dest], vals, written, bound)
                assert wrong is None, f"{c.name}: {name}{' (out NULL)' if out_null else ''}: {wrong}"
                if bound is not None and np.isfinite(bound[written]).all():
                    key = (c.feature, body, dest if dest in ("out16", "stats") else "values")
                    WORST[key] = max(WORST.get(key, 0.0), worst)
                    print(f"{c.name}: {body}: {dest}: worst err / bound {worst:.4f}")
        if c.split3:        # the planes do not depend on whether the f32 rows are written as well
            assert np.array_equal(results[False]["out16"], results[True]["out16"]), f"{c.name}: {body}: planes differ with and without out"
        if first is None:
            first = results
        else:               # the two kernel bodies agree bit for bit
            for out_null, got in results.items():
                for dest in got:
                    assert np.array_equal(first[out_null][dest], got[dest]), f"{c.name}: {dest}: {c.bodies[0]} and {body} differ"
    print(f"{c.name}: {' / '.join(c.bodies)}: M={c.M} N={c.N} K={c.K} tier={c.tier} exact={c.exact}")


def test_worst_error_over_bound_per_group():
    """Prints, per (feature, kernel body, kind of destination), the worst err / bound the cases above measured (bit-equality cases
    measure nothing).  Runs after them; asserts only that no figure exceeds its bound — each case has asserted that already."""
    for key in sorted(WORST):
        print(f"worst err / bound: {key[0]:7s} {key[1]:18s} {key[2]:7s} {WORST[key]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
