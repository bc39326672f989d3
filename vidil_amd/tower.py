"""The pre-LN transformer block of the BLIP vision transformer and both CLIP towers, on the f32 residual stream:

    LN1 -> QKV GEMM (per-head Q/K/V scatter, q pre-scaled) -> softmax attention -> out-proj GEMM (+residual, in place) ->
    LN2 -> fc1 GEMM (+activation) -> fc2 GEMM (+residual, in place)

``pack_layer`` packs one layer's parameters into the dict ``run_layers`` reads; ``run_layers`` holds the launch list of each
operand form (plain / LayerNorm-folded, fp8, parity).  Patch and token embeddings, the LayerNorms around the stack, pooling and
projections stay with the models (vit.py, clip.py).
"""
from __future__ import annotations

import torch

from . import kernels as K
from .packing import FP8, fold_layernorm, v32, w3, w8, w16


def pack_layer(n1, qkv_w, qkv_b, o, n2, fc1, fc2, *, dtype, form="plain", fold_qkv=True):
    """One layer's operands.  n1 / n2: (gamma, beta) of the two LayerNorms; qkv_w / qkv_b: tuples of the Q | K | V weights and
    biases (one fused tensor, or three), concatenated along N; o / fc1 / fc2: (weight, bias) of the out-projection and the MLP.
    form:
      "plain"  — 16-bit weights and f32 vectors only (every form has these);
      "fold"   — + LayerNorm folded into the consuming GEMMs: ``fc1_f`` (LN2), and ``qkv_f`` (LN1) unless ``fold_qkv`` is False
                 (layer 0: its input is written by an embedding / LayerNorm kernel, not by a residual GEMM, so there is no
                 16-bit copy of the stream to read);
      "fp8"    — + ``*_w8`` / ``*_s``: e4m3 weights, per-output-row scaled;
      "parity" — + ``*_w3``: [W_hi | W_hi | W_lo] against [x_hi | x_lo | x_hi] rows (packing.set_parity_mode)."""
    c = dtype
    d = dict(
        n1g=v32(n1[0]), n1b=v32(n1[1]),
        qkv_w=w16(*qkv_w, dtype=c), qkv_b=v32(*qkv_b),
        o_w=w16(o[0], dtype=c), o_b=v32(o[1]),
        n2g=v32(n2[0]), n2b=v32(n2[1]),
        fc1_w=w16(fc1[0], dtype=c), fc1_b=v32(fc1[1]),
        fc2_w=w16(fc2[0], dtype=c), fc2_b=v32(fc2[1]))
    big = (("qkv", qkv_w), ("o", o[:1]), ("fc1", fc1[:1]), ("fc2", fc2[:1]))
    if form == "parity":
        for name, ws in big:
            d[name + "_w3"] = w3(*ws, dtype=c)
    elif form == "fp8":
        for name, ws in big:
            d[name + "_w8"], d[name + "_s"] = w8(*ws)
    elif form == "fold":
        d["fc1_f"] = fold_layernorm(fc1[0], fc1[1], n2[0], n2[1], c)
        if fold_qkv:
            w = qkv_w[0] if len(qkv_w) == 1 else torch.cat(list(qkv_w), dim=0)
            d["qkv_f"] = fold_layernorm(w, v32(*qkv_b), n1[0], n1[1], c)
    elif form != "plain":
        raise ValueError(f"pack_layer: unknown form {form!r}")
    return d


def run_layers(layers, x, B, T, H, eps, act, *, causal=False, kv_len=None, parity=False, f32_attn=True, arith=0, fp8=False,
               cls_last=False):
    """Run the packed ``layers`` in place on the f32 residual stream x [B*T, D]; ``act`` is fc1's activation (K.ACT_*).
    The form is the caller's decision: ``parity`` (layers with ``*_w3``; one without runs as a plain unfused block — the ViT's
    mixed form), else ``fp8`` (layers with ``*_w8``), else plain — LayerNorm-folded where a layer has ``fc1_f``.
    f32_attn / arith: the parity form's attention (packing.set_parity_attention).  cls_last: see ``_cls_last_layer``.
    Returns (rows, operand): rows is x — or, with cls_last, the f32 class-token rows [B, D] —, operand is the form's 16-bit
    operand buffer (plain: [M, D]; parity: [M, 3D] split rows; fp8: None), free for the caller's closing LayerNorm to write."""
    dev = x.device
    M, D = x.shape
    cdt = layers[0]["qkv_w"].dtype
    Dh = layers[0]["fc1_w"].shape[0]
    n = len(layers)
    # more than 32 rows -> LDS-staged attention, which takes V row-major (NP = 0): the QKV GEMM stores it like K with 16-B stores
    # and the kernel transposes it on the way into LDS — cheaper than scattering V^T from the GEMM epilogue.  Short sequences
    # (text batches, tiny test geometries) go through the direct kernels, which read V^T fragments straight from memory
    NP = 0 if T > 32 else (T + 15) // 16 * 16
    q = torch.empty((B, H, T, 64), dtype=cdt, device=dev)
    k = torch.empty((B, H, T, 64), dtype=cdt, device=dev)
    vt = torch.empty((B, H, T, 64) if NP == 0 else (B, H, 64, NP), dtype=cdt, device=dev)
    heads = dict(q=q, k=k, vt=vt, T=T, H=H, part0=0, t_off=0, Tq_cap=T, Tk_cap=T, NP=NP, q_scale=0.125)

    if parity:
        # Parity precision mode: the same block sequence with every GEMM on error-compensated operands (K tripled, ~3x the MFMA
        # work).  LayerNorm and attention write [hi | lo | hi] rows directly (VIDIL_DT_SPLIT3); fc1 + activation run in f32 and are
        # handed to fc2 as split rows by the GEMM's own epilogue (no f32 round trip).  Attention: "split" / "f32" — Q | K | V stay
        # f32 rows of the projection GEMM's output and vidil_attention_f32 reads them in place (split-operand MFMA or f32
        # arithmetic, no per-head scatter); "16" — the per-head scatter and the 16-bit kernels, Q / K / V and the probabilities
        # rounded to 16 bits.
        a3 = torch.empty((M, 3 * D), dtype=cdt, device=dev)
        o3 = torch.empty((M, 3 * D), dtype=cdt, device=dev)
        hid3 = torch.empty((M, 3 * Dh), dtype=cdt, device=dev)
        qkv32 = torch.empty((M, 3 * D), dtype=torch.float32, device=dev) if f32_attn else None
        # Which producers may leave the third plane of their [hi | lo | hi] rows unwritten (planes = 2): only those whose EVERY
        # consumer takes the K-loop form of the compensated product, which reads planes hi | lo alone.  That is asked per CALL
        # (K.split_k_serves) of the first compensated layer's four GEMMs — a3 feeds Q|K|V and fc1, o3 the out-projection, hid3
        # fc2 —, not assumed: the per-head epilogue with fewer than 8 tokens, for one, runs the plain K = 3 Kl product over all
        # three planes.  The consumers then state a_planes, so a launch that would read an unwritten plane fails (EINVAL)
        # instead of computing on it.  The 16-bit attention (kind "16") writes all three planes of o3, whatever ``planes`` is.
        l3 = next((l for l in layers if "qkv_w3" in l), None)
        planes = 3
        if l3 is not None:
            qkv_kw = dict(out=qkv32) if f32_attn else dict(heads=heads)
            if (K.split_k_serves(a3, l3["qkv_w3"], l3["qkv_b"], **qkv_kw) and K.split_k_serves(o3, l3["o_w3"], l3["o_b"], out=x, resid=x)
                    and K.split_k_serves(a3, l3["fc1_w3"], l3["fc1_b"], split3_out=hid3, act=act)
                    and K.split_k_serves(hid3, l3["fc2_w3"], l3["fc2_b"], out=x, resid=x)):
                planes = 2
        K.poison_third_plane(planes, a3, o3, hid3)
        if any("qkv_w3" not in l for l in layers):      # mixed form: scratch of the plain blocks
            xn = torch.empty((M, D), dtype=cdt, device=dev)
            o = torch.empty((M, D), dtype=cdt, device=dev)
            hid = torch.empty((M, Dh), dtype=cdt, device=dev)
        cls_last = cls_last and f32_attn and not causal and kv_len is None and T > 1
        for i, l in enumerate(layers):
            if "qkv_w3" not in l:       # plain 16-bit operands, unfused: both forms meet at the f32 residual stream
                K.layernorm(x, l["n1g"], l["n1b"], eps, out16=xn)
                K.gemm(xn, l["qkv_w"], l["qkv_b"], heads=heads)
                K.attention(q, k, vt, o, Bq=B, H=H, Nq=T, Nk=T, Tq_cap=T, Tk_cap=T, NP=NP, causal=causal, kv_len=kv_len)
                K.gemm(o, l["o_w"], l["o_b"], out=x, resid=x)
                K.layernorm(x, l["n2g"], l["n2b"], eps, out16=xn)
                K.gemm(xn, l["fc1_w"], l["fc1_b"], out=hid, act=act)
                K.gemm(hid, l["fc2_w"], l["fc2_b"], out=x, resid=x)
                continue
            K.layernorm(x, l["n1g"], l["n1b"], eps, out16=a3, split3=True, planes=planes)
            if cls_last and i == n - 1:
                return _cls_last_layer(l, x, a3, qkv32, B, T, H, eps, act, planes), a3
            if f32_attn:
                K.gemm(a3, l["qkv_w3"], l["qkv_b"], out=qkv32, split_k=True, a_planes=planes)
                K.attention_f32(qkv32[:, :D], qkv32[:, D:2 * D], qkv32[:, 2 * D:], o3, Bq=B, H=H, Nq=T, Nk=T, causal=causal, kv_len=kv_len,
                                arith=arith, planes=planes)
            else:
                K.gemm(a3, l["qkv_w3"], l["qkv_b"], heads=heads, split_k=True, a_planes=planes)
                K.attention(q, k, vt, o3, Bq=B, H=H, Nq=T, Nk=T, Tq_cap=T, Tk_cap=T, NP=NP, causal=causal, kv_len=kv_len, split3=True)
            K.gemm(o3, l["o_w3"], l["o_b"], out=x, resid=x, split_k=True, a_planes=planes if f32_attn else 3)
            K.layernorm(x, l["n2g"], l["n2b"], eps, out16=a3, split3=True, planes=planes)
            K.gemm(a3, l["fc1_w3"], l["fc1_b"], split3_out=hid3, act=act, split_k=True, split3_planes=planes, a_planes=planes)
            K.gemm(hid3, l["fc2_w3"], l["fc2_b"], out=x, resid=x, split_k=True, a_planes=planes)
        return x, a3

    if fp8:
        # fp8 tower mode (BASELINE config 5): LN -> fp8 as a stand-alone kernel (its output is well scaled; the raw stream is
        # not), QKV / out-proj / fc1 / fc2 on e4m3 operands at twice the 16-bit MFMA rate, attention on the 16-bit companion type
        # writing fp8.  NOT a parity mode: e4m3 carries 3 mantissa bits (tests/test_fp8_gpu.py states the measured deviation).
        xn8 = torch.empty((M, D), dtype=FP8, device=dev)
        o8 = torch.empty((M, D), dtype=FP8, device=dev)
        hid8 = torch.empty((M, Dh), dtype=FP8, device=dev)
        for l in layers:
            K.layernorm(x, l["n1g"], l["n1b"], eps, out16=xn8)
            K.gemm(xn8, l["qkv_w8"], l["qkv_b"], heads=heads, w_scale=l["qkv_s"])
            K.attention(q, k, vt, o8, Bq=B, H=H, Nq=T, Nk=T, Tq_cap=T, Tk_cap=T, NP=NP, causal=causal, kv_len=kv_len)
            K.gemm(o8, l["o_w8"], l["o_b"], out=x, resid=x, w_scale=l["o_s"], dtype16=cdt)
            K.layernorm(x, l["n2g"], l["n2b"], eps, out16=xn8)
            K.gemm(xn8, l["fc1_w8"], l["fc1_b"], out=hid8, act=act, w_scale=l["fc1_s"], dtype16=cdt)
            K.gemm(hid8, l["fc2_w8"], l["fc2_b"], out=x, resid=x, w_scale=l["fc2_s"], dtype16=cdt)
        return x, None

    xn = torch.empty((M, D), dtype=cdt, device=dev)
    o = torch.empty((M, D), dtype=cdt, device=dev)
    hid = torch.empty((M, Dh), dtype=cdt, device=dev)
    stats = torch.empty((M, D // 64, 2), dtype=torch.float32, device=dev) if "fc1_f" in layers[0] else None
    for i, l in enumerate(layers):
        # Folded LayerNorm: the residual GEMMs (out-proj, fc2) also store the stream in the operand type (``xn`` then holds RAW
        # x, not LN(x)) with per-row partial sums, and the next GEMM applies the LayerNorm to its accumulators
        fused = "fc1_f" in l
        if fused and i > 0:
            w_, b_, cs = l["qkv_f"]
            K.gemm(xn, w_, b_, heads=heads, ln=(cs, eps, stats))
        else:
            K.layernorm(x, l["n1g"], l["n1b"], eps, out16=xn)
            K.gemm(xn, l["qkv_w"], l["qkv_b"], heads=heads)
        K.attention(q, k, vt, o, Bq=B, H=H, Nq=T, Nk=T, Tq_cap=T, Tk_cap=T, NP=NP, causal=causal, kv_len=kv_len)
        if fused:
            K.gemm(o, l["o_w"], l["o_b"], out=x, resid=x, out16=xn, ln_stats_out=stats)
            w_, b_, cs = l["fc1_f"]
            K.gemm(xn, w_, b_, out=hid, act=act, ln=(cs, eps, stats))
            K.gemm(hid, l["fc2_w"], l["fc2_b"], out=x, resid=x, out16=xn if i + 1 < n else None,
                   ln_stats_out=stats if i + 1 < n else None)
        else:
            K.gemm(o, l["o_w"], l["o_b"], out=x, resid=x)
            K.layernorm(x, l["n2g"], l["n2b"], eps, out16=xn)
            K.gemm(xn, l["fc1_w"], l["fc1_b"], out=hid, act=act)
            K.gemm(hid, l["fc2_w"], l["fc2_b"], out=x, resid=x)
    return x, xn


def _cls_last_layer(l, x, a3, qkv32, B, T, H, eps, act, planes):
    """The parity form's LAST layer for a caller that reads token 0 of every sequence only (the CLIP vision tower: pooled output
    = post_layernorm(CLS), HF CLIPVisionTransformer), with the f32-row attention kinds.  a3 holds LN1(x) as split rows with
    ``planes`` planes.  K | V are computed for all rows; everything else — the query, the attention output, out-proj, LayerNorm 2,
    fc1, fc2 — for the B class-token rows alone (10/12 of the layer's GEMM rows are not computed: ~7 % of a 12-layer tower).
    Returns the f32 class-token rows [B, D].  Per class-token row the arithmetic is the full layer's (its attention in plain f32
    arithmetic instead of the split form)."""
    M, D = x.shape
    cdt, dev = a3.dtype, x.device
    Dh = l["fc1_w"].shape[0]
    kv32 = qkv32.view(-1)[:M * 2 * D].view(M, 2 * D)               # (the layers' scratch, re-shaped: [M, 2D] keys | values)
    K.gemm(a3, l["qkv_w3"][D:], l["qkv_b"][D:], out=kv32, split_k=True, a_planes=planes)
    a3c = a3.view(B, T, 3 * D)[:, 0].contiguous()                  # [B, 3D] operand rows of the class tokens
    if planes == 2:
        a3c[:, 2 * D:] = a3c[:, :D]                                # (three valid planes: the small launches below may be plain)
    q32c = K.gemm(a3c, l["qkv_w3"][:D], l["qkv_b"][:D], out_dtype=torch.float32, split_k=True)
    o3c = torch.empty((B, 3 * D), dtype=cdt, device=dev)
    K.attention_f32(q32c, kv32[:, :D], kv32[:, D:], o3c, Bq=B, H=H, Nq=1, Nk=T, kv_rows=T, arith=0, planes=3)
    xc = x.view(B, T, D)[:, 0].contiguous()                        # [B, D] f32 residual rows of the class tokens
    K.gemm(o3c, l["o_w3"], l["o_b"], out=xc, resid=xc, split_k=True)
    K.layernorm(xc, l["n2g"], l["n2b"], eps, out16=a3c, split3=True, planes=3)
    h3c = K.gemm(a3c, l["fc1_w3"], l["fc1_b"], split3_out=torch.empty((B, 3 * Dh), dtype=cdt, device=dev), act=act,
                 split_k=True, split3_planes=3)
    K.gemm(h3c, l["fc2_w3"], l["fc2_b"], out=xc, resid=xc, split_k=True)
    return xc
