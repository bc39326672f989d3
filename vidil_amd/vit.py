"""BLIP vision transformer on the HIP kernels.

Mirror of the reference ``VisionTransformer`` (models/vit.py:113-194): same
constructor arguments, same parameter names (so BLIP ``.pth`` checkpoints load
unchanged: ``patch_embed.proj.weight``, ``cls_token``, ``pos_embed``,
``blocks.N.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}``, ``norm``), same
``forward(x[B,3,S,S]) -> [B,1+P,width]`` fp32 contract.  The arithmetic is:

    patchify (f32->T16 im2col) -> GEMM(+bias+pos, row remap) -> 12 x [
        [LN+]QKV GEMM (per-head Q/K/V scatter, q pre-scaled) -> softmax attention ->
        proj GEMM (+residual, in place, + T16 copy of the stream) ->
        [LN+]fc1 GEMM (+erf-GELU) -> fc2 GEMM (+residual, + T16 copy) ] -> LN

where "[LN+]" is the block's LayerNorm folded into the GEMM (statistics from the A fragments the GEMM streams,
normalisation applied to the accumulators; ``fuse_layernorm``) — only block 0's norm1 and the final norm run as
stand-alone LayerNorm kernels —

with the residual stream, LayerNorm statistics and softmax in f32 and the MFMA
operands in the model's compute dtype (f16 or bf16, packing.set_compute_dtype).
The blocks are packed and run by tower.py (shared with the CLIP towers), which also holds
the fp8 and parity forms of the block.
"""
from __future__ import annotations

import math
from functools import partial

import torch
import torch.nn as nn

from . import kernels as K
from .packing import PackedCache, require_cuda, v32, w3_patch, w16_patch, parity_attention_arith, parity_attention_f32, parity_attention_kind
from .tower import pack_layer, run_layers


class PatchEmbed(nn.Module):
    """Parameter holder matching timm's PatchEmbed (``proj`` = Conv2d k=s=patch)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.grid_size = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=False, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class VisionTransformer(PackedCache, nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, representation_size=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, norm_layer=None,
                 use_grad_checkpointing=False, ckpt_layer=0):
        super().__init__()
        if embed_dim // num_heads != 64:
            raise ValueError("vidil_amd ViT kernels are built for head_dim 64")
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.ln_eps = 1e-6  # models/vit.py:142
        # LayerNorm folded into the QKV / fc1 GEMMs (vidil_gemm_args.ln_fold): on unless VIDIL_FUSE_LN=0
        import os
        self.fuse_layernorm = os.environ.get("VIDIL_FUSE_LN", "1") != "0"
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=self.ln_eps)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([
            Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        # init rules of models/vit.py:163-174
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ------------------------------------------------------------------ packing
    def pack_flags(self):
        return (self.fuse_layernorm, self.fp8, self.parity, self.parity_last_blocks, parity_attention_kind(self))

    @property
    def parity_last_blocks(self):
        """Parity precision mode, MIXED form (round 4): only the last k blocks run on error-compensated operands, the
        first depth - k on plain 16-bit operands (unfused LayerNorm kernels + plain GEMMs: both forms meet at the f32
        residual stream).  None = all blocks (the default).  Rounding errors of the tower accumulate like a random walk over
        its 48 GEMMs, so compensating the last k of 12 blocks removes ~k/12 of the tower's error variance at ~k/12 of the
        3x cost — tests/probes/probe_parity_mix.py measures caption-logit error and time for every k."""
        return self.__dict__.get("_parity_last_blocks")

    def set_parity_last_blocks(self, k):
        if k is not None and not (0 <= int(k) <= len(self.blocks)):
            raise ValueError(f"parity_last_blocks must be in 0..{len(self.blocks)}")
        self.__dict__["_parity_last_blocks"] = None if k is None else int(k)

    def _pack(self):
        D = self.embed_dim
        pe = self.patch_embed.proj
        c = self.cdt
        p = dict(
            pe_w=w16_patch(pe.weight, c), pe_b=v32(pe.bias),
            cls=v32(self.cls_token), pos=v32(self.pos_embed).view(-1, D),
            norm_g=v32(self.norm.weight), norm_b=v32(self.norm.bias), blocks=[])
        wb = lambda m: (m.weight, m.bias)
        k_par = self.parity_last_blocks
        for i, b in enumerate(self.blocks):
            if self.parity:     # (mixed form: only the last parity_last_blocks blocks; the others keep their plain operands)
                form = "parity" if k_par is None or i >= len(self.blocks) - k_par else "plain"
            else:
                form = "fp8" if self.fp8 else "fold" if self.fuse_layernorm else "plain"
            p["blocks"].append(pack_layer(wb(b.norm1), (b.attn.qkv.weight,), (b.attn.qkv.bias,), wb(b.attn.proj), wb(b.norm2),
                                          wb(b.mlp.fc1), wb(b.mlp.fc2), dtype=c, form=form, fold_qkv=i > 0))
        p["fp8"] = self.fp8
        p["parity"] = self.parity
        if self.parity:
            p["pe_w3"] = w3_patch(pe.weight, c)
        return p

    # ------------------------------------------------------------------ forward
    def embed_patches(self, patches16, B):
        """patches16: f16 [B*P, 3*ps*ps] (from patchify_*).  Returns the f32 residual stream [B*T, D]."""
        p = self.packed()
        D, P = self.embed_dim, self.patch_embed.num_patches
        T = P + 1
        x = torch.empty((B * T, D), dtype=torch.float32, device=patches16.device)
        # (parity mode: patches16 holds [hi | lo | hi] rows, see forward_u8)
        K.gemm(patches16, p["pe_w3"] if p["parity"] else p["pe_w"], p["pe_b"], patch=dict(out=x, pos=p["pos"], tpi=P), split_k=p["parity"])
        K.set_cls_row(x, p["cls"], p["pos"], B, T, D)
        return x

    def run_blocks(self, x, B, want16=True):
        """x: f32 [B*T, D] residual stream (modified in place).  Returns (y32, y16) after the final LN; in the parity precision
        mode y16 is [M, 3D]: the [hi | lo | hi] split rows of the final LayerNorm (the cross K|V projection's operand)."""
        p = self.packed()
        T = self.patch_embed.num_patches + 1
        par = p["parity"]
        _, y16 = run_layers(p["blocks"], x, B, T, self.num_heads, self.ln_eps, K.ACT_GELU_ERF, parity=par, fp8=p["fp8"],
                            f32_attn=parity_attention_f32(self), arith=parity_attention_arith(self))
        # the final LayerNorm writes its 16-bit rows into the layers' operand buffer (the fp8 form has none of that type: a fresh one)
        if not want16:
            y16 = None
        elif y16 is None:
            y16 = torch.empty(x.shape, dtype=self.cdt, device=x.device)
        y32 = torch.empty_like(x)
        # (parity: the image tokens leave this module: their consumer — BertModel.project_cross_kv, any epilogue, any token count
        #  — is not known here, so all three planes are written: one launch per forward)
        K.layernorm(x, p["norm_g"], p["norm_b"], self.ln_eps, out16=y16, out32=y32, split3=par, planes=3)
        return y32, y16

    def forward_both(self, x):
        """x f32 [B,3,S,S] on the GPU -> (f32 [B,T,D], f16 [B*T,D])."""
        require_cuda(x, "VisionTransformer.forward")
        B = x.shape[0]
        ps = self.patch_embed.patch_size[0]
        patches = K.patchify_f32(x.contiguous().float(), ps, dtype=self.cdt, split3=self.parity)
        xr = self.embed_patches(patches, B)
        y32, y16 = self.run_blocks(xr, B)
        return y32.view(B, -1, self.embed_dim), y16

    def forward_u8(self, frames_u8, mean, std):
        """uint8 [B,S,S,3] frames (already S x S) with fused /255 + normalise."""
        require_cuda(frames_u8, "VisionTransformer.forward_u8")
        B = frames_u8.shape[0]
        ps = self.patch_embed.patch_size[0]
        patches = K.patchify_u8(frames_u8.contiguous(), ps, mean, std, dtype=self.cdt, split3=self.parity)
        xr = self.embed_patches(patches, B)
        y32, y16 = self.run_blocks(xr, B)
        return y32.view(B, -1, self.embed_dim), y16

    def forward(self, x, register_blk=-1):
        return self.forward_both(x)[0]


def interpolate_pos_embed(pos_embed_checkpoint, visual_encoder):
    """Resize a checkpoint's position grid to this encoder's (reference: models/vit.py:281-305)."""
    width = pos_embed_checkpoint.shape[-1]
    num_patches = visual_encoder.patch_embed.num_patches
    extra = visual_encoder.pos_embed.shape[-2] - num_patches
    old = int((pos_embed_checkpoint.shape[-2] - extra) ** 0.5)
    new = int(num_patches ** 0.5)
    if old == new:
        return pos_embed_checkpoint
    keep = pos_embed_checkpoint[:, :extra]
    grid = pos_embed_checkpoint[:, extra:].reshape(-1, old, old, width).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, size=(new, new), mode="bicubic", align_corners=False)
    grid = grid.permute(0, 2, 3, 1).flatten(1, 2)
    print("reshape position embedding from %d to %d" % (old ** 2, new ** 2))
    return torch.cat((keep, grid), dim=1)
