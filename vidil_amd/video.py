"""What the video-level heads (BLIP_Retrieval, BLIP_Video_VQA, BLIP_Video_Decoder) and their evaluation loops share: a video is
N frames whose ViT tokens are ONE encoder sequence of N*T keys.  Imports no head; a refusal speaks under the name it is given."""
from __future__ import annotations

import torch

from .packing import FP8, compute_dtype, parity_mode, require_cuda

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # run_video_CapFilt.py:133
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_VIDEO_TOKENS = 16384         # keys of vidil_attention's long-key and key-split forms: a video's N frames x T tokens
VIT_VIDEOS = 16                  # videos per ViT pass: BLIP_Video_Decoder's, and video_qa.evaluation's when ``videos`` is one tensor
KV_BLOCK_BYTES = 4 << 30         # budget of one block's cross-attention K / V


def require_video_tokens(n_tokens, who):
    """The attention kernels serve at most MAX_VIDEO_TOKENS keys: refuse more here, by name, before anything is launched."""
    if n_tokens > MAX_VIDEO_TOKENS:
        raise ValueError(f"{who}: {n_tokens} tokens per video (frames x tokens per frame) exceed the {MAX_VIDEO_TOKENS} "
                         f"keys the attention kernels serve — sample fewer frames or build the model with a smaller image_size")


def require_plain(model, who, task, why):
    """Refuse the parity precision mode and fp8 on any module of ``model``: ``task`` is not built for them (``why``)."""
    for m in model.modules():
        if parity_mode(m):
            raise ValueError(f"{who}: the parity precision mode is not built for {task} ({why}) — set_parity_mode(False, model)")
        if compute_dtype(m) == FP8:
            raise ValueError(f"{who}: fp8 is not built for {task} — set_compute_dtype('f16' or 'bf16', model)")


def video_rows(tokens16, B, who):
    """Te of tokens16 [B*Te, width]: the rows must divide into B videos of at most MAX_VIDEO_TOKENS each."""
    if B <= 0 or tokens16.shape[0] % B:
        raise ValueError(f"{who}: {tokens16.shape[0]} token rows do not divide into B={B} videos")
    require_video_tokens(tokens16.shape[0] // B, who)
    return tokens16.shape[0] // B


@torch.no_grad()
def frame_tokens(visual_encoder, video, *, who, u8=None, videos_per_pass=None):
    """f32 [B,N,3,S,S] (normalised) or uint8 [B,N,S,S,3] frames (already S x S; /255 and the normalisation are fused into the
    patch kernel) -> 16-bit [B*N*T, width]: the ViT over the B*N frames, ``videos_per_pass`` videos per pass (default: all in
    one).  A video's N*T rows are contiguous — as encoder states it is ONE unit of N*T tokens, no copy.  ``u8``: the layout
    the caller takes (default: by the dtype).  ``who``: "Class.method" — another layout and more than MAX_VIDEO_TOKENS tokens
    are refused under the class's name, a host tensor under the method's; None: nothing is refused here (the caller has)."""
    if u8 is None:
        u8 = video.dtype == torch.uint8
    if who is not None:
        name = who.split(".")[0]
        if u8 and (video.dim() != 5 or video.shape[-1] != 3 or video.dtype != torch.uint8):
            raise ValueError(f"{name}: uint8 [B,N,S,S,3] expected, got {video.dtype} {tuple(video.shape)}")
        if not u8 and (video.dim() != 5 or video.shape[2] != 3):
            raise ValueError(f"{name}: f32 [B,N,3,S,S] expected, got {tuple(video.shape)}")
        require_video_tokens(video.shape[1] * (visual_encoder.patch_embed.num_patches + 1), name)
        require_cuda(video, who)
    B, parts = video.shape[0], []
    for b0 in (0,) if videos_per_pass is None else range(0, B, videos_per_pass):
        frames = video[b0:b0 + (videos_per_pass or B)].flatten(0, 1)
        parts.append(visual_encoder.forward_u8(frames, CLIP_MEAN, CLIP_STD)[1] if u8 else visual_encoder.forward_both(frames)[1])
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def videos_per_block(config, tokens_per_video):
    """Videos whose cross-attention K / V fit KV_BLOCK_BYTES: KV_BLOCK_BYTES // (L * 2 * N*T * C * 2 bytes), at least 1."""
    return max(1, KV_BLOCK_BYTES // (config.num_hidden_layers * 2 * tokens_per_video * config.hidden_size * 2))


def group_table(unit_of_item, n_units, what="unit_of_item"):
    """unit_of_item int64 [P] in [0, n_units) (host; pure) -> (group_start int32 [n_units+1], max_group): sorted by unit, the
    items of unit u are group_start[u] .. group_start[u+1]-1 (empty for a unit without one); ``max_group`` is the largest gap."""
    if unit_of_item.numel() and not (0 <= int(unit_of_item.min()) and int(unit_of_item.max()) < n_units):
        raise ValueError(f"{what} must hold indices in [0, {n_units})")
    group_start = torch.zeros(n_units + 1, dtype=torch.int64)
    group_start[1:] = torch.cumsum(torch.bincount(unit_of_item, minlength=n_units), 0)
    return group_start.to(torch.int32), int((group_start[1:] - group_start[:-1]).max()) if n_units else 0


def blocks(group_start, n_units, per):
    """The walk over ``n_units`` videos, ``per`` at a time: yields (b0, b1, p0, p1, local_table) for every block of videos
    b0 .. b1-1 that has items, p0 .. p1-1; local_table int32 [b1-b0+1] is the block's own table, group_start[b0:b1+1] - p0."""
    gs = group_start.long()
    for b0 in range(0, n_units, per):
        b1 = min(n_units, b0 + per)
        p0, p1 = int(gs[b0]), int(gs[b1])
        if p1 > p0:
            yield b0, b1, p0, p1, (gs[b0:b1 + 1] - p0).to(torch.int32)


def middle_frame(videos):
    """[b, N, ...] -> [b, 1, ...]: frame int(N / 2), what ``video_representation: single_frame`` looks at."""
    return videos[:, int(videos.shape[1] / 2), None]


def phase_timer(timings):
    """lap = phase_timer(timings): ``t0 = lap()`` marks a start on the current stream and ``lap(name, t0)`` adds the seconds
    between that mark and now to timings[name] (HIP events, synchronised at the end of the phase) and returns a new mark.
    With ``timings`` None nothing is recorded and nothing is synchronised."""
    def lap(name=None, t0=None):
        if timings is None:
            return None
        now = torch.cuda.Event(enable_timing=True)
        now.record()
        if name is not None:
            now.synchronize()
            timings[name] = timings.get(name, 0.0) + t0.elapsed_time(now) / 1e3
        return now
    return lap
