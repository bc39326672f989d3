"""vidil_amd/video.py on the GPU: ``frame_tokens`` with the real ViT at its smallest (ViT-B/16 at 32 x 32: T = 5), f16.  ONE
visual_encoder serves a BLIP_Retrieval, a BLIP_Video_VQA and a BLIP_Video_Decoder built on the small MED geometry: the three
heads launch the same kernels on the same frames, so their token rows are compared for EQUALITY — no tolerance."""
import json

import pytest
import torch

from test_models_gpu import _small_med_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, T, WIDTH = 32, 5, 768


@pytest.fixture(scope="module")
def heads(tmp_path_factory):
    from vidil_amd.blip import BLIP_Video_Decoder, create_vit
    from vidil_amd.blip_retrieval import BLIP_Retrieval
    from vidil_amd.blip_vqa import BLIP_Video_VQA
    from vidil_amd.packing import set_compute_dtype
    from vidil_amd.tokenizer import SyntheticBertTokenizer

    c = _small_med_cfg()
    path = tmp_path_factory.mktemp("cfg") / "med_small.json"
    path.write_text(json.dumps({k: getattr(c, k) for k in ("hidden_size", "num_attention_heads", "intermediate_size", "num_hidden_layers",
                                                           "vocab_size", "max_position_embeddings", "encoder_width")}))
    torch.manual_seed(23)
    vit, width = create_vit("base", SIZE)
    assert width == WIDTH and vit.patch_embed.num_patches + 1 == T
    out = {}
    for cls in (BLIP_Retrieval, BLIP_Video_VQA, BLIP_Video_Decoder):
        m = cls(med_config=str(path), image_size=SIZE, vit="base", tokenizer=SyntheticBertTokenizer())
        m.visual_encoder = vit
        set_compute_dtype("f16", m)
        out[cls.__name__] = m.eval().to(DEV)
    assert all(m.visual_encoder is vit for m in out.values())
    return out


def _frames(B, N):
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (B, N, SIZE, SIZE, 3), dtype=torch.uint8, generator=g)
    return u8.to(DEV), torch.randn(B, N, 3, SIZE, SIZE, generator=g).to(DEV)


def test_the_three_heads_give_the_same_token_rows_bit_for_bit(heads):
    B, N = 2, 2
    u8, f32 = _frames(B, N)
    r, q, d = heads["BLIP_Retrieval"], heads["BLIP_Video_VQA"], heads["BLIP_Video_Decoder"]
    rows_u8 = [r.video_features_u8(u8)[0], q.video_tokens_u8(u8), d.video_tokens_u8(u8)]
    rows_f32 = [r.video_features(f32)[0], q.video_tokens(f32), d.video_tokens(f32)]
    for rows in (rows_u8, rows_f32):
        assert all(x.shape == (B * N * T, WIDTH) and x.dtype == torch.float16 for x in rows)
        assert bool(torch.isfinite(rows[0].float()).all()) and rows[0].float().std().item() > 0
        assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
    assert not torch.equal(rows_u8[0], rows_f32[0])                                       # (the two inputs are different frames)
    assert r.video_features_u8(u8)[1].shape == (B, 256)                                   # the head's own part is still behind it


def test_the_decoders_vit_passes_are_direct_calls_on_the_frames_in_order(heads, monkeypatch):
    from vidil_amd import video as V
    from vidil_amd.video import CLIP_MEAN, CLIP_STD

    B, N = 3, 2
    u8, f32 = _frames(B, N)
    d, vit = heads["BLIP_Video_Decoder"], heads["BLIP_Video_Decoder"].visual_encoder
    monkeypatch.setattr(V, "VIT_VIDEOS", 2)                                               # passes of 2 videos: frames 0-3, then 4-5
    flat = u8.view(B * N, SIZE, SIZE, 3)
    want = torch.cat([vit.forward_u8(flat[:4], CLIP_MEAN, CLIP_STD)[1], vit.forward_u8(flat[4:], CLIP_MEAN, CLIP_STD)[1]], 0)
    assert torch.equal(d.video_tokens_u8(u8), want) and want.shape == (B * N * T, WIDTH)
    flat = f32.view(B * N, 3, SIZE, SIZE)
    want = torch.cat([vit.forward_both(flat[:4])[1], vit.forward_both(flat[4:])[1]], 0)
    assert torch.equal(d.video_tokens(f32), want)
    assert torch.equal(V.frame_tokens(vit, u8, who="BLIP_Video_Decoder.video_tokens_u8", videos_per_pass=2), d.video_tokens_u8(u8))
