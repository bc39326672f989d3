"""vidil_amd/video.py, what the video-level heads share, without a GPU: the group table and the walk over blocks against brute
force, the K / V budget against its formula and both entry points, and ``frame_tokens`` on a ViT that records its calls."""
import types

import numpy as np
import pytest
import torch

from common import ROOT  # noqa: F401  (puts the repository root on sys.path)

HEADS = ("BLIP_Retrieval", "BLIP_Video_VQA", "BLIP_Video_Decoder")


# ---------------------------------------------------------------------------------------------- group_table
def _brute_table(units, n):
    counts = [sum(1 for u in units if u == j) for j in range(n)]
    return [sum(counts[:j]) for j in range(n + 1)], max(counts, default=0)


def test_group_table_against_a_brute_force_count():
    from vidil_amd.video import group_table

    rng = np.random.default_rng(5)
    cases = [([], 0), ([], 3), ([0], 1), ([2, 2, 2], 5), ([1, 3, 1, 0, 1, 3, 1], 4)]
    cases += [(rng.integers(0, n, size=p).tolist(), n) for n, p in ((1, 7), (9, 40), (30, 12), (6, 200))]
    for units, n in cases:
        gs, mg = group_table(torch.tensor(units, dtype=torch.int64), n)
        want_gs, want_mg = _brute_table(units, n)
        assert gs.dtype == torch.int32 and gs.tolist() == want_gs and mg == want_mg and isinstance(mg, int), (units, n)
    assert any(0 in np.diff(_brute_table(u, n)[0]) for u, n in cases if u)           # units without an item are among them


def test_group_table_refuses_an_index_out_of_range():
    from vidil_amd.video import group_table

    for bad in ([0, 3], [-1, 0], [3]):
        with pytest.raises(ValueError, match=r"unit_of_item must hold indices in \[0, 3\)"):
            group_table(torch.tensor(bad), 3)
    with pytest.raises(ValueError, match=r"video_of_question must hold indices in \[0, 0\)"):
        group_table(torch.tensor([0]), 0, "video_of_question")


def test_pair_union_and_video_major_order_return_what_they_did():
    from vidil_amd.blip_vqa import video_major_order
    from vidil_amd.video_retrieval import pair_union

    s = video_major_order([1, 3, 1, 0, 1, 3, 1], 4)
    assert sorted(s) == ["group_start", "inverse", "max_group", "order"]
    assert s["group_start"].dtype == torch.int32 and s["group_start"].tolist() == [0, 1, 5, 5, 7] and s["max_group"] == 4
    assert s["order"].tolist() == [3, 0, 2, 4, 6, 1, 5] and s["inverse"].tolist() == [1, 5, 2, 0, 3, 6, 4]
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(ValueError, match=r"^video_of_question must hold indices in \[0, 4\)$"):
            video_major_order(bad, 4)
    empty = video_major_order([], 0)
    assert empty["group_start"].tolist() == [0] and empty["max_group"] == 0
    p = pair_union(torch.tensor([[0, 1], [1, 2], [2, 0]]), torch.tensor([[0, 2], [2, 1], [2, 2]]))
    assert sorted(p) == ["group_start", "max_group", "pair_text", "pair_video", "slot_t2v", "slot_v2t"]
    assert list(zip(p["pair_video"].tolist(), p["pair_text"].tolist())) == [(0, 0), (0, 1), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
    assert p["group_start"].dtype == torch.int32 and p["group_start"].tolist() == [0, 2, 4, 7] and p["max_group"] == 3
    assert p["slot_v2t"].tolist() == [[0, 1], [2, 3], [6, 4]] and p["slot_t2v"].tolist() == [[0, 4], [5, 2], [6, 6]]
    p = pair_union(torch.empty((4, 0), dtype=torch.int64), torch.tensor([[1], [1], [3]]))
    assert p["group_start"].tolist() == [0, 0, 2, 2, 3] and p["max_group"] == 2           # videos 0 and 2: empty groups


# ---------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("counts", [[0, 0, 3, 0, 1, 2, 0, 0, 4, 0], [2, 0, 0, 0, 0, 1], [0, 0, 0], [5], [1, 1, 1, 1]],
                         ids=["empty_start_middle_end", "long_empty_run", "all_empty", "one_unit", "no_empty"])
def test_blocks_cover_every_item_once_in_order_and_skip_empty_blocks(counts):
    from vidil_amd.video import blocks, group_table

    n = len(counts)
    gs, _ = group_table(torch.repeat_interleave(torch.arange(n), torch.tensor(counts)), n)
    for per in (1, 2, 3, n, n + 5):
        seen, last_b1 = [], 0
        for b0, b1, p0, p1, local in blocks(gs, n, per):
            assert b0 % per == 0 and b0 >= last_b1 and b1 == min(n, b0 + per)        # whole blocks of ``per``, in order
            assert p1 > p0 and (p0, p1) == (int(gs[b0]), int(gs[b1]))                # no empty block
            assert local.dtype == torch.int32 and local[0] == 0 and local[-1] == p1 - p0
            assert torch.equal(local, (gs[b0:b1 + 1].long() - p0).to(torch.int32))
            seen += list(range(p0, p1))
            last_b1 = b1
        assert seen == list(range(sum(counts))), per                                  # every item once, in order
        skipped = sum(1 for b0 in range(0, n, per) if sum(counts[b0:b0 + per]) == 0)
        assert len(list(blocks(gs, n, per))) == -(-n // per) - skipped


# ---------------------------------------------------------------------------------------------- videos_per_block
def test_videos_per_block_is_the_one_formula_behind_both_entry_points():
    from vidil_amd import video as V
    from vidil_amd.blip import BLIP_Video_Decoder
    from vidil_amd.video_retrieval import KV_BLOCK_BYTES, default_videos_per_block

    assert V.KV_BLOCK_BYTES == KV_BLOCK_BYTES == 4 << 30
    for L, C in ((12, 768), (2, 256), (24, 1024)):
        cfg = types.SimpleNamespace(num_hidden_layers=L, hidden_size=C)
        for Te in (1, 5, 197, 1576, 4616, 16384, 10 ** 9):
            want = max(1, KV_BLOCK_BYTES // (L * 2 * Te * C * 2))
            assert V.videos_per_block(cfg, Te) == want
            assert default_videos_per_block(types.SimpleNamespace(text_encoder=types.SimpleNamespace(config=cfg)), Te) == want
            assert BLIP_Video_Decoder.videos_per_block(types.SimpleNamespace(text_decoder=types.SimpleNamespace(config=cfg)), Te) == want
    assert V.videos_per_block(types.SimpleNamespace(num_hidden_layers=12, hidden_size=768), 1576) == 73
    assert V.videos_per_block(types.SimpleNamespace(num_hidden_layers=12, hidden_size=768), 10 ** 9) == 1       # floored at 1


# ---------------------------------------------------------------------------------------------- frame_tokens
class _RecordingViT:
    """The interface frame_tokens uses.  A frame's first value is its number; its T = 2 token rows hold 10 * number + row."""

    def __init__(self, num_patches=1):
        self.patch_embed = types.SimpleNamespace(num_patches=num_patches)
        self.calls = []

    def _rows(self, numbers):
        rows = (10 * numbers.float()[:, None] + torch.arange(2.0)).reshape(-1, 1)
        return rows.view(-1, 2, 1), rows

    def forward_both(self, x):
        assert x.dim() == 4 and x.shape[1] == 3
        self.calls.append(("forward_both", x[:, 0, 0, 0].tolist()))
        return self._rows(x[:, 0, 0, 0])

    def forward_u8(self, x, mean, std):
        from vidil_amd.video import CLIP_MEAN, CLIP_STD

        assert x.dim() == 4 and x.shape[-1] == 3 and x.dtype == torch.uint8 and (mean, std) == (CLIP_MEAN, CLIP_STD)
        self.calls.append(("forward_u8", x[:, 0, 0, 0].tolist()))
        return self._rows(x[:, 0, 0, 0])


def _numbered(B, N, u8):
    v = torch.zeros(B, N, 4, 4, 3, dtype=torch.uint8) if u8 else torch.zeros(B, N, 3, 4, 4)
    v[:, :, 0, 0, 0] = torch.arange(B * N).view(B, N).to(v.dtype)
    return v


@pytest.fixture
def on_the_host(monkeypatch):
    """frame_tokens' own refusal of host tensors switched off: what it hands to the (stub) ViT is the subject."""
    from vidil_amd import video as V

    asked = []
    monkeypatch.setattr(V, "require_cuda", lambda t, what: asked.append(what))
    return asked


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "uint8"])
def test_frame_tokens_routes_the_layouts_and_runs_in_passes(on_the_host, u8):
    from vidil_amd.video import frame_tokens

    entry, N = ("forward_u8" if u8 else "forward_both"), 3
    want = [10.0 * f + r for f in range(3 * N) for r in range(2)]
    for explicit in (None, u8):                                    # by the dtype, and as the caller says
        vit = _RecordingViT()
        rows = frame_tokens(vit, _numbered(3, N, u8), who="Head.method", u8=explicit)
        assert vit.calls == [(entry, list(range(9)))]              # videos_per_pass=None: ONE pass over all B*N frames
        assert rows.shape == (3 * N * 2, 1) and rows.view(-1).tolist() == want
    vit = _RecordingViT()
    rows = frame_tokens(vit, _numbered(3, N, u8), who="Head.method", videos_per_pass=2)
    assert vit.calls == [(entry, list(range(6))), (entry, [6, 7, 8])]          # 2N frames, then N, in order
    assert rows.view(-1).tolist() == want                                      # ... and the rows joined in order
    for per, sizes in ((1, [3, 3, 3]), (3, [9]), (16, [9])):
        vit = _RecordingViT()
        assert frame_tokens(vit, _numbered(3, N, u8), who="Head.method", videos_per_pass=per).view(-1).tolist() == want
        assert [len(c[1]) for c in vit.calls] == sizes
    assert on_the_host == ["Head.method"] * 6                                  # the host refusal speaks under the method's name


@pytest.mark.parametrize("head", HEADS)
def test_frame_tokens_refusals_keep_their_text_under_every_heads_name(on_the_host, head):
    from vidil_amd.video import frame_tokens

    vit, who = _RecordingViT(), head + ".video_tokens"
    bad_f32 = [torch.zeros(2, 3, 4, 4), torch.zeros(2, 2, 4, 4, 3), torch.zeros(2, 2, 1, 3, 4, 4)]    # rank, channel position, rank
    for x in bad_f32:
        with pytest.raises(ValueError) as e:
            frame_tokens(vit, x, who=who, u8=False)
        assert str(e.value) == f"{head}: f32 [B,N,3,S,S] expected, got {tuple(x.shape)}"
    bad_u8 = [torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 2, 3, 4, 4, dtype=torch.uint8), torch.zeros(2, 2, 4, 4, 3)]
    for x in bad_u8:                                                                                    # rank, channel position, dtype
        with pytest.raises(ValueError) as e:
            frame_tokens(vit, x, who=who, u8=True)
        assert str(e.value) == f"{head}: uint8 [B,N,S,S,3] expected, got {x.dtype} {tuple(x.shape)}"
    with pytest.raises(ValueError) as e:                           # N x T = 8193 x 2 tokens: before the ViT, on a host tensor
        frame_tokens(vit, torch.zeros(1, 1, 3, 4, 4).expand(1, 8193, 3, 4, 4), who=who)
    assert str(e.value) == (f"{head}: 16386 tokens per video (frames x tokens per frame) exceed the 16384 keys the attention kernels "
                            f"serve — sample fewer frames or build the model with a smaller image_size")
    assert not vit.calls and not on_the_host                       # every refusal came before the host check and the ViT
    frame_tokens(vit, torch.zeros(1, 8192, 3, 4, 4), who=who)      # 16,384 tokens pass
    assert len(vit.calls) == 1


def test_the_heads_still_refuse_in_their_own_words(monkeypatch):
    """The text and the type of the heads' refusals on host tensors, as they were before video.py: BLIP_Retrieval's are
    VidilHipErrors under the method's name (a host tensor first), the other two ValueErrors under the class's."""
    from vidil_amd import blip_vqa
    from vidil_amd import kernels as K
    from vidil_amd.blip import BLIP_Video_Decoder
    from vidil_amd.blip_retrieval import BLIP_Retrieval
    from vidil_amd.blip_vqa import BLIP_Video_VQA

    stub = types.SimpleNamespace(visual_encoder=_RecordingViT(), _require_plain=lambda: None, _require_image_tokens=lambda: None)
    host = "input is on cpu; the vidil_amd product path runs only on an AMD GPU through libvidil_hip.so (no CPU fallback)"
    for cls in (BLIP_Video_VQA, BLIP_Video_Decoder):
        name = cls.__name__
        with pytest.raises(ValueError) as e:
            cls.video_tokens(stub, torch.zeros(2, 2, 4, 4, 3))
        assert str(e.value) == f"{name}: f32 [B,N,3,S,S] expected, got (2, 2, 4, 4, 3)"
        with pytest.raises(ValueError) as e:
            cls.video_tokens_u8(stub, torch.zeros(2, 2, 4, 4, 3))
        assert str(e.value) == f"{name}: uint8 [B,N,S,S,3] expected, got torch.float32 (2, 2, 4, 4, 3)"
        with pytest.raises(K.VidilHipError) as e:
            cls.video_tokens(stub, torch.zeros(2, 2, 3, 4, 4))
        assert str(e.value) == f"{name}.video_tokens: {host}"
        with pytest.raises(K.VidilHipError) as e:
            cls.video_tokens_u8(stub, torch.zeros(2, 2, 4, 4, 3, dtype=torch.uint8))
        assert str(e.value) == f"{name}.video_tokens_u8: {host}"
        with pytest.raises(ValueError, match=f"^{name}: 16386 tokens per video"):
            cls._require_video_tokens(stub, 16386)
        monkeypatch.setattr(blip_vqa, "require_cuda", lambda t, what: None)     # (question_states_grouped's own, not frame_tokens')
        with pytest.raises(ValueError) as e:
            cls._check_tokens(stub, torch.zeros(7, 4), 2) if cls is BLIP_Video_Decoder else \
                cls.question_states_grouped(stub, torch.zeros(7, 4), 2, None, None, None)
        assert str(e.value) == f"{name}: 7 token rows do not divide into B=2 videos"
    with pytest.raises(K.VidilHipError) as e:
        BLIP_Retrieval.video_features(stub, torch.zeros(2, 2, 3, 4, 4))
    assert str(e.value) == f"BLIP_Retrieval.video_features: {host}"
    with pytest.raises(K.VidilHipError) as e:
        BLIP_Retrieval.video_features_u8(stub, torch.zeros(2, 2, 4, 4, 3, dtype=torch.uint8))
    assert str(e.value) == f"BLIP_Retrieval.video_features_u8: {host}"
    assert not stub.visual_encoder.calls


def test_retrievals_layout_refusals_and_no_token_bound(monkeypatch):
    """Past the host check (switched off): BLIP_Retrieval's own layout refusals, and NO token bound on its video path."""
    from vidil_amd import blip_retrieval as R
    from vidil_amd import kernels as K

    monkeypatch.setattr(R, "require_cuda", lambda t, what: None)
    stub = types.SimpleNamespace(visual_encoder=_RecordingViT(), _video_embeds=lambda y16, B, N: (B, N))
    with pytest.raises(K.VidilHipError) as e:
        R.BLIP_Retrieval.video_features(stub, torch.zeros(2, 2, 4, 4, 3))
    assert str(e.value) == "video_features: f32 [B,N,3,S,S] expected, got (2, 2, 4, 4, 3)"
    with pytest.raises(K.VidilHipError) as e:
        R.BLIP_Retrieval.video_features_u8(stub, torch.zeros(2, 3, 4, 4, dtype=torch.uint8))
    assert str(e.value) == "video_features_u8: uint8 [B,N,S,S,3] expected, got (2, 3, 4, 4)"
    assert not stub.visual_encoder.calls
    y16, shape = R.BLIP_Retrieval.video_features(stub, torch.zeros(1, 1, 3, 4, 4).expand(1, 8193, 3, 4, 4))     # 16,386 tokens
    assert y16.shape == (16386, 1) and shape == (1, 8193) and [len(c[1]) for c in stub.visual_encoder.calls] == [8193]
    y16, shape = R.BLIP_Retrieval.video_features_u8(stub, _numbered(3, 2, True))
    assert y16.view(-1).tolist() == [10.0 * f + r for f in range(6) for r in range(2)] and shape == (3, 2)
    assert stub.visual_encoder.calls[-1] == ("forward_u8", list(range(6)))                                      # one pass


# ---------------------------------------------------------------------------------------------- the rest
def test_middle_frame_is_frame_int_n_over_2_with_its_axis_kept():
    from vidil_amd.video import middle_frame

    for N in (1, 2, 3, 4, 5, 8):
        v = torch.arange(2 * N * 3).view(2, N, 3)
        m = middle_frame(v)
        assert m.shape == (2, 1, 3) and torch.equal(m[:, 0], v[:, int(N / 2)]) and torch.equal(m, v[:, N // 2:N // 2 + 1])


def test_one_definition_of_every_limit_and_the_old_homes_still_import():
    from vidil_amd import blip, blip_vqa, video, video_qa, video_retrieval

    assert video.MAX_VIDEO_TOKENS == 16384 and video.VIT_VIDEOS == 16 and video.KV_BLOCK_BYTES == 4 << 30
    assert blip.MAX_VIDEO_TOKENS is video.MAX_VIDEO_TOKENS and blip_vqa.MAX_VIDEO_TOKENS is video.MAX_VIDEO_TOKENS
    assert video_qa.VIT_VIDEOS is video.VIT_VIDEOS and video_retrieval.KV_BLOCK_BYTES is video.KV_BLOCK_BYTES
    assert video_retrieval.phase_timer is video.phase_timer and blip.CLIP_MEAN is video.CLIP_MEAN and blip.CLIP_STD is video.CLIP_STD
    assert callable(blip_vqa.video_major_order) and callable(video_retrieval.default_videos_per_block)
    assert video.phase_timer(None)() is None and video.phase_timer(None)("vit", None) is None      # no timings: no event, no wait
    for name in ("blip", "blip_vqa", "blip_retrieval", "blip_itm", "video_qa", "video_retrieval", "video_captioning"):
        assert "vidil_amd." + name not in {getattr(v, "__module__", None) for v in vars(video).values()}      # imports no head
