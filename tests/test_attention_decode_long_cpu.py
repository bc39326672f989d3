"""The slicing constants that tests/test_attention_decode_long_gpu.py mirrors from csrc/attention.hip (attn_dsplit_kernel: NW
waves per unit, wave w owns tiles [w * n / NW, (w + 1) * n / NW)), spelled out — as CH is pinned for the long-key form."""
import os
import re

import attention_decode_long_cases as A
from common import ROOT


def test_slices_are_contiguous_balanced_and_spelled_out():
    assert A.NW == 4
    assert A.slice_tiles(769) == [(0, 6), (6, 12), (12, 18), (18, 25)]              # 25 tiles
    assert A.slice_tiles(1576) == [(0, 12), (12, 25), (25, 37), (37, 50)]           # 50 tiles: 8 frames x 197 tokens
    assert A.slice_tiles(4616) == [(0, 36), (36, 72), (72, 108), (108, 145)]        # 145 tiles: 8 frames x 577 tokens
    assert A.slice_tiles(16384) == [(0, 128), (128, 256), (256, 384), (384, 512)]
    assert A.slice_keys(1576) == [384, 800, 1184]
    for Nk in (769, 800, 1025, 1576, 4616, 9232, 16384):
        sl = A.slice_tiles(Nk)
        n = (Nk + 31) // 32
        assert sl[0][0] == 0 and sl[-1][1] == n and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        sizes = [t1 - t0 for t0, t1 in sl]
        assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 6


def test_targets_sit_on_both_sides_of_every_slice_boundary():
    assert A.targets(800) == [0, 191, 192, 193, 383, 384, 385, 575, 576, 577, 767, 768, 784, 798, 799]
    t = A.targets(1576)
    for k0 in (384, 800, 1184):
        assert {k0 - 1, k0, k0 + 1} <= set(t)
    assert {0, 767, 768, 1568, 1574, 1575} <= set(t)                                # 1568: the last (partial) 16-key block and tile


def test_the_kernel_source_launches_the_mirrored_wave_count():
    src = open(os.path.join(ROOT, "vidil_amd", "csrc", "attention.hip")).read()
    assert re.findall(r"return launch_dsplit<T, (\d+)>\(p, s\);", src) == [str(A.NW)]
    assert "const int t0 = (int)(((long long)wave * ntiles) / NW), t1 = (int)(((long long)(wave + 1) * ntiles) / NW);" in src
