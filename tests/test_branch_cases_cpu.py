"""Preconditions of tests/test_kernel_branches_gpu.py, asserted on the inputs and references of tests/branch_cases.py alone (no
GPU): that each case really has the size, tie, gap or count that sends the kernel down the branch it is named for, and that
the references are what the GPU tests take them to be."""
import numpy as np
import torch

import branch_cases as bc


# ---------------------------------------------------------------------------------------------- A. beam candidate selection
def test_beam_vocabularies_reach_the_ragged_refresh_the_empty_threads_and_the_scalar_path():
    for V in bc.BEAM_V_RAGGED:
        it, lanes = bc.beam_last_iteration(V)
        assert V % 4 == 0 and V % 1024 != 0 and it % 8 == 1 and 0 < lanes < 256, (V, it, lanes)   # ragged AND a refresh iteration
    assert bc.beam_last_iteration(1028) == (1, 1)            # exactly one lane is active
    assert bc.beam_last_iteration(1500) == (1, 119)          # wave 0 full, wave 1 partial (55 lanes), waves 2 and 3 gone
    assert bc.beam_last_iteration(2044) == (1, 255)          # wave 3 is missing one lane
    assert [bc.beam_last_iteration(V)[0] for V in (9220, 9716, 10236)] == [9, 9, 9]    # after a refresh with every lane (it = 1)
    for V in bc.BEAM_V_EMPTY:
        assert V % 4 == 0 and V // 4 < 256                   # vector path, and some threads see no element (m = -inf)
    assert 8 // 4 == 2 and 260 // 4 == 65 and 1000 // 4 == 250
    # a wave with fewer than 2 nb elements: wave 1 of V = 260 holds one thread's four, waves 1..3 of V = 8 none
    assert (260 // 4 - 64) * 4 < 2 * 3
    for V in bc.BEAM_V_SCALAR:
        assert V % 4 != 0
    assert sorted({nb for nb, _ in bc.BEAM_NB_NBL}) == [1, 2, 3, 4]
    assert all((nb, 1) in bc.BEAM_NB_NBL and (nb, nb) in bc.BEAM_NB_NBL for nb in (1, 2, 3, 4))


def test_beam_only_the_launches_without_enough_candidates_are_left_out():
    assert bc.BEAM_SKIPPED == ((8, 4, 1),)
    keys = bc.beam_case_keys()
    assert len(keys) == (len(bc.BEAM_V) * len(bc.BEAM_NB_NBL) - 1) * 2 * (1 + len(bc.BEAM_PENALTIES) * len(bc.BEAM_CUR_LENS))
    assert len(set(keys)) == len(keys)


def test_beam_reference_scores_are_more_than_1e_4_apart_in_every_case_and_image():
    worst = (np.inf, None)
    for key in bc.beam_case_keys():
        case = bc.beam_case(*key)
        nb = case["nb"]
        assert case["order"].shape == (bc.BEAM_B, 2 * nb + 1) and np.isfinite(case["ref32"]).all(), key
        gap = bc.beam_min_gap(case)
        if gap < worst[0]:
            worst = (gap, key)
        assert gap > 1e-4, (key, gap)
        assert 0.0 < case["yardstick"] < 1e-4, (key, case["yardstick"])     # far below the gaps: rounding cannot reorder them
        d = np.abs(case["ref32"].astype(np.float64) - np.take_along_axis(case["full64"], case["order"], 1)).max()
        assert d <= case["yardstick"], key
    print(f"\nsmallest gap among the best 2 nb + 1 reference scores: {worst[0]:.3e} at {worst[1]}")


def test_beam_ban_and_histories_hold_what_the_cases_are_named_for():
    for V in bc.BEAM_V:
        for nb, nbl in bc.BEAM_NB_NBL:
            if (V, nb, nbl) in bc.BEAM_SKIPPED:
                continue
            x = bc.beam_logits(V, nbl)[0].numpy()
            ban = bc.beam_ban(V, nbl)
            assert (x[0] > x[0, ban]).sum() == 1                             # the second best logit of its row
            plain = bc.beam_case(V, nb, nbl, False)
            assert ban in (plain["order"][0][:2 * nb] % V)                    # ... and a winner while it is not banned
            banned = bc.beam_case(V, nb, nbl, True)
            assert not np.isin(banned["order"][:, :2 * nb] % V, [ban]).any()
            h = bc.beam_history(V, nb, nbl, ban)
            assert h.shape == (bc.BEAM_B * nb, 64) and h.dtype == np.int32
            for b in range(bc.BEAM_B):
                for j in range(nbl):
                    row = h[b * nb + j]
                    assert row[0] == x[b * nbl + j].argmax()                  # cur_len = 1: the row's best token
                    assert -1 in row and V in row and ban in row
                    assert len(np.unique(row)) < 64                           # a repeated token (penalised once)
            # the penalty moves the selection: at cur_len = 1 each row's best token is rescored
            for pen in bc.BEAM_PENALTIES:
                moved = bc.beam_case(V, nb, nbl, False, pen, 1)
                assert not np.array_equal(moved["ref32"], plain["ref32"]), (V, nb, nbl, pen)


# ------------------------------------------------------------------------------------------------------------ B. topk_rows
def test_topk_rows_hold_the_planted_ties_and_the_short_row():
    for N in bc.TOPK_N:
        x = bc.topk_input(N)
        k = min(N, 128)
        v, i = bc.topk_ref(x, k)
        assert all((np.diff(row[np.isfinite(row)].astype(np.float64)) <= 0).all() for row in v)
        if N > 515:
            assert v[0, :3].tolist() == [9.0] * 3 and i[0, :3].tolist() == [3, 259, 515]       # one thread's stride: i % 256 == 3
            assert v[0, 3:9].tolist() == [8.5] * 6
            assert i[0, 3:9].tolist() == [5, 70, 133, 200, N - 257, N - 1]                     # lanes of all four waves
            assert sorted({(j % 256) // 64 for j in (5, 70, 133, 200)}) == [0, 1, 2, 3] and (N - 1) % 256 == (N - 257) % 256
        finite = int(np.isfinite(x[2]).sum())
        assert finite == k // 2 < max(k, 2)                                                   # fewer than k finite values
        assert np.isneginf(v[2, finite:]).all() and (i[2, finite:] == -1).all() and (i[2, :finite] >= 0).all()
    assert bc.TOPK_LDS_OPT_IN_ABOVE * 4 == 64 * 1024 and 16385 * 4 > 64 * 1024                 # the dynamic-LDS opt-in
    assert 38400 * 4 == 150 * 1024 and bc.TOPK_TOO_LONG * 4 > 150 * 1024
    assert {1, 63, 255}.issubset(bc.TOPK_N) and bc.TOPK_STRIDED_N in bc.TOPK_N                 # N < 256: threads that hold nothing


# ------------------------------------------------------------------------------------------------------------------ C. rows
def test_layernorm_rows_families_and_yardsticks():
    assert [bc.ln_family(r) for r in range(5)] == [0, 1, 2, 3, 4]
    assert sorted(bc.ln_family(r) for r in range(0, 25, 5)) == [0, 1, 2, 3, 4]                 # the strided form sees every family
    assert 1280 // 256 == 5 and set(bc.LN_D) == {256, 512, 768, 1024, 1280}
    for D in bc.LN_D:
        x, g, b = bc.ln_input(D)
        fam = np.array([bc.ln_family(m) for m in range(x.shape[0])])
        const = x[fam == 2]
        assert (const == np.float32(bc.LN_CONST)).all()
        # the constant row's sum is exact in f32 in any order (every partial sum n * 7.25 = n * 29 / 4 fits 24 bits) ...
        assert 29 * D < 2 ** 24 and np.float32(bc.LN_CONST * D) == bc.LN_CONST * D
        # ... and the f32 product with the rounded 1 / D the kernel uses gives the mean back exactly: the result is beta
        assert np.float32(np.float32(bc.LN_CONST * D) * (np.float32(1.0) / np.float32(D))) == np.float32(bc.LN_CONST)
        spikes = x[fam == 3]
        assert ((spikes == 1e4).sum(1) == 1).all() and np.sort(np.abs(spikes), 1)[:, -2].max() < 1e-2
        for eps in bc.LN_EPS:
            ref, yard = bc.ln_reference(D, eps)
            assert np.isfinite(ref).all()
            assert np.array_equal(ref[fam == 2], np.broadcast_to(b.astype(np.float64), ref[fam == 2].shape))
            assert yard[2] == 0.0 and (yard[[0, 1, 3, 4]] > 0).all() and yard.max() < 5e-3, (D, eps, yard)
            assert yard[1] > 10 * yard[0]               # the offset rows are limited by the f32 mean: no single bound fits


def test_patchify_batches_make_a_second_partial_grid_stride_pass():
    full = bc.GRID_CAP_ITEMS
    assert full == 1_048_576
    want = {"f32": 1_053_696, "u8": 1_053_696, "any": 1_146_880}
    for kernel, (ps, S, B) in bc.PATCH_BIG.items():
        n = bc.patch_items(kernel, ps, S, B)
        assert n == want[kernel] and full < n < 2 * full                     # a second pass, and a partial one
        assert bc.patch_items(kernel, ps, S, B - 1) <= full                  # ... at the smallest such batch
    assert (bc.PATCH_BIG["f32"][0] % 8, bc.PATCH_BIG["u8"][0] % 8, bc.PATCH_BIG["any"][0] % 8) == (0, 0, 6)
    for ps, S in bc.PATCH_GEOMETRIES:
        assert S % ps == 0 and bc.patch_items("any", ps, S, bc.PATCH_B) <= full
    assert bc.patch_ldk(14) == 640 > 588 and bc.patch_ldk(16) == 768 and bc.patch_ldk(32) == 3072
    t = bc.patch_u8_table()
    lo, hi = bc.patch_u8_bounds(torch.float16)
    assert t.shape == (256, 3) and (lo.double().numpy() <= t).all() and (t <= hi.double().numpy()).all()
    f32, u8 = bc.patch_images(14, 28, 1)
    rows = bc.patch_rows(f32, 14)
    assert rows.shape == (4, 640) and (rows[:, 588:] == 0).all()
    assert rows[3, 2 * 196 + 5 * 14 + 7] == f32[0, 2, 14 + 5, 14 + 7]          # patch (1, 1), channel 2, y 5, x 7
    assert torch.equal(bc.patch_u8_lookup(u8, torch.from_numpy(t), 14)[3, 196 + 3 * 14 + 1], torch.from_numpy(t)[int(u8[0, 17, 15, 1]), 1])


def test_split3_embed_and_l2_cases():
    M, D = bc.SPLIT3_BIG
    assert D % 8 == 0 and bc.GRID_CAP_ITEMS < M * (D // 4) == 1_049_088 < 2 * bc.GRID_CAP_ITEMS
    x = bc.split3_input(4, 264)
    s = bc.split3_ref(x, torch.float16)
    assert s.shape == (4, 792) and torch.equal(s[:, :264], s[:, 528:])
    assert (s[:, :264].double() + s[:, 264:528].double() - x.double()).abs().max() < 2e-6
    seen = set()
    for D in bc.EMBED_D:
        assert D % 4 == 0
        for M, T, ids in bc.EMBED_CASES:
            ids_t, word, pos, pos_off, want = bc.embed_case(D, M, T, ids)
            assert M % T == 0 and pos_off + T == pos.shape[0] == bc.EMBED_POS       # the last position row is reached
            seen |= set(ids_t.tolist())
            assert torch.equal(want[M - 1], word[min(max(int(ids_t[-1]), 0), bc.EMBED_VOCAB - 1)] + pos[-1])
            if M > 1:
                assert -5 in ids_t.tolist() and bc.EMBED_VOCAB + 3 in ids_t.tolist()
                assert torch.equal(want[0], word[0] + pos[pos_off])                     # id -5 -> row 0
                assert torch.equal(want[M // 2], word[-1] + pos[pos_off + (M // 2) % T])    # id vocab + 3 -> the last row
    assert {-5, bc.EMBED_VOCAB + 3}.issubset(seen) and {1, 30, 31} == {c[0] for c in bc.EMBED_CASES}
    assert 260 % 256 == 4                      # D = 260: the second trip of the column loop serves lane 0 alone
    for D in bc.L2_D:
        for n in bc.L2_N:
            x, ref, yard = bc.l2_case(D, n)
            assert np.allclose((ref * ref).sum(1), 1.0, rtol=0, atol=1e-12) and 0 < yard < 1e-6


# ---------------------------------------------------------------------------------------------------------------- D. resize
def test_resize_geometries_reach_the_fallback_kernels():
    from vidil_amd import preprocess

    H, W, S = bc.RESIZE_H_GENERIC
    ksize, _, _ = preprocess.axis_weights(W, S)
    assert ksize == 71 and bc.resample_h_lds_bytes(W, S, ksize) == 111_488 > 64 * 1024           # generic horizontal kernel
    k640, _, _ = preprocess.axis_weights(640, 224)
    assert bc.resample_h_lds_bytes(640, 224, k640) <= 64 * 1024                                  # (the widest frame tested so far)
    assert (bc.RESIZE_ODD_S * 3) % 4 != 0 and all((s * 3) % 4 == 0 for s in (224, 336, 384, 480))
    cap = bc.RESAMPLE_CAP_ITEMS
    assert cap == 4_194_304
    for kind, n in (("h", 4_197_600), ("v", 4_195_323), ("v4", 4_196_352)):
        assert cap < bc.resample_items(kind) == n < 2 * cap
    B, in_h, in_w, out_h, out_w = bc.RESIZE_STRIDE["h"]
    kh, _, _ = preprocess.axis_weights(in_w, out_w)
    assert bc.resample_h_lds_bytes(in_w, out_w, kh) == 67_392 > 64 * 1024 and in_h == out_h
    assert (bc.RESIZE_STRIDE["v"][4] * 3) % 4 != 0 and (bc.RESIZE_STRIDE["v4"][4] * 3) % 4 == 0
    for kind in ("v", "v4"):
        assert bc.RESIZE_STRIDE[kind][2] == bc.RESIZE_STRIDE[kind][4]                            # a vertical pass keeps the width


def test_resize_pass_reference_is_the_oracles_resize():
    """One pass of the stride cases' formula, chained horizontally then vertically with the kernel-side tables, is
    oracle/resize_ref.py's whole resize (itself pinned against Pillow by tests/test_resize_cpu.py)."""
    from oracle import resize_ref
    from vidil_amd import preprocess

    img = bc.resize_frames(1, 19, 45)[0]
    _, bh, kh = preprocess.axis_weights(45, 30)
    _, bv, kv = preprocess.axis_weights(19, 26)
    mid = resize_ref._pass(img, np.array(bh, np.int64), np.array(kh, np.int64), 1)
    out = resize_ref._pass(mid, np.array(bv, np.int64), np.array(kv, np.int64), 0)
    assert np.array_equal(out, resize_ref.resize_bicubic_u8(img, 30, 26))


# ------------------------------------------------------------------------------------------------------- E. beam_attention
def test_beam_attention_cases_sit_on_the_kernel_boundaries():
    assert [(n + 7) // 8 for n in bc.ATTN_NKEYS] == [1, 2, 4, 5, 8]           # key slots per lane group: 8/9, 32/33 (MAXJ 4 -> 8), 64
    assert max(bc.ATTN_NKEYS) == 64 < 65 <= bc.ATTN_TCAP
    for dtype in (torch.float16, torch.bfloat16):
        q, ka, va, anc, ref, f32_err = bc.attn_case(33, 2, dtype)
        assert torch.isnan(ka).any() and torch.isnan(va[33:]).all() and np.isfinite(ref).all() and 0 < f32_err < 1e-5
        assert q.dtype == dtype and anc.dtype == torch.int32 and int(anc.min()) >= 0 and int(anc.max()) < bc.ATTN_ROWS
    assert bc.ulp(1.0, torch.float16) == 2.0 ** -10 and bc.ulp(1.5, torch.bfloat16) == 2.0 ** -7
    assert bc.ulp(1e-7, torch.float16) == 2.0 ** -24 and bc.ulp(448.0, torch.float8_e4m3fn) == 32.0
