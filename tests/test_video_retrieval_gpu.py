"""Video-text retrieval evaluation (vidil_amd/video_retrieval.py) on the GPU against the fp32 oracle composed from oracle/
(tests/video_retrieval_cases.py): 5 videos of N frames at 128 x 128 (65 tokens per frame), 7 texts, k_test = 3.
N = 13: 845 keys per video, the long-key form of vidil_attention; N = 2: 130 keys, kernels that existed before it (the host
logic alone)."""
import numpy as np
import pytest
import torch

import video_retrieval_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", params=[13, 2], ids=["N13", "N2"])
def case(request, tmp_path_factory):
    """The model, the oracle's numbers and the device's evaluation for videos_per_block = 1, 2, 5 — computed once per N."""
    from vidil_amd import kernels as K
    from vidil_amd import video_retrieval as VR

    N = request.param
    m = C.small_video_retrieval(tmp_path_factory.mktemp("med"))
    u8 = C.frames(N)
    ref = C.oracle(m, u8)
    m = m.to(DEV)
    _, vid = m.video_features_u8(torch.from_numpy(u8).to(DEV))
    txt, _, _ = m.text_features(C.TEXTS, DEV)
    sims = K.scan_scores(vid, txt).cpu().numpy()
    runs = {vpb: VR.evaluation(m, [u8[:3], u8[3:]], C.TEXTS, C.K_TEST, videos_per_block=vpb) for vpb in (1, 2, 5)}
    return dict(N=N, model=m, ref=ref, vid=vid.cpu(), txt=txt.cpu(), sims=sims, runs=runs)


def test_embeddings_vs_oracle(case):
    assert (case["vid"] - case["ref"]["vid_emb"]).abs().max().item() < 2e-3
    assert (case["txt"] - case["ref"]["txt_emb"]).abs().max().item() < 2e-3


def _topk(mat, k):
    """(value desc, index asc) top-k of every row."""
    return np.lexsort((np.broadcast_to(np.arange(mat.shape[1]), mat.shape), -mat.astype(np.float64)), axis=1)[:, :k]


def test_candidates_are_the_topk_of_the_devices_own_similarities(case):
    v2t, t2v = case["runs"][5]
    sims = case["sims"]
    assert v2t.shape == (5, 7) and t2v.shape == (7, 5) and v2t.dtype == np.float32 and t2v.dtype == np.float32
    for score, mat in ((v2t, sims), (t2v, np.ascontiguousarray(sims.T))):
        want = np.zeros(mat.shape, dtype=bool)
        np.put_along_axis(want, _topk(mat, C.K_TEST), True, axis=1)
        assert np.array_equal(score != -100.0, want)
        assert (score[~want] == -100.0).all()


def test_candidate_scores_vs_oracle(case):
    v2t, t2v = case["runs"][5]
    ref = (case["ref"]["itm"] + case["ref"]["sims"]).numpy()              # [5, 7]: ITM logit of class 1 + similarity
    n = 0
    for score, want in ((v2t, ref), (t2v, ref.T)):
        cand = score != -100.0
        err = np.abs(score[cand] - want[cand])
        n += int(cand.sum())
        assert err.max() < 2e-2, (case["N"], err.max())
    assert n == 5 * C.K_TEST + 7 * C.K_TEST                               # no row skipped


def test_a_pair_scored_in_both_directions_has_one_score(case):
    v2t, t2v = case["runs"][5]
    both = (v2t != -100.0) & (t2v.T != -100.0)
    assert both.any()
    assert np.array_equal(v2t[both].view(np.uint32), np.ascontiguousarray(t2v.T)[both].view(np.uint32))


def test_results_do_not_depend_on_videos_per_block(case):
    for vpb in (1, 2):
        for a, b in zip(case["runs"][vpb], case["runs"][5]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), vpb


def test_long_keys_need_the_group_start_form(tmp_path):
    """More than 768 tokens per image with image_index (one pair's rows per unit): a VidilHipError that names group_start."""
    from vidil_amd import kernels as K

    m = C.small_video_retrieval(tmp_path).to(DEV)
    y16, _ = m.video_features_u8(torch.from_numpy(C.frames(13)[:2]).to(DEV))
    ids, lens = m.tokenize(C.TEXTS[:2])
    with pytest.raises(K.VidilHipError, match="group_start"):
        m.itm_pairs(y16, 2, ids, lens, image_index=torch.tensor([0, 1], dtype=torch.int32))


def test_video_embedding_is_the_normalised_mean_of_the_unnormalised_projections(tmp_path):
    """eval_retrieval_video.py:65-67: mean over the frames of vision_proj(cls), THEN normalise — on frames whose projections
    differ in length tenfold, where normalising first gives another vector (asserted on the oracle's two forms)."""
    u8 = C.contrast_frames()
    m = C.cancel_black_frame_(C.small_video_retrieval(tmp_path), u8)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    tokens_ref, mean_first, norm_first = C.video_embeds_ref(sd, u8)
    assert (mean_first - norm_first).abs().max(dim=-1).values.min().item() > 10 * 2e-3      # the input tells the two apart
    m = m.to(DEV)
    y16, emb = m.video_features_u8(torch.from_numpy(u8).to(DEV))
    assert tuple(emb.shape) == (2, 64) and emb.dtype == torch.float32
    assert tuple(y16.shape) == (2 * 4 * C.TOKENS, 256)
    assert (emb.cpu() - mean_first).abs().max().item() < 2e-3
    assert (y16.float().cpu().view(2, 4 * C.TOKENS, 256) - tokens_ref).abs().max().item() < 2e-2   # a video's rows are contiguous
    # the f32 entry point: same frames, normalised on the host
    from oracle import clip_ref
    x = clip_ref.preprocess_u8(u8.reshape(8, C.SIZE, C.SIZE, 3)).view(2, 4, 3, C.SIZE, C.SIZE)
    _, emb2 = m.video_features(x.to(DEV))
    assert (emb2.cpu() - mean_first).abs().max().item() < 2e-3


def test_evaluation_refuses_the_parity_mode(tmp_path):
    from vidil_amd import kernels as K
    from vidil_amd import video_retrieval as VR
    from vidil_amd.packing import set_parity_mode

    m = C.small_video_retrieval(tmp_path).to(DEV)
    set_parity_mode(True, m)
    with pytest.raises(K.VidilHipError, match="parity"):
        VR.evaluation(m, [C.frames(2)], C.TEXTS, C.K_TEST)
