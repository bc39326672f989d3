"""The host parts of vidil_amd/video_retrieval.py that need no GPU: itm_eval, the pair-union schedule, the annotation reader."""
import json

import numpy as np
import torch

from common import ROOT  # noqa: F401  (puts the repository root on sys.path)


def _scores_with_ranks(ranks, truth, n, rng):
    """A row per entry of `ranks`: distinct values, the entry truth[i] at descending rank ranks[i]."""
    out = np.empty((len(ranks), n), dtype=np.float32)
    for i, (r, t) in enumerate(zip(ranks, truth)):
        vals = np.sort(rng.permutation(n).astype(np.float32))[::-1]        # n-1 .. 0
        others = [c for c in range(n) if c != t]
        rng.shuffle(others)
        order = others[:r] + [t] + others[r:]                                # column at each descending rank
        out[i, order] = vals
    return out


def test_itm_eval_on_hand_built_matrices():
    from vidil_amd.video_retrieval import itm_eval

    rng = np.random.default_rng(0)
    n = 12
    truth = [0, 1, 2, 3, 4, 5]
    # video -> text: true match at ranks 0, 4, 5, 9, 11, 0 -> R@1 = 2/6, R@5 = 3/6, R@10 = 5/6
    v2t = _scores_with_ranks([0, 4, 5, 9, 11, 0], truth, n, rng)
    # text -> video: ranks 0, 0, 4, 5, 10 and an exact tie
    t2v = _scores_with_ranks([0, 0, 4, 5, 10, 0], truth, n, rng)
    # row 5: the true match (column 5) ties with column 9 for the best value.  np.argsort is ascending and, on 12 values, stable;
    # reversed, the HIGHER index of a tie comes first: column 9 takes rank 0 and the true match rank 1
    t2v[5] = np.arange(n, dtype=np.float32) * 0.01
    t2v[5, 5] = t2v[5, 9] = 7.0
    res = itm_eval(v2t, t2v, truth, truth)
    assert set(res) == {"txt_r1", "txt_r5", "txt_r10", "txt_r_mean", "vid_r1", "vid_r5", "vid_r10", "vid_r_mean", "vid_mdR", "r_mean"}
    assert res["txt_r1"] == 100.0 * 2 / 6 and res["txt_r5"] == 100.0 * 3 / 6 and res["txt_r10"] == 100.0 * 5 / 6
    # text -> video ranks: 0, 0, 4, 5, 10, 1 -> R@1 = 2/6, R@5 = 4/6, R@10 = 5/6; median of rank + 1 = median(1,1,5,6,11,2) = 3.5
    assert res["vid_r1"] == 100.0 * 2 / 6 and res["vid_r5"] == 100.0 * 4 / 6 and res["vid_r10"] == 100.0 * 5 / 6
    assert res["vid_mdR"] == 3.5
    assert res["txt_r_mean"] == (100.0 * 2 / 6 + 100.0 * 3 / 6 + 100.0 * 5 / 6) / 3
    assert res["vid_r_mean"] == (100.0 * 2 / 6 + 100.0 * 4 / 6 + 100.0 * 5 / 6) / 3
    assert res["r_mean"] == (res["txt_r_mean"] + res["vid_r_mean"]) / 2


def test_itm_eval_on_six_by_six_matrices():
    """6 x 6 as an evaluation of six pairs has them: ranks 0 and 4 and 5 inside the matrix (9+ needs more columns: above)."""
    from vidil_amd.video_retrieval import itm_eval

    rng = np.random.default_rng(1)
    truth = [3, 0, 5, 1, 2, 4]
    v2t = _scores_with_ranks([0, 4, 5, 0, 1, 2], truth, 6, rng)
    t2v = _scores_with_ranks([5, 5, 0, 4, 0, 3], truth, 6, rng)
    res = itm_eval(v2t, t2v, truth, truth)
    assert res["txt_r1"] == 100.0 * 2 / 6 and res["txt_r5"] == 100.0 * 5 / 6 and res["txt_r10"] == 100.0
    assert res["vid_r1"] == 100.0 * 2 / 6 and res["vid_r5"] == 100.0 * 4 / 6 and res["vid_r10"] == 100.0
    assert res["vid_mdR"] == np.median([6, 6, 1, 5, 1, 4])


def test_itm_eval_against_a_numpy_restatement():
    from vidil_amd.video_retrieval import itm_eval

    rng = np.random.default_rng(7)
    a = rng.standard_normal((50, 50)).astype(np.float32)
    b = rng.standard_normal((50, 50)).astype(np.float32)
    t2v_truth = rng.permutation(50)
    v2t_truth = rng.permutation(50)
    res = itm_eval(a, b, t2v_truth, v2t_truth)

    def ranks(m, truth):        # number of entries strictly above the true one (no ties in random floats)
        return np.array([(row > row[t]).sum() for row, t in zip(m, truth)])

    ra, rb = ranks(a, v2t_truth), ranks(b, t2v_truth)
    for key, r, k in (("txt_r1", ra, 1), ("txt_r5", ra, 5), ("txt_r10", ra, 10), ("vid_r1", rb, 1), ("vid_r5", rb, 5), ("vid_r10", rb, 10)):
        assert np.isclose(res[key], 100.0 * (r < k).mean()), key
    assert res["vid_mdR"] == np.median(rb + 1)
    assert np.isclose(res["r_mean"], (np.mean([res["txt_r1"], res["txt_r5"], res["txt_r10"]])
                                      + np.mean([res["vid_r1"], res["vid_r5"], res["vid_r10"]])) / 2)


def test_pair_union_schedule_and_scatter():
    from vidil_amd.video_retrieval import FILL, pair_union, scatter_scores

    V, Tn = 6, 9
    # video 4 lists texts but no text lists it; video 5 appears in NO list of the texts and lists texts itself ... and to have a
    # video in no candidate list at all, video 3's own row is taken out below (k differs per direction)
    idx_v2t = torch.tensor([[0, 1, 2], [2, 1, 8], [4, 5, 6], [7, 8, 0], [3, 4, 5], [6, 7, 8]])
    idx_t2v = torch.tensor([[0, 3], [0, 1], [1, 0], [4, 2], [2, 4], [2, 1], [2, 5], [5, 0], [1, 5]])
    s = pair_union(idx_v2t, idx_t2v)
    pv, pt, gs = s["pair_video"], s["pair_text"], s["group_start"]
    want = sorted({(v, int(t)) for v in range(V) for t in idx_v2t[v]} | {(int(v), t) for t in range(Tn) for v in idx_t2v[t]})
    assert list(zip(pv.tolist(), pt.tolist())) == want                     # every candidate exactly once, video-major
    assert gs.dtype == torch.int32 and gs[0] == 0 and gs[-1] == len(want)
    for v in range(V):
        assert (pv[gs[v]:gs[v + 1]] == v).all()
    assert s["max_group"] == int((gs[1:] - gs[:-1]).max())
    assert (pv[s["slot_v2t"]] == torch.arange(V)[:, None]).all() and (pt[s["slot_v2t"]] == idx_v2t).all()
    assert (pt[s["slot_t2v"]] == torch.arange(Tn)[:, None]).all() and (pv[s["slot_t2v"]] == idx_t2v).all()
    # scatter a known per-pair vector
    score = (pv * 100 + pt).to(torch.float32).numpy() + 0.5
    v2t, t2v = scatter_scores(s, score, idx_v2t.numpy(), idx_t2v.numpy(), V, Tn)
    for v in range(V):
        for t in range(Tn):
            assert v2t[v, t] == (v * 100 + t + 0.5 if t in idx_v2t[v].tolist() else FILL)
            assert t2v[t, v] == (v * 100 + t + 0.5 if v in idx_t2v[t].tolist() else FILL)
    # a video that appears in no candidate list has an empty group: only texts list videos here (a text -> video pass alone)
    s2 = pair_union(torch.empty((V, 0), dtype=torch.int64), torch.tensor([[0, 5]] * Tn))
    g2 = s2["group_start"].tolist()
    assert g2 == [0, Tn, Tn, Tn, Tn, Tn, 2 * Tn] and s2["max_group"] == Tn
    assert s2["pair_video"].tolist() == [0] * Tn + [5] * Tn and s2["pair_text"].tolist() == list(range(Tn)) * 2


def test_load_retrieval_annotations(tmp_path):
    from vidil_amd.video_retrieval import load_retrieval_annotations, pre_caption

    rows = [dict(clip_name="video7010", caption="A man is  TALKING: (loudly)!  "),
            dict(clip_name="video7011", caption=" ".join(f"w{i}" for i in range(45)) + "."),
            dict(clip_name="video7012", caption='she said "hi"; then left')]
    path = tmp_path / "ann.jsonl"
    path.write_text("\n".join(json.dumps(r) for r in rows) + "\n")
    names, texts, txt2video, video2txt = load_retrieval_annotations(str(path))
    assert names == ["video7010", "video7011", "video7012"]
    assert texts[0] == "a man is talking loudly"
    assert texts[1] == " ".join(f"w{i}" for i in range(40))                 # pre_caption(caption, 40)
    assert texts[2] == "she said hi then left"
    assert txt2video == [0, 1, 2] and video2txt == [0, 1, 2]
    assert pre_caption("One.Two", 50) == "one two"
