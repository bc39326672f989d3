"""Preconditions of tests/wide_beam_cases.py (no GPU): the selection cases cover every kind of path at 5, 8 and 16 beams and all
qualify for an exact comparison of indices; the tied cases are decided by construction; the search cases fill, displace and end
early in the oracle's own run; the oracle equals the installed transformers at the new widths; the host refuses what the kernels
do not serve before any launch."""
import ctypes

import numpy as np
import pytest

import branch_cases as bc
import wide_beam_cases as W
from oracle import beam_ref


def test_the_selection_cases_are_complete():
    shapes = W.selection_shapes()
    assert len(shapes) == len(set(shapes)) == 3 * 2 * 4 + 1
    for nb in W.NBS:
        for nbl in (1, nb):
            kinds = {W.kind_of(V) for V, n, l in shapes if (n, l) == (nb, nbl) and (V, n, l) != W.MINIMAL}
            assert kinds == set(W.KINDS), (nb, nbl, kinds)
    for V, nb, nbl in shapes:
        k = W.kind_of(V)
        assert nbl * V >= 2 * nb + 1
        if k == "ragged":
            assert V % 4 == 0 and V > 1024 and V % 1024 != 0
        if k == "empty":
            assert V % 4 == 0 and V < 1024              # threads 66.. hold nothing, waves 2 and 3 see no element (V <= 512: wave 2 too)
        if k in ("scalar", "scalar_large"):
            assert V % 4 != 0 and (V > 30000) == (k == "scalar_large")
    V, nb, nbl = W.MINIMAL
    assert (nb, nbl) == (16, 1) and 2 * nb + 1 < V * nbl <= 2 * nb + 8
    keys = W.selection_keys()
    assert len(keys) == len(shapes) * 2 * (1 + len(bc.BEAM_PENALTIES) * len(bc.BEAM_CUR_LENS))
    assert {k[4] for k in keys} == {None, 0.6, 1.3} and {k[5] for k in keys if k[4]} == {64, 1} and {k[3] for k in keys} == {False, True}


@pytest.mark.parametrize("nb", W.NBS)
def test_every_selection_case_qualifies_for_exact_indices(nb):
    """The best 2 nb + 1 reference scores of every image of every case are more than 1e-4 apart (branch_cases.beam_min_gap)."""
    worst = np.inf
    for key in W.selection_keys():
        if key[1] != nb:
            continue
        c = bc.beam_case(*key)
        gap = bc.beam_min_gap(c)
        worst = min(worst, gap)
        assert gap > 1e-4, (key, gap)
        assert c["order"].shape == (bc.BEAM_B, 2 * nb + 1)
        if c["hist"] is not None:
            h = c["hist"][:, :c["cur_len"]].numpy()
            assert c["hist"].shape == (bc.BEAM_B * nb, 64)
            if c["cur_len"] == 64:
                assert (h == -1).any() and (h == c["V"]).any()                   # ids outside [0, V) are on the list
    print(f"\nnb={nb}: smallest gap among the best {2 * nb + 1} reference scores over the cases {worst:.2e}")


@pytest.mark.parametrize("name,nb,nbl", W.TIED)
def test_tied_cases_are_decided_by_construction(name, nb, nbl):
    c = W.tied_case(name, nb, nbl)
    x = c["logits"].numpy()
    assert c["order"].shape == (W.TIED_B, 2 * nb)
    if name == "constant":
        assert len(np.unique(x)) == 1
        want = [i for i in range(2 * nb + 1) if i != c["ban"]][:2 * nb]
        assert all(c["order"][b].tolist() == want for b in range(W.TIED_B))      # row 0 of the image, lowest indices, ban left out
    else:
        assert set(np.unique(x)) == {0.0, 0.5, 1.0, 2.0} and ((x == 2.0).sum(1) == 3).all()
        assert ((x == 1.0).sum(1) > 3000).all()                                  # far more than half a wave's buffer per wave
        assert W.tied_class_gap(c) > 0.05 and c["yardstick"] < 1e-5
        for b in range(W.TIED_B):
            o = c["order"][b]
            beam, tok = o // c["V"], o % c["V"]
            lev = x[b * nbl + beam, tok]
            n2 = int((lev == 2.0).sum())
            assert n2 == min(3 * min(nbl, 4), 2 * nb) and (lev[:n2] == 2.0).all() and (lev[n2:] == 1.0).all()
            assert (beam[n2:] == 0).all() and (np.diff(tok[n2:]) > 0).all()        # then row 0's elements at 1, lowest index first


@pytest.mark.parametrize("nb", W.NBS)
def test_search_cases_fill_displace_and_end_early(nb):
    small, voc = W.search_reference("small", nb), W.search_reference("vocabulary", nb)
    c = W.SEARCH["small"]
    assert c["V"] >= 2 * nb
    assert small["displaced"] >= 1 and small["ended_early"] >= 1, small
    assert any(len(s) < c["max_length"] and s[-1] == c["eos"] for s in small["seqs"])
    assert small["min_gap"] > 1e-4 and voc["min_gap"] > 1e-4, (small["min_gap"], voc["min_gap"])
    pen = W.search_reference("small", nb, W.SEARCH_PENALTY)
    assert pen["displaced"] >= 1 and pen["ended_early"] >= 1
    assert any(a.tolist() != b.tolist() for a, b in zip(pen["seqs"], small["seqs"]))      # the penalty moves the search
    print(f"\nnb={nb}: small: {small['steps']} steps, {small['displaced']} displaced, {small['ended_early']} done verdicts before the "
          f"last step, min gap {small['min_gap']:.2e}; vocabulary: min gap {voc['min_gap']:.2e}")


@pytest.mark.parametrize("nb,max_len,min_len,eos_boost", [(5, 12, 5, 0.3), (8, 12, 6, 0.3), (5, 9, 5, 0.6), (8, 10, 5, 0.1)])
def test_oracle_equals_installed_transformers_at_5_and_8_beams(nb, max_len, min_len, eos_boost):
    """oracle/beam_ref.py rule="5.15" against generate(num_beams=...) of the installed transformers, as tests/test_beam_hf.py does
    for the narrow widths; a vocabulary of 40 so that 2 nb candidates exist on the first step."""
    pytest.importorskip("transformers")
    from oracle import hf_beam

    V, EOS, PAD = 40, 2, 7
    ended = 0
    for seed in range(6):
        fn = hf_beam.table_logits_fn(V, 300 + seed, EOS, eos_boost=eos_boost, ban=(PAD,))
        prompts = np.array([[5, 1, 3, 1]] * 3, dtype=np.int64)
        prompts[:, 1] = [1, 4, 6]
        seqs, scores = beam_ref.beam_search(lambda ids, bi: fn(ids), prompts, num_beams=nb, max_length=max_len, min_length=min_len,
                                            eos_token_id=EOS, pad_token_id=PAD, rule="5.15")
        hseqs, hscores = hf_beam.hf_generate(fn, prompts, V, num_beams=nb, max_length=max_len, min_length=min_len,
                                             eos_token_id=EOS, pad_token_id=PAD)
        for b in range(3):
            assert seqs[b].tolist() == hseqs[b].tolist(), (seed, b, seqs[b], hseqs[b])
            assert scores[b] == pytest.approx(hscores[b], rel=1e-5, abs=1e-6)
            ended += int(seqs[b][-1] == EOS)
    if eos_boost >= 0.3:
        assert ended > 0


def test_the_host_refuses_before_any_launch():
    """17 beams, and a wide launch with fewer than 2 nb candidates: refused with a message that names the numbers, from argument
    checks that run before any launch (dummy non-null pointers, no GPU touched)."""
    from vidil_amd import _lib
    from vidil_amd import kernels as K

    assert K.MAX_BEAMS == 16
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    assert lib.vidil_logsoftmax_topk(p, p, 2, 17, 17, 100, -1, p, p, None) == -3
    assert b"num_beams=17 not supported (1..16)" in lib.vidil_last_error()
    assert lib.vidil_logsoftmax_topk(p, p, 2, 16, 1, 31, -1, p, p, None) == -1
    msg = lib.vidil_last_error()
    assert b"beams_in_logits=1" in msg and b"V=31" in msg and b"2*num_beams=32" in msg
    assert lib.vidil_logsoftmax_topk_penalty(p, p, 2, 5, 5, 1, -1, p, 4, 8, 1.3, p, p, None) == -1
    msg = lib.vidil_last_error()
    assert b"beams_in_logits=5" in msg and b"V=1" in msg and b"2*num_beams=10" in msg
    # valid shapes at 5 and 16 beams, logits that are no device memory: refused by the runtime query, with or without a GPU
    for nb in (5, 16):
        assert lib.vidil_logsoftmax_topk(p, p, 2, nb, nb, 100, -1, p, p, None) == -3
        assert b"host memory is not supported" in lib.vidil_last_error()
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(K.VidilHipError, match="1..16"):
            K.require_num_beams(bad, "generate")
    for ok in (1, 4, 5, 16, np.int64(8)):
        K.require_num_beams(ok, "generate")
