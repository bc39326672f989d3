"""Inputs and references for beam searches of 5..16 beams (tests/test_wide_beam_cpu.py asserts their preconditions without a GPU,
tests/test_wide_beam_gpu.py runs them on `lsm_topk_wide_kernel` / `beam_update_wide_kernel` of beam.hip and the generators).

A. Selection cases: `branch_cases.beam_case(V, nb, nbl, banned, penalty, cur_len)` — fp64 references for any nb — at nb 5, 8, 16,
   beams_in_logits 1 and nb, one V per kind of path.  The project compares indices exactly only where the best 2 nb + 1 reference
   scores of every image are more than 1e-4 apart; with seed 0 of branch_cases that does not hold for every form (plain, banned,
   both penalties, both history lengths) at V = 9716 / 1023 / 30521 / 260 and every width, so SELECT_V names, per (kind, nb,
   nbl), the first V of the same kind for which it does (found by search; asserted by the CPU test).
B. Tied rows (own logits): rows of a few logit LEVELS and constant rows.  More than half of a wave's buffer then lies within the
   margin of its K-th best logit, which is the kernel's strict form; equal logits of a row have equal scores, so the expected
   order is exact: (level descending, index ascending) inside a row, rows apart by far more than any rounding.
C. Search cases: seeded table language models keyed by (length, last two tokens, image) — every row drawn from a generator seeded by
   its key, so the table does not depend on who asks first — at V = 30524 and at V = 64 with [SEP] boosted from length 7 on, where
   the hypothesis set fills, displaces entries and fires `done`."""
import contextlib
from functools import lru_cache

import numpy as np
import torch

import branch_cases as bc
from oracle import beam_ref

NBS = (5, 8, 16)
KINDS = ("ragged", "scalar", "scalar_large", "empty")
#   ragged        V % 4 == 0, V > 1024, V % 1024 != 0: 16-byte loads, a last pass that some lanes and waves sit out
#   scalar        V % 4 != 0: one logit per lane and pass
#   scalar_large  the same at the vocabulary's size
#   empty         V % 4 == 0, V < 1024: threads and whole waves see no element
SELECT_V = {
    ("ragged", 5, 1): 9716, ("scalar", 5, 1): 1023, ("scalar_large", 5, 1): 30521, ("empty", 5, 1): 264,
    ("ragged", 5, 5): 9716, ("scalar", 5, 5): 1023, ("scalar_large", 5, 5): 30521, ("empty", 5, 5): 264,
    ("ragged", 8, 1): 9716, ("scalar", 8, 1): 1023, ("scalar_large", 8, 1): 30521, ("empty", 8, 1): 264,
    ("ragged", 8, 8): 9716, ("scalar", 8, 8): 1023, ("scalar_large", 8, 8): 30521, ("empty", 8, 8): 276,
    ("ragged", 16, 1): 9732, ("scalar", 16, 1): 1025, ("scalar_large", 16, 1): 30525, ("empty", 16, 1): 264,
    ("ragged", 16, 16): 9960, ("scalar", 16, 16): 1031, ("scalar_large", 16, 16): 30526, ("empty", 16, 16): 304,
}
MINIMAL = (40, 16, 1)            # (V, nb, nbl): 40 candidates for 2 nb + 1 = 33 places


def kind_of(V):
    if V % 4:
        return "scalar_large" if V > 30000 else "scalar"
    return "empty" if V < 1024 else "ragged"


def selection_shapes():
    """Every (V, nb, nbl) of part A."""
    return [(SELECT_V[(kind, nb, nbl)], nb, nbl) for nb in NBS for nbl in (1, nb) for kind in KINDS] + [MINIMAL]


def selection_keys(shapes=None):
    """Every (V, nb, nbl, banned, penalty, cur_len) the GPU test launches: the plain form and the penalty form, as
    branch_cases.beam_case_keys does for the narrow widths."""
    keys = []
    for V, nb, nbl in (selection_shapes() if shapes is None else shapes):
        for banned in (False, True):
            keys.append((V, nb, nbl, banned, None, 0))
            for pen in bc.BEAM_PENALTIES:
                for cur in bc.BEAM_CUR_LENS:
                    keys.append((V, nb, nbl, banned, pen, cur))
    return keys


# ===================================================================================================== B. tied rows
TIED = tuple((name, nb, nbl) for name in ("levels", "constant") for nb in NBS for nbl in (1, nb))
TIED_V = {"levels": 9716, "constant": 2044}
TIED_B = 3


@lru_cache(maxsize=None)
def tied_case(name, nb, nbl):
    """dict(logits f32 [B * nbl, V], beam_scores f32 [B * nb], ban, order i64 [B, 2 nb], full64 [B, nbl * V], yardstick).

    levels: every logit is 0, 0.5 or 1 (a third each), and three elements per row are 2.  Beam j starts at -0.3 j, so the classes
    of the image are apart by at least 0.1 while the rows' log-sum-exps differ by ~1e-2: the best 2 nb are the 2-elements of rows
    0..3 (scores 2, 1.7, 1.4, 1.1 - lse), then the lowest indices of row 0's ~3,200 elements at 1.  constant: all logits 0.25,
    one row per image counts: the lowest indices of row 0, the banned index 1 left out."""
    V, B = TIED_V[name], TIED_B
    r = bc._rng(601, nb, nbl, len(name))
    if name == "levels":
        x = r.integers(0, 3, (B * nbl, V)).astype(np.float32) * np.float32(0.5)
        for row in x:
            row[r.permutation(V)[:3]] = 2.0
        ban = -1
    else:
        x = np.full((B * nbl, V), 0.25, dtype=np.float32)
        ban = 1
    bs = np.tile(-np.float32(0.3) * np.arange(nb, dtype=np.float32), B)
    xt = torch.from_numpy(x)
    lp32 = torch.log_softmax(xt, -1).numpy()
    lp64 = torch.log_softmax(xt.double(), -1).numpy()
    row_bs = bs.reshape(B, nb)[:, :nbl].reshape(-1)
    c32, c64 = lp32 + row_bs[:, None], lp64 + row_bs.astype(np.float64)[:, None]
    yardstick = float(np.abs(c32.astype(np.float64) - c64).max())
    if ban >= 0:
        c64[:, ban] = -np.inf
    c64 = c64.reshape(B, nbl * V)
    # exact expected order from the construction: (row's class score descending, flat index ascending); fp64 scores of equal
    # logits of a row are equal bit for bit, so a lexsort of them IS that order
    order = np.stack([np.lexsort((np.arange(nbl * V), -c64[b]))[:2 * nb] for b in range(B)])
    return dict(V=V, nb=nb, nbl=nbl, ban=ban, logits=xt, beam_scores=torch.from_numpy(bs), order=order, full64=c64,
                yardstick=yardstick)


def tied_class_gap(case):
    """Smallest distance between two DIFFERENT fp64 scores among an image's best 2 nb + 1."""
    g = np.inf
    for b in range(case["full64"].shape[0]):
        s = np.sort(case["full64"][b])[::-1][:2 * case["nb"] + 1]
        d = -np.diff(s)
        g = min(g, d[d > 0].min() if (d > 0).any() else np.inf)
    return float(g)


# ================================================================================================== C. search cases
SEARCH = {
    # [SEP] competitive from length 6 on, as tests/test_models_gpu.py::test_device_beam_search_random_tables_match_oracle has it
    "vocabulary": dict(V=30524, B=3, max_length=9, min_length=5, eos=102, pad=0, prompt=(30522, 1037, 3861, 1997), scale=3.0,
                       eos_from=6, eos_boost=6.0, repeat_boost=4.0),
    # a small vocabulary whose [SEP] is among every row's best from length 7 on: hypotheses are banked at every step
    "small": dict(V=64, B=3, max_length=16, min_length=5, eos=2, pad=0, prompt=(5, 1, 3, 1), scale=3.0, eos_from=7, eos_boost=7.0,
                  repeat_boost=4.0),
}
# seeds chosen so that, in the oracle's plain search, neighbours among the best 2 nb + 1 scores of every searching image are more
# than 1e-4 apart at every step (the project's condition for comparing ids exactly), and so that the small case displaces and ends
# early at every width; tests/test_wide_beam_cpu.py asserts both
SEARCH_SEEDS = {("vocabulary", 5): 0, ("vocabulary", 8): 3, ("vocabulary", 16): 4, ("small", 5): 0, ("small", 8): 3, ("small", 16): 1}
SEARCH_PENALTY = 1.3


def search_prompt(name):
    c = SEARCH[name]
    p = np.array([c["prompt"]] * c["B"], dtype=np.int64)
    p[:, 1] += np.arange(c["B"])                              # distinct contexts per image
    return p


def table_logits_fn(name, nb):
    """ids i64 [rows, cur_len] -> f32 [rows, V]: the row of (cur_len, last token, the one before, the image's prompt token), drawn
    on first use from a generator seeded by that key; every token the sequence already holds is raised by `repeat_boost`."""
    c = SEARCH[name]
    seed = SEARCH_SEEDS[(name, nb)]
    rows = {}

    def fn(ids):
        ids = np.asarray(ids)
        cur = ids.shape[1]
        out = np.empty((ids.shape[0], c["V"]), dtype=np.float32)
        for r in range(ids.shape[0]):
            key = (cur, int(ids[r, -1]), int(ids[r, -2]), int(ids[r, 1]))   # (ids[r, 1]: the image's own prompt token)
            if key not in rows:
                row = bc._rng(701, seed, nb, c["V"], *key).standard_normal(c["V"], dtype=np.float32) * np.float32(c["scale"])
                if cur >= c["eos_from"]:
                    row[c["eos"]] += np.float32(c["eos_boost"])
                rows[key] = row
            out[r] = rows[key]
            out[r, ids[r]] += np.float32(c["repeat_boost"])      # what the row already holds is attractive: the penalty decides
        return out

    return fn


@contextlib.contextmanager
def _watch_hypotheses(events):
    """Counts, inside oracle/beam_ref.py's own BeamHypotheses, the entries displaced from a full set and the lengths at which
    an image's set was found complete (`done`)."""
    add, is_done = beam_ref.BeamHypotheses.add, beam_ref.BeamHypotheses.is_done

    def add_(self, hyp, sum_logprobs, norm_len=None):
        full = len(self) == self.num_beams
        before = [id(t) for _, t in self.beams]
        add(self, hyp, sum_logprobs, norm_len)
        if full and [id(t) for _, t in self.beams] != before:
            events["displaced"] += 1

    def is_done_(self, best_sum_logprobs, cur_len):
        d = is_done(self, best_sum_logprobs, cur_len)
        if d:
            events["done_at"].append(cur_len)
        return d

    beam_ref.BeamHypotheses.add, beam_ref.BeamHypotheses.is_done = add_, is_done_
    try:
        yield
    finally:
        beam_ref.BeamHypotheses.add, beam_ref.BeamHypotheses.is_done = add, is_done


@lru_cache(maxsize=None)
def search_reference(name, nb, penalty=1.0):
    """oracle/beam_ref.py's search (4.15 rule) on the case: dict(seqs, scores, steps, displaced, ended_early, min_gap).
    `ended_early`: `done` verdicts before the last step.  `min_gap` (plain searches only): the smallest distance between neighbours among the best 2 nb + 1 scores of any image at any step, from the
    oracle's own trace — the margin the f32 roundings of a second implementation have."""
    c = SEARCH[name]
    fn = table_logits_fn(name, nb)
    events, trace = dict(displaced=0, done_at=[]), []
    with _watch_hypotheses(events):
        seqs, scores = beam_ref.beam_search(lambda ids, bi: fn(ids), search_prompt(name), num_beams=nb, max_length=c["max_length"],
                                            min_length=c["min_length"], eos_token_id=c["eos"], pad_token_id=c["pad"], trace=trace,
                                            repetition_penalty=penalty)
    gap = np.inf
    if penalty == 1.0:
        for t in trace:
            s = beam_ref.log_softmax_rows(t["logits"])
            if t["cur_len"] < c["min_length"]:
                s[:, c["eos"]] = -np.inf
            s = (s + t["beam_scores"][:, None]).reshape(c["B"], nb * c["V"]).astype(np.float64)
            top = -np.sort(-s, axis=1)[:, :2 * nb + 1]
            top = top[:, np.isfinite(top).all(0) & (top > -1e8).all(0)]          # (first step: beams 1.. start at -1e9)
            top = top[(t["beam_scores"].reshape(c["B"], nb) != 0).any(1)]        # (a finished image is padded out: all beams 0)
            if top.shape[1] > 1:
                gap = min(gap, float((-np.diff(top, axis=1)).min()))
    return dict(seqs=seqs, scores=scores, steps=len(trace), displaced=events["displaced"],
                ended_early=sum(cl + 1 < c["max_length"] for cl in events["done_at"]), min_gap=gap)
