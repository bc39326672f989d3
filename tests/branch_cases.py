"""Inputs and references for the branch-coverage tests of the row and selection kernels (tests/test_kernel_branches_gpu.py;
preconditions asserted without a GPU by tests/test_branch_cases_cpu.py).  Everything here is numpy / torch on the CPU, in fp64
or exact integers; the sizes are the ones at which `rowops.hip`, `topk.hip`, `resample.hip`, `beam_attention.hip` and
`lsm_topk_kernel` of `beam.hip` take a branch or a loop pass that the workload's own shapes never reach.

Random inputs come from numpy's PCG64 streams (bit-identical on every host; torch's seeded CPU normal sampler is not)."""
from functools import lru_cache

import numpy as np
import torch

from oracle import resize_ref

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
GRID_CAP_ITEMS = 4096 * 256          # rowops.hip grid_for: at most 4,096 blocks of 256 threads per launch
RESAMPLE_CAP_ITEMS = 16384 * 256     # resample.hip: at most 256 * 64 blocks of 256 threads


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def ulp(a, dtype):
    """Spacing of ``dtype`` (float16 / bfloat16 / float8_e4m3fn) at magnitude |a| (float64 array), subnormal spacing below the
    smallest normal number."""
    p, emin = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float8_e4m3fn: (3, -6)}[dtype]
    a = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (e - p)


def split3_ref(x32, dtype):
    """[hi | lo | hi] with hi = T(x), lo = T(x - hi): the rows `vidil_split3_f32` and the VIDIL_DT_SPLIT3 producers write."""
    hi = x32.to(dtype)
    lo = (x32 - hi.float()).to(dtype)
    return torch.cat([hi, lo, hi], dim=-1)


# =============================================================================================== A. beam candidate selection
BEAM_B = 5
BEAM_V_RAGGED = (1028, 1500, 2044, 9220, 9716, 10236)   # vector path; the last iteration is ragged AND a refresh ((it & 7) == 1)
BEAM_V_EMPTY = (8, 260, 1000)                           # vector path; threads / waves that see no element
BEAM_V_SCALAR = (1023, 30521)                           # V % 4 != 0
BEAM_V = BEAM_V_RAGGED + BEAM_V_EMPTY + BEAM_V_SCALAR
BEAM_NB_NBL = tuple((nb, nbl) for nb in (1, 2, 3, 4) for nbl in sorted({1, nb}))
BEAM_HIST_LEN = 64                                      # MAXLEN of beam.hip: all of hs_tok
BEAM_PENALTIES = (0.6, 1.3)
BEAM_CUR_LENS = (64, 1)
# the only combinations left out: fewer than 2 nb + 1 candidates in the launch
BEAM_SKIPPED = tuple((V, nb, nbl) for V in BEAM_V for nb, nbl in BEAM_NB_NBL if nbl * V < 2 * nb + 1)
# seeds of the logits per (V, beams_in_logits), chosen so that every case below has its best 2 nb + 1 reference scores more
# than 1e-4 apart (tests/test_branch_cases_cpu.py asserts it for every case and image); 0 unless listed
BEAM_SEEDS = {(1028, 4): 2, (2044, 3): 1, (9220, 3): 1, (260, 1): 1, (260, 4): 1, (1000, 3): 2, (1000, 4): 1, (1023, 3): 1,
              (30521, 1): 1}


def beam_last_iteration(V):
    """(index of the last iteration of the vector loop `for (i = tid * 4; i < V; i += 1024)`, lanes active in it)."""
    it = (V + 1023) // 1024 - 1
    return it, (V - 1024 * it + 3) // 4


@lru_cache(maxsize=None)
def beam_logits(V, nbl):
    """f32 [B * nbl, V] logits, their f32 (torch) and fp64 log-softmax."""
    seed = BEAM_SEEDS.get((V, nbl), 0)
    x = torch.from_numpy(_rng(101, V, nbl, seed).standard_normal((BEAM_B * nbl, V), dtype=np.float32) * np.float32(2.0))
    return x, torch.log_softmax(x, -1).numpy(), torch.log_softmax(x.double(), -1).numpy()


@lru_cache(maxsize=None)
def beam_scores(nb):
    """f32 [B * nb]: image 0 starts at 0, every other beam somewhere in (-6, 0)."""
    bs = -np.abs(_rng(102, nb).standard_normal(BEAM_B * nb, dtype=np.float32)) * np.float32(1.5)
    bs[0] = 0.0
    return bs


def beam_ban(V, nbl):
    """The second best logit of image 0's first row: a token among the row's best."""
    x = beam_logits(V, nbl)[0][0].numpy()
    return int(np.argsort(-x, kind="stable")[1])


@lru_cache(maxsize=None)
def beam_history(V, nb, nbl, ban):
    """i32 [B * nb, 64] token histories of the penalty form.  Position 0 is the row's best logit (so cur_len = 1 still moves the
    selection); then the out-of-range ids -1 and V, the banned token, four of the row's twelve best logits, one of them again,
    two mid-ranked ones, and random ids of [0, V) (repeats among them at small V) up to all 64 cells of `hs_tok`."""
    x = beam_logits(V, nbl)[0].numpy()
    r = _rng(103, V, nb, nbl, ban + 1)
    h = np.zeros((BEAM_B * nb, BEAM_HIST_LEN), dtype=np.int32)
    for b in range(BEAM_B):
        for j in range(nbl):
            order = np.argsort(-x[b * nbl + j], kind="stable")
            top = order[r.permutation(min(12, V))[:4]]
            lo = min(50, V // 2)
            mid = order[lo + r.permutation(min(100, V - lo))[:2]]
            head = np.concatenate([order[:1], [-1, V, max(ban, 0)], top, top[:1], mid])
            h[b * nb + j] = np.concatenate([head, r.integers(0, V, BEAM_HIST_LEN - len(head))]).astype(np.int32)
    return h


def _best(c, n):
    """Indices of the n best entries of a 1-D score array in the order (score descending, index ascending), exactly."""
    n = min(n, c.size)
    thr = np.partition(c, c.size - n)[c.size - n]
    cand = np.nonzero(c >= thr)[0]
    return cand[np.lexsort((cand, -c[cand]))][:n]


def beam_case(V, nb, nbl, banned, penalty=None, cur_len=0):
    """One launch of `logsoftmax_topk`.  Returns a dict with the inputs, and per image: `order` (flat indices of the best 2 nb + 1
    reference scores), `ref32` (their f32 reference scores), `full64` (fp64 scores of every candidate, [B, nbl * V]) and
    `yardstick` = max |f32 reference - fp64| over the finite candidates of the case.

    Reference, as tests/test_kernels_gpu.py::test_logsoftmax_topk_on_structured_rows defines it: torch's f32 log-softmax, the
    repetition penalty `lp < 0 ? lp * p : lp / p` on each history token in [0, V) once (f32, p rounded to f32 as the C ABI
    takes it), plus the beam score, the banned token at -inf; the fp64 scores are the same chain in double precision."""
    x, lp32, lp64 = beam_logits(V, nbl)
    bs = beam_scores(nb)
    ban = beam_ban(V, nbl) if banned else -1
    lp32, lp64 = lp32.copy(), lp64.copy()
    hist = None
    if penalty is not None:
        hist = beam_history(V, nb, nbl, ban)
        p32 = np.float32(penalty)
        for b in range(BEAM_B):
            for j in range(nbl):
                t = np.unique(hist[b * nb + j, :cur_len])
                t = t[(t >= 0) & (t < V)]
                r = b * nbl + j
                s32, s64 = lp32[r, t], lp64[r, t]
                lp32[r, t] = np.where(s32 < 0, s32 * p32, s32 / p32)
                lp64[r, t] = np.where(s64 < 0, s64 * np.float64(p32), s64 / np.float64(p32))
    row_bs = bs.reshape(BEAM_B, nb)[:, :nbl].reshape(-1)
    c32 = lp32 + row_bs[:, None]
    c64 = lp64 + row_bs.astype(np.float64)[:, None]
    yardstick = float(np.abs(c32.astype(np.float64) - c64).max())
    if ban >= 0:
        c32[:, ban] = -np.inf
        c64[:, ban] = -np.inf
    c32, c64 = c32.reshape(BEAM_B, nbl * V), c64.reshape(BEAM_B, nbl * V)
    order = np.stack([_best(c32[b], 2 * nb + 1) for b in range(BEAM_B)])
    return dict(V=V, nb=nb, nbl=nbl, ban=ban, penalty=penalty, cur_len=cur_len, logits=x, beam_scores=torch.from_numpy(bs),
                hist=None if hist is None else torch.from_numpy(hist), order=order,
                ref32=np.take_along_axis(c32, order, 1), full64=c64, yardstick=yardstick)


def beam_case_keys():
    """Every (V, nb, nbl, banned, penalty, cur_len) the GPU test launches: the plain form and the penalty form."""
    keys = []
    for V in BEAM_V:
        for nb, nbl in BEAM_NB_NBL:
            if (V, nb, nbl) in BEAM_SKIPPED:
                continue
            for banned in (False, True):
                keys.append((V, nb, nbl, banned, None, 0))
                for pen in BEAM_PENALTIES:
                    for cur in BEAM_CUR_LENS:
                        keys.append((V, nb, nbl, banned, pen, cur))
    return keys


def beam_min_gap(case):
    """Smallest pairwise distance among the best 2 nb + 1 reference scores, over the images of a case."""
    s = case["ref32"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(s[:, :, None] - s[:, None, :])          # (-inf) - (-inf) = nan: two banned / missing entries never compare apart
    d[:, np.arange(s.shape[1]), np.arange(s.shape[1])] = np.inf
    return float(np.nan_to_num(d, nan=0.0).min())


# ============================================================================================================ B. topk_rows
TOPK_N = (1, 63, 255, 257, 16384, 16385, 38400)
TOPK_ROWS = 3
TOPK_STRIDED_N = 257            # this N is launched with row_stride = N + 7 as well
TOPK_LDS_OPT_IN_ABOVE = 16384   # rows of more values need > 64 KB of dynamic LDS
TOPK_TOO_LONG = 38401


@lru_cache(maxsize=None)
def topk_input(N):
    """f32 [3, N].  Row 0: exact ties planted at the top, inside one thread's stride (i, i + 256, i + 512: thread i % 256) and
    across waves (lanes 5, 70, 133, 200 of the four waves).  Row 1: plain.  Row 2: fewer than min(N, 128) finite values (all of
    them when N == 1 is impossible: the row is then -inf), so the tail of its top-k is -inf / -1."""
    x = _rng(201, N).standard_normal((TOPK_ROWS, N), dtype=np.float32)
    same_thread = [i for i in (3, 259, 515) if i < N]
    x[0, same_thread] = 9.0
    across = [i for i in (5, 70, 133, 200) if i < N]
    x[0, across] = 8.5
    if N > 300:
        x[0, [N - 1, N - 257]] = 8.5        # the last element, and its thread's previous one
    keep = _rng(202, N).permutation(N)[:min(N, 128) // 2]
    fin = np.full(N, -np.inf, dtype=np.float32)
    fin[keep] = x[2, keep]
    x[2] = fin
    return x


def topk_ref(x, k):
    """(values f32 [R, k], indices i32 [R, k]) by lexsort (value descending, index ascending); -inf entries are not winners:
    their places hold -inf / -1."""
    R, N = x.shape
    v = np.empty((R, k), np.float32)
    i = np.empty((R, k), np.int32)
    for r in range(R):
        o = np.lexsort((np.arange(N), -x[r].astype(np.float64)))[:k]
        v[r] = x[r, o]
        i[r] = np.where(np.isneginf(x[r, o]), -1, o)
    return v, i


# ================================================================================================================ C. rows
LN_D = (256, 512, 768, 1024, 1280)
LN_EPS = (1e-6, 1e-12)
LN_M = (1, 5, 333)
LN_FAMILIES = ("3*randn+0.5", "100+0.05*randn", "constant 7.25", "1e4 spike over 1e-3*randn", "1e-4*randn")
LN_CONST = 7.25
LN_PERMUTATIONS = 8


def ln_family(r):
    """Family of row r: the first five rows are one of each, and so are rows 0, 5, 10, 15, 20 (the strided form)."""
    return (r + r // 5) % 5


@lru_cache(maxsize=None)
def ln_input(D):
    """(x f32 [333, D], gamma f32 [D], beta f32 [D])."""
    r = _rng(301, D)
    M = max(LN_M)
    z = r.standard_normal((M, D), dtype=np.float32)
    x = np.empty((M, D), np.float32)
    for m in range(M):
        f = ln_family(m)
        if f == 0:
            x[m] = np.float32(3.0) * z[m] + np.float32(0.5)
        elif f == 1:
            x[m] = np.float32(100.0) + np.float32(0.05) * z[m]
        elif f == 2:
            x[m] = LN_CONST
        elif f == 3:
            x[m] = np.float32(1e-3) * z[m]
            x[m, (37 * m) % D] = 1e4
        else:
            x[m] = np.float32(1e-4) * z[m]
    g = (1.0 + 0.1 * r.standard_normal(D, dtype=np.float32)).astype(np.float32)
    b = (0.1 * r.standard_normal(D, dtype=np.float32)).astype(np.float32)
    return x, g, b


def _ln_f32(x, g, b, eps):
    """Plain numpy-f32 two-pass LayerNorm: mean, centred sum of squares, everything in f32."""
    D = np.float32(x.shape[1])
    mean = x.sum(1, dtype=np.float32, keepdims=True) / D
    d = x - mean
    var = (d * d).sum(1, dtype=np.float32, keepdims=True) / D
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    return d * rstd * g + b


@lru_cache(maxsize=None)
def ln_reference(D, eps):
    """(fp64 LayerNorm [333, D] of ln_input(D) with eps as the f32 the C ABI takes, yardstick [5]): the yardstick of a row
    family is the largest |error| against fp64 of the numpy-f32 LayerNorm over its rows and 8 column permutations (the
    identity among them) — what summation order alone is worth in f32."""
    x, g, b = ln_input(D)
    x64, e64 = x.astype(np.float64), np.float64(np.float32(eps))
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    ref = (x64 - mean) / np.sqrt(var + e64) * g.astype(np.float64) + b.astype(np.float64)
    fam = np.array([ln_family(m) for m in range(x.shape[0])])
    yard = np.zeros(len(LN_FAMILIES))
    r = _rng(302, D)
    for p in range(LN_PERMUTATIONS):
        perm = np.arange(D) if p == 0 else r.permutation(D)
        err = np.abs(_ln_f32(x[:, perm], g[perm], b[perm], eps).astype(np.float64) - ref[:, perm]).max(1)
        for f in range(len(LN_FAMILIES)):
            yard[f] = max(yard[f], err[fam == f].max())
    return ref, yard


# ---- patchify
PATCH_GEOMETRIES = ((16, 224), (32, 224), (14, 224), (14, 336), (16, 384))     # (ps, S)
PATCH_B = 2
# the smallest batches whose work items (the `total` expressions of rowops.hip) exceed one full grid of 4,096 x 256 threads, so
# the grid-stride loop makes a second, partial pass:
#   patchify_f32_kernel  total = B * G * G * 3 * ps * (ps / 8)   (16, 224): 18,816 per image  -> B =  56: 1,053,696
#   patchify_u8_kernel   total = B * G * G * ps * (ps / 8)       (16, 224):  6,272 per image  -> B = 168: 1,053,696
#   patchify_any_kernel  total = B * G * G * round_up(3 ps^2, 64) (14, 224): 163,840 per image -> B =   7: 1,146,880
PATCH_BIG = {"f32": (16, 224, 56), "u8": (16, 224, 168), "any": (14, 224, 7)}


def patch_ldk(ps):
    return (3 * ps * ps + 63) // 64 * 64


def patch_items(kernel, ps, S, B):
    G = S // ps
    if kernel == "f32":
        return B * G * G * 3 * ps * (ps // 8)
    if kernel == "u8":
        return B * G * G * ps * (ps // 8)
    return B * G * G * patch_ldk(ps)


def patch_images(ps, S, B):
    """(f32 [B, 3, S, S] image, u8 [B, S, S, 3] image)."""
    r = _rng(311, ps, S, B)
    return (torch.from_numpy(r.standard_normal((B, 3, S, S), dtype=np.float32)),
            torch.from_numpy(r.integers(0, 256, (B, S, S, 3), dtype=np.uint8)))


def patch_rows(chw, ps):
    """[B, 3, S, S] -> patch rows [B * G * G, round_up(3 ps^2, 64)] (zero padded), any dtype: a pure rearrangement."""
    B, _, S, _ = chw.shape
    G = S // ps
    rows = chw.view(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * ps * ps)
    out = torch.zeros((B * G * G, patch_ldk(ps)), dtype=chw.dtype)
    out[:, :3 * ps * ps] = rows
    return out


def patch_u8_table():
    """fp64 value of (x / 255 - mean) / std for every byte x and channel: [256, 3]."""
    x = np.arange(256, dtype=np.float64)[:, None]
    return (x / 255.0 - np.array(CLIP_MEAN, np.float64)) / np.array(CLIP_STD, np.float64)


def patch_u8_bounds(dtype):
    """(lo, hi) f32 [256, 3]: the values of ``dtype`` within one unit in the last place of the fp64 value lie in [lo, hi]."""
    t = patch_u8_table()
    u = ulp(t, dtype)
    return torch.from_numpy((t - u).astype(np.float32)), torch.from_numpy((t + u).astype(np.float32))


def patch_u8_lookup(u8, table, ps):
    """table[byte, channel] for every pixel, as patch rows (pad columns 0)."""
    B, S, _, _ = u8.shape
    chw = torch.stack([table[:, c][u8[..., c].long()] for c in range(3)], dim=1)
    return patch_rows(chw, ps)


# ---- split3
SPLIT3_D = (8, 264, 768, 3072)
SPLIT3_M = 37
SPLIT3_BIG = (1366, 3072)        # 1,049,088 float4s: 512 more than one full grid of 4,096 x 256 threads


def split3_input(M, D):
    """f32 [M, D]: 3 * randn, with every 7th column scaled into the f16 subnormal range."""
    x = _rng(321, M, D).standard_normal((M, D), dtype=np.float32) * np.float32(3.0)
    x[:, ::7] *= np.float32(1e-6)
    return torch.from_numpy(x)


# ---- embed_tokens
EMBED_D = (256, 260, 512, 1024)
EMBED_VOCAB, EMBED_POS = 50, 40
EMBED_CASES = ((1, 1, (-5,)), (1, 1, (EMBED_VOCAB + 3,)), (30, 5, None), (31, 31, None))      # (M, T, ids or None)


def embed_case(D, M, T, ids):
    """(ids i32 [M], word f32 [vocab, D], pos f32 [P, D], pos_off, expected f32 [M, D]): ids below 0 / at or past the vocabulary
    are clamped to 0 / vocab - 1, and pos_off + T is the position table's last row + 1."""
    r = _rng(331, D, M)
    word = r.standard_normal((EMBED_VOCAB, D), dtype=np.float32)
    pos = r.standard_normal((EMBED_POS, D), dtype=np.float32)
    if ids is None:
        ids = r.integers(0, EMBED_VOCAB, M)
        ids[[0, M // 2, M - 1]] = [-5, EMBED_VOCAB + 3, EMBED_VOCAB - 1]
    ids = np.asarray(ids, dtype=np.int32)
    pos_off = EMBED_POS - T
    want = word[np.clip(ids, 0, EMBED_VOCAB - 1)] + pos[pos_off + np.arange(M) % T]
    return torch.from_numpy(ids), torch.from_numpy(word), torch.from_numpy(pos), pos_off, torch.from_numpy(want)


# ---- l2_normalize_rows
L2_D = (256, 260, 512, 768)
L2_N = (1, 9)


def l2_case(D, n):
    """(x f32 [n, D], fp64 x / ||x||, yardstick = max |numpy-f32 x / ||x|| - fp64|)."""
    x = _rng(341, D, n).standard_normal((n, D), dtype=np.float32)
    x64 = x.astype(np.float64)
    ref = x64 / np.sqrt((x64 * x64).sum(1, keepdims=True))
    f32 = x / np.sqrt((x * x).sum(1, dtype=np.float32, keepdims=True), dtype=np.float32)
    return torch.from_numpy(x), ref, float(np.abs(f32.astype(np.float64) - ref).max())


# ========================================================================================================== D. resize
RESIZE_H_GENERIC = (8, 3840, 224)       # (H, W, S): blip_frames of an 8 x 3840 frame to 224 x 224
RESIZE_ODD_S = 225                      # out_w * 3 = 675 is no multiple of 4: the byte-wise vertical kernel
RESIZE_ODD_FRAMES = ((37, 53), (300, 260))
# grid-stride geometries, one pass each, (B, in_h, in_w, out_h, out_w); items = output bytes (words for v4)
RESIZE_STRIDE = {
    "h": (1, 583, 16, 583, 2400),       # LDS need 67,392 B > 64 KB -> generic horizontal kernel; 4,197,600 bytes
    "v": (1, 8, 1023, 1367, 1023),      # 3,069-byte rows -> byte-wise vertical kernel; 4,195,323 bytes
    "v4": (1, 8, 1024, 5464, 1024),     # 768-word rows -> four-byte vertical kernel; 4,196,352 words
}


def resample_h_lds_bytes(in_w, out_w, ksize):
    """LDS need of the tiled horizontal kernel, restated from `vidil_resample_u8` (HR = 4 staged rows of in_w * 3 bytes rounded
    up to 4, the weight table, the bounds table); above 64 KB the generic kernel runs."""
    return 4 * ((in_w * 3 + 3) & ~3) + out_w * ksize * 4 + out_w * 8


def resize_frames(N, H, W, seed=0):
    return _rng(401, H, W, seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def resize_stride_case(kind):
    """(src u8 [B, in_h, in_w, 3], bounds i32 [n, 2], coeffs i32 [n, ksize], vertical, expected u8): one pass of
    clip8((2^21 + sum p * k) >> 22) in numpy int64, tables from vidil_amd.preprocess.axis_weights."""
    from vidil_amd import preprocess

    B, in_h, in_w, out_h, out_w = RESIZE_STRIDE[kind]
    vertical = kind != "h"
    _, bounds, coeffs = preprocess.axis_weights(in_h, out_h) if vertical else preprocess.axis_weights(in_w, out_w)
    bounds, coeffs = np.array(bounds, np.int64), np.array(coeffs, np.int64)
    src = resize_frames(B, in_h, in_w, seed=1)
    want = np.stack([resize_ref._pass(f, bounds, coeffs, 0 if vertical else 1) for f in src])
    return src, bounds.astype(np.int32), coeffs.astype(np.int32), vertical, want


def resample_items(kind):
    B, _, _, out_h, out_w = RESIZE_STRIDE[kind]
    n = B * out_h * out_w * 3
    return n // 4 if kind == "v4" else n


# ================================================================================================== E. beam_attention
ATTN_ROWS = 5
ATTN_NKEYS = (8, 9, 32, 33, 64)
ATTN_H = (2, 12)
ATTN_TCAP = 70                  # > 65, so that n_keys = 65 is refused for the kernel's limit and not for the table's


def attn_case(n_keys, H, dtype):
    """q T [rows, H*64] (already scaled by 1/8), K / V arenas T [Tcap, rows, H*64] with NaN in every cell no ancestry entry
    names, anc i32 [rows, Tcap]; ref fp64 [rows, H*64] = softmax attention of those 16-bit values; f32_err = max |error| of the
    same computation in torch f32."""
    rows, C, Tcap = ATTN_ROWS, H * 64, ATTN_TCAP
    r = _rng(501, n_keys, H)
    q = torch.from_numpy(r.standard_normal((rows, C), dtype=np.float32) * np.float32(0.125)).to(dtype)
    anc = torch.from_numpy(r.integers(0, rows, (rows, Tcap)).astype(np.int32))
    used = torch.zeros(Tcap, rows, dtype=torch.bool)
    t = torch.arange(n_keys)
    used[t[None, :].expand(rows, -1), anc[:, :n_keys].long()] = True
    ka = torch.full((Tcap, rows, C), float("nan"), dtype=dtype)
    va = torch.full((Tcap, rows, C), float("nan"), dtype=dtype)
    n = int(used.sum())
    ka[used] = torch.from_numpy(r.standard_normal((n, C), dtype=np.float32)).to(dtype)
    va[used] = torch.from_numpy(r.standard_normal((n, C), dtype=np.float32)).to(dtype)

    def attend(ft):
        kg = ka[t[None, :], anc[:, :n_keys].long()].to(ft).view(rows, n_keys, H, 64)
        vg = va[t[None, :], anc[:, :n_keys].long()].to(ft).view(rows, n_keys, H, 64)
        s = torch.einsum("rhd,rthd->rht", q.to(ft).view(rows, H, 64), kg)
        return torch.einsum("rht,rthd->rhd", torch.softmax(s, dim=-1), vg).reshape(rows, C)

    ref = attend(torch.float64)
    f32_err = (attend(torch.float32).double() - ref).abs().max().item()
    return q, ka, va, anc, ref.numpy(), f32_err
