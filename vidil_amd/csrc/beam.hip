// beam.hip — device-side beam search bookkeeping so a whole caption batch
// decodes without a host round trip per step.  Semantics follow HF
// transformers 4.15 (generation_utils.beam_search + BeamSearchScorer +
// MinLengthLogitsProcessor), the version models/med.py:7-8 of the reference
// names; the reference call site is models/blip.py:154-161.
//
//   logsoftmax_topk : one workgroup per image; log-softmax of its nb rows (one
//                     pass per row: online max / sum of exponentials),
//                     optional EOS ban, + beam score, sorted top-2nb over
//                     nb*V candidates (ties -> lower flat index).
//                     nb 1..4: lsm_topk_kernel<NB, RP>, sorted candidate lists in
//                     registers.  nb 5..16: lsm_topk_wide_kernel<RP>, a streaming
//                     selection through a per-wave LDS buffer (same contract,
//                     nb a run-time argument).
//   beam_update     : BeamSearchScorer.process + the input_ids gather/append; one
//                     thread per image for nb <= 4, one wave per image (lane 0
//                     keeps the books, 64 lanes copy the tokens) for nb 5..16.
//   beam_finalize   : one thread per image; BeamSearchScorer.finalize.
#include <math.h>
#include "common.h"

namespace {

constexpr int MAXNB = 4;        // widest search of the register-list selection kernel and the thread-per-image update
constexpr int MAXNB_WIDE = 16;  // widest search at all
constexpr int MAXLEN = 64;

struct Cand {
  float s;
  int i;
};
__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) {
  return s1 > s2 || (s1 == s2 && i1 < i2);
}
__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s = __shfl_xor(c.s, o, 64);
    const int i = __shfl_xor(c.i, o, 64);
    if (better(s, i, c.s, c.i)) { c.s = s; c.i = i; }
  }
  return c;
}

__device__ float block_reduce_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ float block_reduce_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// RP: the repetition penalty of `generate(..., repetition_penalty != 1.0)` with beam search (reference: models/blip.py:161
// passes it to HF generate, whose RepetitionPenaltyLogitsProcessor runs FIRST in the processor list and, in beam search, on the
// LOG-PROBABILITIES: every token already in a row's sequence — prompt included — gets `s < 0 ? s * penalty : s / penalty`; oracle:
// oracle/beam_ref.py, pinned against the installed transformers by tests/test_beam_hf.py).  The row's history tokens are kept
// out of the raw-logit candidates (a penalty < 1 RAISES their score, so "best logits = best scores" does not hold for them)
// and are scored one per thread once the row's log-sum-exp is known.
template <int NB, bool RP>
__global__ __launch_bounds__(256) void lsm_topk_kernel(const float* __restrict__ logits,
                                                       const float* __restrict__ beam_scores, int NBL, int V,
                                                       int ban, float* __restrict__ out_s, int* __restrict__ out_i,
                                                       const int32_t* __restrict__ hist, int hist_len, int ld_hist,
                                                       float penalty) {
  constexpr int K = 2 * NB;
  __shared__ float red[4];
  __shared__ int hs_tok[MAXLEN];
  __shared__ float ls[256 * K];
  __shared__ int li[256 * K];
  __shared__ Cand wbest[4];
  const int b = blockIdx.x, tid = threadIdx.x;

  float ts[K];
  int ti[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { ts[j] = -INFINITY; ti[j] = 0x7fffffff; }

  const bool vec = (V & 3) == 0;   // rows are then 16-B aligned: 4 logits per load
  auto consider = [&](float c, int flat) {
    if (better(c, flat, ts[K - 1], ti[K - 1])) {
      ts[K - 1] = c; ti[K - 1] = flat;
#pragma unroll
      for (int j = K - 1; j > 0; --j) {
        if (better(ts[j], ti[j], ts[j - 1], ti[j - 1])) {
          const float s = ts[j]; ts[j] = ts[j - 1]; ts[j - 1] = s;
          const int x = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = x;
        }
      }
    }
  };
  // ONE pass over the logits per row (round 4; the round-1 form read every row three times: max, sum of exponentials,
  // candidates — 3.68 GB instead of 1.31 GB per launch at 10,752 x 30,524): every thread keeps an ONLINE softmax state
  // (running maximum m, sum of exp(x - m), rescaled when the maximum moves) and its K best RAW logits of the row; the
  // block then combines the states into the row's (max, log-sum-exp), and only the K survivors per thread are turned into
  // scores `(x - max) - lse + beam_score` and merged into the thread's candidates of the image.  log_softmax is monotone
  // in x, so a row's best scores are its best logits (ties in the rounded score are ordered by the final merge, which
  // compares (score, flat index) exactly as before).
  constexpr float L2E = 1.4426950408889634f;
  for (int beam = 0; beam < NBL; ++beam) {
    const float* row = logits + ((size_t)b * NBL + beam) * V;
    if (RP) {
      __syncthreads();                                   // (the previous row's readers are done)
      if (tid < hist_len) hs_tok[tid] = hist[((size_t)b * NB + beam) * ld_hist + tid];
      __syncthreads();
    }
    auto in_hist = [&](int t) {
      bool f = false;
      for (int h = 0; h < hist_len; ++h) f |= hs_tok[h] == t;
      return f;
    };
    float m = -INFINITY, sum = 0.f;
    float rs[K];
    int ri[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { rs[j] = -INFINITY; ri[j] = 0x7fffffff; }
    auto consider_raw = [&](float x, int i) {
      if (better(x, i, rs[K - 1], ri[K - 1])) {
        rs[K - 1] = x; ri[K - 1] = i;
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
          if (better(rs[j], ri[j], rs[j - 1], ri[j - 1])) {
            const float t = rs[j]; rs[j] = rs[j - 1]; rs[j - 1] = t;
            const int x_ = ri[j]; ri[j] = ri[j - 1]; ri[j - 1] = x_;
          }
        }
      }
    };
    if (vec) {
      // Candidate filter (second half of round 4).  A thread sees ~120 logits of a row, so some lane of a wave has a new
      // personal best at nearly every element and the (divergent) sorted insertion ran for all of them: ~200 instructions
      // per 16-byte load, the kernel's bound (2.9 TB/s).  `thr` is a wave-uniform LOWER bound of the row's K-th best logit
      // — the K-th largest of the lanes' current best candidates, which are K distinct elements of the row — minus a margin
      // far wider than any pair of logits whose rounded scores could tie: an element below it cannot be among the row's K
      // best in the (score, index) order of the final merge, so skipping it changes no output (same digests, 459 -> 347 us;
      // the bound re-derived every 2 / 4 / 8 / 16 loads: 430 / 360 / 347 / 358 us; four loads per thread issued ahead of
      // their use on top of it: 374 us — slower, left out).
      float thr = -INFINITY;
      int it = 0;
      for (int i = tid * 4; i < V; i += 1024, ++it) {
        const f32x4 x = *(const f32x4*)(row + i);
        const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        if (mx > m) {                                   // (m = -inf at first: sum = 0 * 2^-inf = 0)
          sum *= __builtin_amdgcn_exp2f((m - mx) * L2E);
          m = mx;
        }
        const float ml = m * L2E;
        sum += (__builtin_amdgcn_exp2f(__builtin_fmaf(x[0], L2E, -ml)) + __builtin_amdgcn_exp2f(__builtin_fmaf(x[1], L2E, -ml))) +
               (__builtin_amdgcn_exp2f(__builtin_fmaf(x[2], L2E, -ml)) + __builtin_amdgcn_exp2f(__builtin_fmaf(x[3], L2E, -ml)));
        if (__builtin_amdgcn_ballot_w64(mx >= thr) != 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (i + e != ban && x[e] >= thr && !(RP && in_hist(i + e))) consider_raw(x[e], i + e);  // (the banned token counts in the softmax, never as a candidate)
        }
        // (the refresh shuffles across the wave, so it runs only while EVERY lane is still inside the loop — on the
        //  ragged last iteration of a vocabulary that is not a multiple of 1,024 some lanes have left, their registers are
        //  undefined to a shuffle, and a bound derived from them could exceed real logits)
        if ((it & 7) == 1 && __builtin_amdgcn_ballot_w64(true) == ~0ull) {
          float c = rs[0], t = -INFINITY;
#pragma unroll
          for (int r = 0; r < K; ++r) {
            t = wave_max(c);
            const unsigned long long holders = __builtin_amdgcn_ballot_w64(c == t);
            if (holders == 0) break;                     // (NaNs: leave the bound where it is)
            if ((int)(threadIdx.x & 63) == __builtin_ctzll(holders)) c = -INFINITY;   // one holder leaves per round
          }
          const float bound = t - 1e-5f * (fabsf(t) + 64.f);
          if (bound > thr) thr = bound;                  // (t = -inf while the wave has seen fewer than K elements)
        }
      }
    } else {
      for (int i = tid; i < V; i += 256) {
        const float x = row[i];
        if (x > m) {
          sum *= __builtin_amdgcn_exp2f((m - x) * L2E);
          m = x;
        }
        sum += __builtin_amdgcn_exp2f((x - m) * L2E);
        if (i != ban && !(RP && in_hist(i))) consider_raw(x, i);
      }
    }
    const float M = block_reduce_max(m, red);
    // (a thread that saw no element has m = -inf, sum = 0: contributes 0)
    sum = block_reduce_sum(m == -INFINITY ? 0.f : sum * __builtin_amdgcn_exp2f((m - M) * L2E), red);
    const float lse = logf(sum);
    const float bs = beam_scores[b * NB + beam];
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (ri[j] != 0x7fffffff) consider((rs[j] - M) - lse + bs, beam * V + ri[j]);
    if (RP && tid < hist_len) {
      const int t = hs_tok[tid];
      bool first = t >= 0 && t < V && t != ban;          // (scatter_ of equal values: a repeated token is penalised once)
      for (int h = 0; h < tid; ++h) first &= hs_tok[h] != t;
      if (first) {
        const float lp = (row[t] - M) - lse;
        consider((lp < 0.f ? lp * penalty : lp / penalty) + bs, beam * V + t);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) { ls[tid * K + j] = ts[j]; li[tid * K + j] = ti[j]; }
  __syncthreads();
  int head = 0;
  for (int round = 0; round < K; ++round) {
    Cand c;
    c.s = head < K ? ls[tid * K + head] : -INFINITY;
    c.i = head < K ? li[tid * K + head] : 0x7fffffff;
    c = wave_best(c);
    if ((tid & 63) == 0) wbest[tid >> 6] = c;
    __syncthreads();
    Cand g = wbest[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (better(wbest[w].s, wbest[w].i, g.s, g.i)) g = wbest[w];
    if (head < K && li[tid * K + head] == g.i) ++head;  // flat indices are unique
    if (tid == 0) { out_s[b * K + round] = g.s; out_i[b * K + round] = g.i; }
    __syncthreads();
  }
}

// ---- wide selection: 5 <= nb <= 16 (K = 2 nb up to 32).  The register lists of lsm_topk_kernel do not stretch that far (two
// sorted K-lists per thread, 256 * K * 8 bytes of LDS), so this kernel keeps NO per-thread list.  Same contract, same single read
// of every row, same online softmax per thread; nb is a run-time argument.
//
//   buffer   Every wave owns WCAP cells (value, index) in LDS.  Cells [0, ic) hold candidates of the image from earlier rows as
//            (score, flat index); cells [ic, cnt) hold candidates of the row being read as (logit, index in the row).
//   stream   An element at or above the wave's bound `thr` (-inf at the start of a row) that is neither banned nor in the row's
//            history is appended by ballot compaction: position = cnt + number of appending lanes below this one.
//   reduce   When cnt passes WCAP - 64 the wave reduces the row's cells: every lane takes the largest of its (up to) WPL cells,
//            and `t` is the K-th largest of those 64 lane maxima (rank by counting over 64 lane broadcasts).  The maxima are 64
//            DISTINCT elements of the row, so t is a lower bound of the row's K-th best logit; thr = t minus the margin of the
//            narrow kernel (far wider than any pair of logits whose rounded scores could tie), and the cells below thr are
//            compacted away.  An element below thr has K elements of the row whose SCORES are strictly greater, so it is in no
//            top K: dropping it changes no output.  (On Gaussian logits the 32nd largest of 64 maxima of 8 is about the 42nd of
//            512: the cells shrink to ~1/12 and fill up again about twice in a row of 30,524.)
//   bounded  Appends happen only while cnt <= WCAP - 64 and add at most 64.  A reduce leaves at most WCAP / 2 cells of the row, or
//            else (more than that within the margin of t: rows of near-equal logits) the wave switches to the STRICT form for the
//            rest of the row: the row's cells are cut to their exact best K in (logit descending, index ascending) order by K
//            rounds of a wave-wide arg-max, and only elements better than the K-th in that order are appended from then on.  That
//            is the order the narrow kernel's per-thread lists keep, and what equal logits need (equal logits give equal scores,
//            the lower index wins); it is the one place where two DIFFERENT logits whose rounded scores tie are ordered by logit.
//            A row starts with ic <= WKEEP cells of the image, so cnt <= WKEEP + WCAP / 2 after a reduce.  NaN compares false
//            against every bound, so a NaN never enters a buffer; every loop has a trip count fixed by V, K or WCAP.
//   row end  The block combines the threads' softmax states into (max, log-sum-exp) as the narrow kernel does; every wave turns
//            the row's cells into scores `(x - max) - lse + beam_score` in place and, in the penalty form, appends the history
//            tokens (one per thread, scored as in the narrow kernel).  All cells are candidates of the image now.  With more than
//            WKEEP of them the wave prunes: the K-th largest lane maximum of the SCORES bounds the image's K-th best score from
//            below, cells under it have K strictly better ones; should more than WKEEP tie or pass (not seen on real logits), the
//            exact best K in (score descending, flat index ascending) order are kept.  No margin: these are the final keys.
//   merge    After the last row every wave selects its exact best K (K rounds of arg-max over its cells), the four lists meet
//            in LDS, wave 0 selects the image's K best and lane r writes place r.
//
// All loops over a row have the same trip count in every lane (a lane past the end of the row carries a false predicate), because
// reduce and the selections shuffle across the wave.
constexpr int WCAP = 512;           // cells per wave
constexpr int WPL = WCAP / 64;      // cells per lane
constexpr int WKEEP = 128;          // cells of the image a wave takes into the next row at most
constexpr int WMAXK = 2 * MAXNB_WIDE;

__device__ __forceinline__ void wave_lds_sync() {   // LDS written by some lanes of a wave is read by others: no instruction,
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // (a wave's LDS operations execute in order) but the compiler
  __builtin_amdgcn_wave_barrier();                         // must not move accesses across this point
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int lanes_below(unsigned long long bal) {   // set bits of `bal` below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}
// K-th largest (1 <= K <= 64, with multiplicity) of the 64 lanes' values; no NaN among them.
__device__ __forceinline__ float lanes_kth_largest(float v, int K) {
  int above = 0;
#pragma unroll
  for (int l = 0; l < 64; ++l)
    above += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)) > v ? 1 : 0;
  // the values with fewer than K values above them are the K largest: their smallest is the K-th
  return -wave_max(above < K ? -v : -INFINITY);
}
// The best K (<= 64) of the wave's 64 * N cells in (s descending, i ascending) order: lane r returns the r-th, every other lane
// (and every place past the number of cells) the empty cell (-inf, 0x7fffffff).  Empty cells are never chosen; indices are unique.
// The cells are consumed.  All 64 lanes must call it.
template <int N>
__device__ __forceinline__ Cand select_k(float (&s)[N], int (&x)[N], int K) {
  const int lane = threadIdx.x & 63;
  Cand mine{-INFINITY, 0x7fffffff};
  for (int r = 0; r < K; ++r) {
    Cand c{-INFINITY, 0x7fffffff};
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (better(s[j], x[j], c.s, c.i)) { c.s = s[j]; c.i = x[j]; }
    c = wave_best(c);
    if (c.i == 0x7fffffff) break;                      // (wave-uniform) nothing left
    if (lane == r) mine = c;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (x[j] == c.i) { s[j] = -INFINITY; x[j] = 0x7fffffff; }
  }
  return mine;
}

template <bool RP>
__global__ __launch_bounds__(256) void lsm_topk_wide_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ beam_scores, int NB, int NBL, int V,
                                                            int ban, float* __restrict__ out_s, int* __restrict__ out_i,
                                                            const int32_t* __restrict__ hist, int hist_len, int ld_hist,
                                                            float penalty) {
  __shared__ float red[4];
  __shared__ int hs_tok[MAXLEN];
  __shared__ unsigned hs_bits[256];                      // penalty form: 8,192-bit filter in front of the history list
  __shared__ float buf_x[4 * WCAP];
  __shared__ int buf_i[4 * WCAP];
  __shared__ float mg_s[4 * WMAXK];
  __shared__ int mg_i[4 * WMAXK];
  const int K = 2 * NB;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* bx = buf_x + w * WCAP;
  int* bi = buf_i + w * WCAP;
  int cnt = 0;                                           // wave-uniform: cells of bx / bi in use
  const bool vec = (V & 3) == 0;                         // rows are then 16-B aligned: 4 logits per load
  constexpr float L2E = 1.4426950408889634f;
  for (int beam = 0; beam < NBL; ++beam) {
    const float* row = logits + ((size_t)b * NBL + beam) * V;
    if (RP) {
      __syncthreads();                                   // (the previous row's readers are done)
      if (tid < hist_len) hs_tok[tid] = hist[((size_t)b * NB + beam) * ld_hist + tid];
      hs_bits[tid] = 0u;
      __syncthreads();
      if (tid < hist_len) {
        const int t = hs_tok[tid];
        if (t >= 0 && t < V) atomicOr(&hs_bits[(t >> 5) & 255], 1u << (t & 31));
      }
      __syncthreads();
    }
    // (64 of 8,192 bits are set at most: 127 of 128 candidates skip the walk over the list)
    auto in_hist = [&](int t) {
      bool f = false;
      if ((hs_bits[(t >> 5) & 255] >> (t & 31)) & 1u)
        for (int h = 0; h < hist_len; ++h) f |= hs_tok[h] == t;
      return f;
    };
    const int ic = cnt;                                  // cells [0, ic): the image so far, (score, flat index); ic <= WKEEP
    float m = -INFINITY, sum = 0.f;
    float thr = -INFINITY;                               // wave-uniform bound of the margin form
    bool strict = false;                                 // wave-uniform: the strict form is on for the rest of the row
    Cand kth{-INFINITY, 0x7fffffff};                     // strict form: the row's K-th best (logit, index) so far
    auto wanted = [&](float x, int i) { return strict ? better(x, i, kth.s, kth.i) : x >= thr; };
    auto reduce = [&]() {                                // over the row's cells [ic, cnt); cnt - ic <= WCAP
      wave_lds_sync();
      float ev[WPL];
      int ei[WPL];
#pragma unroll
      for (int j = 0; j < WPL; ++j) {
        const int p = ic + j * 64 + lane;
        ev[j] = p < cnt ? bx[p] : -INFINITY;
        ei[j] = p < cnt ? bi[p] : 0x7fffffff;
      }
      wave_lds_sync();                                   // every cell is in a register before any is overwritten
      if (!strict) {
        float lm = ev[0];
#pragma unroll
        for (int j = 1; j < WPL; ++j) lm = fmaxf(lm, ev[j]);
        const float t = lanes_kth_largest(lm, K);
        const float bound = t - 1e-5f * (fabsf(t) + 64.f);
        if (bound > thr) thr = bound;                    // (t = -inf: the bound stays)
        int n = ic;
#pragma unroll
        for (int j = 0; j < WPL; ++j) {
          const bool keep = ei[j] != 0x7fffffff && ev[j] >= thr;
          const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
          if (keep) {                                    // (n + lanes below <= ic + j * 64 + lane: never past the cell it came from)
            const int p = n + lanes_below(bal);
            bx[p] = ev[j]; bi[p] = ei[j];
          }
          n += __builtin_popcountll(bal);
        }
        cnt = n;
        if (cnt - ic <= WCAP / 2) { wave_lds_sync(); return; }
        strict = true;
      }
      const Cand c = select_k<WPL>(ev, ei, K);
      const bool have = c.i != 0x7fffffff;                 // lanes 0 .. min(K, cells) - 1
      if (have) { bx[ic + lane] = c.s; bi[ic + lane] = c.i; }
      cnt = ic + __builtin_popcountll(__builtin_amdgcn_ballot_w64(have));
      kth.s = __shfl(c.s, K - 1, 64);
      kth.i = __shfl(c.i, K - 1, 64);                    // (fewer than K cells: the empty cell, which everything beats)
      wave_lds_sync();
    };
    auto append = [&](float x, int i, bool ok) {         // needs cnt <= WCAP - 64
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(ok);
      if (ok) {
        const int p = cnt + lanes_below(bal);            // < WCAP by the line above; the test costs nothing
        if (p < WCAP) { bx[p] = x; bi[p] = i; }
      }
      cnt += __builtin_popcountll(bal);
    };
    auto push = [&](float x, int i, bool ok) {
      if (__builtin_amdgcn_ballot_w64(ok) == 0) return;
      append(x, i, ok);
      if (cnt > WCAP - 64) reduce();                     // leaves cnt <= WKEEP + WCAP / 2
    };
    if (vec) {
      for (int i0 = 0; i0 < V; i0 += 1024) {
        const int i = i0 + tid * 4;
        const bool in = i < V;
        f32x4 x = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        float mx = -INFINITY;
        if (in) {
          x = *(const f32x4*)(row + i);
          mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
          if (mx > m) {                                   // (m = -inf at first: sum = 0 * 2^-inf = 0)
            sum *= __builtin_amdgcn_exp2f((m - mx) * L2E);
            m = mx;
          }
          const float ml = m * L2E;
          sum += (__builtin_amdgcn_exp2f(__builtin_fmaf(x[0], L2E, -ml)) + __builtin_amdgcn_exp2f(__builtin_fmaf(x[1], L2E, -ml))) +
                 (__builtin_amdgcn_exp2f(__builtin_fmaf(x[2], L2E, -ml)) + __builtin_amdgcn_exp2f(__builtin_fmaf(x[3], L2E, -ml)));
        }
        if (__builtin_amdgcn_ballot_w64(in && (strict || mx >= thr)) != 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            bool ok = in && i + e != ban && wanted(x[e], i + e);   // (the banned token counts in the softmax, never as a candidate)
            if (RP && ok) ok = !in_hist(i + e);
            push(x[e], i + e, ok);
          }
        }
      }
    } else {
      for (int i0 = 0; i0 < V; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < V;
        float x = -INFINITY;
        if (in) {
          x = row[i];
          if (x > m) {
            sum *= __builtin_amdgcn_exp2f((m - x) * L2E);
            m = x;
          }
          sum += __builtin_amdgcn_exp2f((x - m) * L2E);
        }
        bool ok = in && i != ban && wanted(x, i);
        if (RP && ok) ok = !in_hist(i);
        push(x, i, ok);
      }
    }
    const float M = block_reduce_max(m, red);
    // (a thread that saw no element has m = -inf, sum = 0: contributes 0)
    sum = block_reduce_sum(m == -INFINITY ? 0.f : sum * __builtin_amdgcn_exp2f((m - M) * L2E), red);
    const float lse = logf(sum);
    const float bs = beam_scores[b * NB + beam];
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < WPL; ++j) {                      // the row's cells become candidates of the image, in place
      const int p = ic + j * 64 + lane;
      if (p < cnt) { bx[p] = (bx[p] - M) - lse + bs; bi[p] += beam * V; }
    }
    if (RP) {                                            // (cnt <= WCAP - 64 after every push)
      float hs = 0.f;
      int hi = 0;
      bool first = false;
      if (tid < hist_len) {
        const int t = hs_tok[tid];
        first = t >= 0 && t < V && t != ban;             // (scatter_ of equal values: a repeated token is penalised once)
        for (int h = 0; h < tid; ++h) first &= hs_tok[h] != t;
        if (first) {
          const float lp = (row[t] - M) - lse;
          hs = (lp < 0.f ? lp * penalty : lp / penalty) + bs;
          hi = beam * V + t;
        }
      }
      append(hs, hi, first && hs == hs);                 // (a NaN never enters the buffer)
    }
    wave_lds_sync();
    if (cnt > WKEEP && beam + 1 < NBL) {                 // prune the image's cells [0, cnt) by their final keys
      float ev[WPL];
      int ei[WPL];
#pragma unroll
      for (int j = 0; j < WPL; ++j) {
        const int p = j * 64 + lane;
        ev[j] = p < cnt ? bx[p] : -INFINITY;
        ei[j] = p < cnt ? bi[p] : 0x7fffffff;
      }
      wave_lds_sync();
      float lm = ev[0];
#pragma unroll
      for (int j = 1; j < WPL; ++j) lm = fmaxf(lm, ev[j]);
      const float t = lanes_kth_largest(lm, K);          // K distinct cells score t or more
      int n = 0;
#pragma unroll
      for (int j = 0; j < WPL; ++j) {
        const bool keep = ei[j] != 0x7fffffff && ev[j] >= t;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
        if (keep) {
          const int p = n + lanes_below(bal);
          bx[p] = ev[j]; bi[p] = ei[j];
        }
        n += __builtin_popcountll(bal);
      }
      cnt = n;
      if (cnt > WKEEP) {                                 // (wave-uniform) exact: the best K by (score, flat index)
        const Cand c = select_k<WPL>(ev, ei, K);
        const bool have = c.i != 0x7fffffff;
        if (have) { bx[lane] = c.s; bi[lane] = c.i; }
        cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(have));
      }
      wave_lds_sync();
    }
  }
  {
    float cs[WPL];
    int ci[WPL];
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
      const int p = j * 64 + lane;
      cs[j] = p < cnt ? bx[p] : -INFINITY;
      ci[j] = p < cnt ? bi[p] : 0x7fffffff;
    }
    const Cand best = select_k<WPL>(cs, ci, K);          // lane r: the r-th best candidate of the image in this wave
    if (lane < WMAXK) { mg_s[w * WMAXK + lane] = best.s; mg_i[w * WMAXK + lane] = best.i; }
  }
  __syncthreads();
  if (w == 0) {
    float fs[2] = {mg_s[lane], mg_s[64 + lane]};
    int fi[2] = {mg_i[lane], mg_i[64 + lane]};
    const Cand g = select_k<2>(fs, fi, K);
    if (lane < K) { out_s[(size_t)b * K + lane] = g.s; out_i[(size_t)b * K + lane] = g.i; }
  }
}

// ---- teacher-forced form (vidil_logsoftmax_topk_penalty with num_beams == 0): no search, score the GIVEN token of every row
// (reference: models/med.py:909-917, CrossEntropyLoss(label_smoothing) on the shifted prediction scores).  One workgroup per
// row, ONE read of the row: every thread keeps an online-softmax state (running maximum m, sum of exp(x - m)), the plain sum
// of its logits (the label-smoothing term needs mean_j lp[j] = mean logit - lse) and its best (logit, index); the states are
// combined as (max, sum) pairs by wave shuffles and one LDS exchange.  Rows start 4-byte aligned only (V = 30,524: odd rows
// are 8 bytes off a 16-byte boundary), so a row is a scalar head up to the next 16-byte boundary, 16-byte loads, a scalar tail.
// exp(x - m) is formed from the DIFFERENCE (x - m) * log2(e): an -inf logit gives exp2(-inf) = 0, and no term is ever
// inf - inf because a thread adds nothing while its maximum is still -inf.
struct TfState {
  float m, sum, tot, bv;
  int bi;
};
__device__ __forceinline__ void tf_one(TfState& s, float x, int i) {
  constexpr float L2E = 1.4426950408889634f;
  if (x > s.m) {
    s.sum *= __builtin_amdgcn_exp2f((s.m - x) * L2E);
    s.m = x;
  }
  if (s.m > -INFINITY) s.sum += __builtin_amdgcn_exp2f((x - s.m) * L2E);
  s.tot += x;
  if (x > s.bv) { s.bv = x; s.bi = i; }            // (indices arrive in increasing order: the first of equals stays)
}
__device__ __forceinline__ void tf_four(TfState& s, const f32x4 x, int i) {
  constexpr float L2E = 1.4426950408889634f;
  const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
  if (mx > s.m) {
    s.sum *= __builtin_amdgcn_exp2f((s.m - mx) * L2E);
    s.m = mx;
  }
  if (s.m > -INFINITY)
    s.sum += (__builtin_amdgcn_exp2f((x[0] - s.m) * L2E) + __builtin_amdgcn_exp2f((x[1] - s.m) * L2E)) +
             (__builtin_amdgcn_exp2f((x[2] - s.m) * L2E) + __builtin_amdgcn_exp2f((x[3] - s.m) * L2E));
  s.tot += (x[0] + x[1]) + (x[2] + x[3]);
  if (mx > s.bv) {                                 // rare after the first few loads: a thread's best moves O(log n) times
    s.bv = mx;
    s.bi = i + (x[0] == mx ? 0 : x[1] == mx ? 1 : x[2] == mx ? 2 : 3);
  }
}

// CANDS (vidil_logsoftmax_topk_penalty with num_beams == 0 and beams_in_logits = A > 0): the many-labels sibling — `labels`
// holds A candidate token ids SHARED by all rows (ld_labels = A) and out_s is [rows, A]: out_s[r][a] = log_softmax(row r)[labels[a]]
// (reference: models/blip_vqa.py:134-135, the first-token probabilities of an answer list).  Same first pass; every thread then
// combines the four waves' states itself (same order as thread 0, so the same bits) and the workgroup strides over the candidates:
// a gather from the 122 KB row it has just read, a coalesced store.  Candidates outside [0, V) and -inf logits score -inf
// (never inf - inf).
template <bool CANDS>
__global__ __launch_bounds__(256) void tf_logprob_kernel(const float* __restrict__ logits, int V,
                                                         const int32_t* __restrict__ labels, int ld_labels,
                                                         float* __restrict__ out_s, int* __restrict__ out_i) {
  __shared__ float red_m[4], red_s[4], red_t[4];
  __shared__ Cand red_b[4];
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x;
  const float* row = logits + r * (size_t)V;
  TfState s{-INFINITY, 0.f, 0.f, -INFINITY, 0x7fffffff};
  int head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);   // elements before the first 16-byte boundary
  if (head > V) head = V;
  const int nvec = (V - head) >> 2;
  const int tail0 = head + nvec * 4;
  // (a thread's indices must arrive in increasing order for the tie rule: head, then its vectors, then the tail)
  if (tid < head) tf_one(s, row[tid], tid);
  const f32x4* rv = (const f32x4*)(row + head);
#pragma unroll 2
  for (int v = tid; v < nvec; v += 256) tf_four(s, rv[v], head + v * 4);
  if (tid < V - tail0) tf_one(s, row[tail0 + tid], tail0 + tid);

  // ---- the block's (max, sum) pair, total and best element: shuffles inside a wave, one LDS exchange across the four
  const float wm = wave_max(s.m);
  constexpr float L2E = 1.4426950408889634f;
  const float ws = wave_sum(s.m == -INFINITY ? 0.f : s.sum * __builtin_amdgcn_exp2f((s.m - wm) * L2E));
  const float wt = wave_sum(s.tot);
  Cand c{s.bv, s.bi};
  c = wave_best(c);
  if ((tid & 63) == 0) {
    red_m[tid >> 6] = wm; red_s[tid >> 6] = ws; red_t[tid >> 6] = wt; red_b[tid >> 6] = c;
  }
  __syncthreads();
  if (!CANDS && tid != 0) return;
  const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
  float sum = 0.f, tot = 0.f;
  Cand g = red_b[0];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (red_m[w] > -INFINITY) sum += red_s[w] * __builtin_amdgcn_exp2f((red_m[w] - M) * L2E);
    tot += red_t[w];
    if (w > 0 && better(red_b[w].s, red_b[w].i, g.s, g.i)) g = red_b[w];
  }
  if (tid == 0) out_i[r] = g.i == 0x7fffffff ? 0 : g.i;          // (a row of -inf only has no maximum: index 0)
  if (CANDS) {
    const int A = ld_labels;
    const float lse_c = logf(sum);
    float* o = out_s + r * (size_t)A;
    for (int a = tid; a < A; a += 256) {
      const int c = labels[a];
      float lp_c = -INFINITY;
      if (c >= 0 && c < V) {
        const float x = row[c];
        if (x > -INFINITY) lp_c = (x - M) - lse_c;
      }
      o[a] = lp_c;
    }
    return;
  }
  const int label = labels[r * (size_t)ld_labels];
  float lp = 0.f, lp_mean = 0.f;
  if (label >= 0 && label < V) {                   // (label < 0: ignored; label >= V cannot be refused by the host: ignored too)
    const float lse = logf(sum);
    lp = (row[label] - M) - lse;
    lp_mean = (tot / (float)V - M) - lse;
  }
  out_s[2 * r] = lp;
  out_s[2 * r + 1] = lp_mean;
}

// ---- BeamHypotheses.add (double arithmetic: the reference does this on Python floats)
__device__ void hyp_add(const vidil_beam_state& st, int b, int nb, int max_len, const int32_t* toks, int len,
                        double sum_logprobs) {
  const double score = sum_logprobs / (double)len;
  int n = st.n_hyp[b];
  double* hs = st.hyp_score + (size_t)b * nb;
  int32_t* hl = st.hyp_len + (size_t)b * nb;
  int32_t* ht = st.hyp_tok + (size_t)b * nb * max_len;
  if (n < nb) {
    hs[n] = score; hl[n] = len;
    for (int t = 0; t < len; ++t) ht[(size_t)n * max_len + t] = toks[t];
    st.n_hyp[b] = n + 1;
    st.worst[b] = fmin(score, st.worst[b]);
    return;
  }
  if (!(score > st.worst[b])) return;
  // list is full: the new one is appended, then the lowest (score, position) is deleted.
  int lo = 0;
  for (int j = 1; j < nb; ++j)
    if (hs[j] < hs[lo]) lo = j;
  // (the appended entry has score > worst == hs[lo], so it is never the one deleted)
  for (int j = lo; j + 1 < nb; ++j) {
    hs[j] = hs[j + 1]; hl[j] = hl[j + 1];
    for (int t = 0; t < hl[j]; ++t) ht[(size_t)j * max_len + t] = ht[(size_t)(j + 1) * max_len + t];
  }
  hs[nb - 1] = score; hl[nb - 1] = len;
  for (int t = 0; t < len; ++t) ht[(size_t)(nb - 1) * max_len + t] = toks[t];
  double w = hs[0];
  for (int j = 1; j < nb; ++j) w = fmin(w, hs[j]);
  st.worst[b] = w;
}

__global__ void beam_update_kernel(const vidil_beam_state st, const float* __restrict__ cand_s,
                                   const int32_t* __restrict__ cand_i, int B, int nb, int V, int cur_len, int max_len,
                                   int eos_id, int pad_id) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int K = 2 * nb;
  float ns[MAXNB];
  int nt[MAXNB], nsrc[MAXNB];
  if (st.done[b]) {
    for (int j = 0; j < nb; ++j) { ns[j] = 0.f; nt[j] = pad_id; nsrc[j] = b * nb + j; }
  } else {
    int slot = 0;
    for (int rank = 0; rank < K && slot < nb; ++rank) {
      const int flat = cand_i[b * K + rank];
      const float sc = cand_s[b * K + rank];
      const int beam = flat / V, tok = flat - beam * V;
      const int src = b * nb + beam;
      if (tok == eos_id) {
        if (rank >= nb) continue;
        hyp_add(st, b, nb, max_len, st.seqs + (size_t)src * max_len, cur_len, (double)sc);
      } else {
        ns[slot] = sc; nt[slot] = tok; nsrc[slot] = src; ++slot;
      }
    }
    for (; slot < nb; ++slot) { ns[slot] = -1e9f; nt[slot] = pad_id; nsrc[slot] = b * nb; }  // unreachable
    if (st.n_hyp[b] >= nb) {
      const double cur_score = (double)cand_s[b * K] / (double)cur_len;
      if (st.worst[b] >= cur_score) st.done[b] = 1;
    }
  }
  for (int j = 0; j < nb; ++j) {
    const int row = b * nb + j;
    st.beam_scores[row] = ns[j];
    st.beam_idx[row] = nsrc[j];
    st.next_tok[row] = nt[j];
    const int32_t* src = st.seqs + (size_t)nsrc[j] * max_len;
    int32_t* dst = st.seqs_next + (size_t)row * max_len;
    for (int t = 0; t < cur_len; ++t) dst[t] = src[t];
    dst[cur_len] = nt[j];
  }
  if (st.done[b] && st.n_done != nullptr) atomicAdd(st.n_done, 1);
}

// nb 5..16: one wave per image.  Lane 0 keeps the books exactly as the thread of beam_update_kernel does (same statements, the
// chosen beams in LDS instead of dynamically indexed registers); the 64 lanes then copy the nb x cur_len tokens, which is
// where a single thread spends its time at 16 beams (16 x up to 63 dependent-address loads and stores, one row at a time).
__global__ __launch_bounds__(64) void beam_update_wide_kernel(const vidil_beam_state st, const float* __restrict__ cand_s,
                                                              const int32_t* __restrict__ cand_i, int B, int nb, int V,
                                                              int cur_len, int max_len, int eos_id, int pad_id) {
  __shared__ float ns[MAXNB_WIDE];
  __shared__ int nt[MAXNB_WIDE], nsrc[MAXNB_WIDE];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (lane == 0) {
    const int K = 2 * nb;
    if (st.done[b]) {
      for (int j = 0; j < nb; ++j) { ns[j] = 0.f; nt[j] = pad_id; nsrc[j] = b * nb + j; }
    } else {
      int slot = 0;
      for (int rank = 0; rank < K && slot < nb; ++rank) {
        const int flat = cand_i[b * K + rank];
        const float sc = cand_s[b * K + rank];
        const int beam = flat / V, tok = flat - beam * V;
        if (flat < 0 || beam >= nb) continue;            // (an empty place of the selection, NaN logits: names no row)
        const int src = b * nb + beam;
        if (tok == eos_id) {
          if (rank >= nb) continue;
          hyp_add(st, b, nb, max_len, st.seqs + (size_t)src * max_len, cur_len, (double)sc);
        } else {
          ns[slot] = sc; nt[slot] = tok; nsrc[slot] = src; ++slot;
        }
      }
      for (; slot < nb; ++slot) { ns[slot] = -1e9f; nt[slot] = pad_id; nsrc[slot] = b * nb; }  // (only after empty places)
      if (st.n_hyp[b] >= nb) {
        const double cur_score = (double)cand_s[b * K] / (double)cur_len;
        if (st.worst[b] >= cur_score) st.done[b] = 1;
      }
    }
    if (st.done[b] && st.n_done != nullptr) atomicAdd(st.n_done, 1);
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    const int row = b * nb + j;
    const int32_t* src = st.seqs + (size_t)nsrc[j] * max_len;
    int32_t* dst = st.seqs_next + (size_t)row * max_len;
    for (int t = lane; t < cur_len; t += 64) dst[t] = src[t];
    if (lane == 0) {
      st.beam_scores[row] = ns[j];
      st.beam_idx[row] = nsrc[j];
      st.next_tok[row] = nt[j];
      dst[cur_len] = nt[j];
    }
  }
}

__global__ void beam_finalize_kernel(const vidil_beam_state st, int B, int nb, int cur_len, int max_len, int eos_id,
                                     int pad_id, int32_t* __restrict__ out_tok, int32_t* __restrict__ out_len,
                                     float* __restrict__ out_score) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (!st.done[b]) {
    for (int j = 0; j < nb; ++j) {
      const int row = b * nb + j;
      hyp_add(st, b, nb, max_len, st.seqs + (size_t)row * max_len, cur_len, (double)st.beam_scores[row]);
    }
  }
  // sorted(beams, key=score).pop(): the highest score, the LAST one among equals
  const int n = st.n_hyp[b];
  const double* hs = st.hyp_score + (size_t)b * nb;
  int best = 0;
  for (int j = 1; j < n; ++j)
    if (hs[j] >= hs[best]) best = j;
  const int len = st.hyp_len[(size_t)b * nb + best];
  const int32_t* ht = st.hyp_tok + ((size_t)b * nb + best) * max_len;
  for (int t = 0; t < max_len; ++t) out_tok[(size_t)b * max_len + t] = t < len ? ht[t] : pad_id;
  if (len < max_len) out_tok[(size_t)b * max_len + len] = eos_id;
  out_len[b] = len;
  out_score[b] = (float)hs[best];
}

}  // namespace

static int launch_lsm_topk(const float* logits, const float* beam_scores, int32_t B, int32_t nb, int32_t nbl, int32_t V,
                           int32_t ban_token, float* out_scores, int32_t* out_index, const int32_t* hist, int32_t hist_len,
                           int32_t ld_hist, float penalty, void* stream, const char* who) {
  VIDIL_REQUIRE(nbl >= 1 && nbl <= nb, "%s: beams_in_logits=%d must be in [1, num_beams=%d]", who, nbl, nb);
  VIDIL_REQUIRE(logits && beam_scores && out_scores && out_index, "%s: null pointer", who);
  VIDIL_REQUIRE(B > 0 && V > 0, "%s: bad shape", who);
  VIDIL_REQUIRE((long)nb * V < 0x7fffffffL, "%s: nb*V overflows int32", who);
  hipStream_t s = (hipStream_t)stream;
  if (nb > MAXNB && nb <= MAXNB_WIDE) {
    // (HF's topk over nb * V scores fails there as well; the narrow kernel fills such places with -inf / 0x7fffffff)
    VIDIL_REQUIRE((long)nbl * V >= 2L * nb, "%s: beams_in_logits=%d rows of V=%d logits hold fewer than 2*num_beams=%d candidates",
                  who, nbl, V, 2 * nb);
    // The logits must be device memory: there is no host path (the Python layer refuses CPU tensors the same way), and a
    // host address handed to 256 threads per image faults the GPU for everyone on it.  One runtime query per launch, no stream
    // operation (legal inside a stream capture).  It also keeps argument-check tests, which pass small integers as pointers,
    // from launching: tests/test_caption_scoring_cpu.py pins VIDIL_EUNSUP for such a 5-beam call.
    {
      hipPointerAttribute_t at;
      const hipError_t e = hipPointerGetAttributes(&at, logits);
      if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged)) {
        if (e != hipSuccess) (void)hipGetLastError();      // (the query's own error is not a launch error of a later call)
        vidil_set_error("%s: num_beams=%d: logits %p are not device memory: host memory is not supported (no CPU path)", who, nb,
                        (const void*)logits);
        return VIDIL_EUNSUP;
      }
    }
    if (hist) hipLaunchKernelGGL(lsm_topk_wide_kernel<true>, dim3(B), dim3(256), 0, s, logits, beam_scores, nb, nbl, V, ban_token,
                                 out_scores, out_index, hist, hist_len, ld_hist, penalty);
    else hipLaunchKernelGGL(lsm_topk_wide_kernel<false>, dim3(B), dim3(256), 0, s, logits, beam_scores, nb, nbl, V, ban_token,
                            out_scores, out_index, nullptr, 0, 0, 1.f);
    VIDIL_CHECK_LAUNCH(who);
    return VIDIL_OK;
  }
#define VIDIL_LSM(NB_)                                                                                                          \
  case NB_:                                                                                                                     \
    if (hist) hipLaunchKernelGGL((lsm_topk_kernel<NB_, true>), dim3(B), dim3(256), 0, s, logits, beam_scores, nbl, V, ban_token, \
                                 out_scores, out_index, hist, hist_len, ld_hist, penalty);                                      \
    else hipLaunchKernelGGL((lsm_topk_kernel<NB_, false>), dim3(B), dim3(256), 0, s, logits, beam_scores, nbl, V, ban_token,     \
                            out_scores, out_index, nullptr, 0, 0, 1.f);                                                         \
    break;
  switch (nb) {
    VIDIL_LSM(1) VIDIL_LSM(2) VIDIL_LSM(3) VIDIL_LSM(4)
    default:
      vidil_set_error("%s: num_beams=%d not supported (1..16)", who, nb);
      return VIDIL_EUNSUP;
  }
#undef VIDIL_LSM
  VIDIL_CHECK_LAUNCH(who);
  return VIDIL_OK;
}

extern "C" int vidil_logsoftmax_topk(const float* logits, const float* beam_scores, int32_t B, int32_t nb,
                                     int32_t beams_in_logits, int32_t V, int32_t ban_token, float* out_scores,
                                     int32_t* out_index, void* stream) {
  return launch_lsm_topk(logits, beam_scores, B, nb, beams_in_logits, V, ban_token, out_scores, out_index, nullptr, 0, 0, 1.f,
                         stream, "logsoftmax_topk");
}

extern "C" int vidil_logsoftmax_topk_penalty(const float* logits, const float* beam_scores, int32_t B, int32_t nb,
                                             int32_t beams_in_logits, int32_t V, int32_t ban_token, const int32_t* seqs,
                                             int32_t cur_len, int32_t ld_seqs, float penalty, float* out_scores,
                                             int32_t* out_index, void* stream) {
  if (nb == 0 && beams_in_logits != 0) {
    // candidate form: seqs holds beams_in_logits = A token ids shared by all rows, out_scores is [B, A]; beam_scores, ban_token,
    // cur_len, ld_seqs and penalty are not read
    const char* who = "logsoftmax_topk_penalty (num_beams=0, candidates)";
    VIDIL_REQUIRE(beams_in_logits > 0, "%s: beams_in_logits=%d must be the number of candidates (> 0; 0: teacher-forced form)", who,
                  beams_in_logits);
    VIDIL_REQUIRE(seqs != nullptr, "%s: null candidate ids (seqs)", who);
    VIDIL_REQUIRE(logits && out_scores && out_index, "%s: null pointer", who);
    VIDIL_REQUIRE(B > 0 && V > 0, "%s: bad shape rows=%d V=%d", who, B, V);
    hipLaunchKernelGGL(tf_logprob_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, V, seqs, beams_in_logits,
                       out_scores, out_index);
    VIDIL_CHECK_LAUNCH("logsoftmax_topk_penalty (candidates)");
    return VIDIL_OK;
  }
  if (nb == 0) {
    // teacher-forced form: seqs holds one label per row (row stride ld_seqs); beam_scores, ban_token, cur_len and penalty are
    // not read (beams_in_logits == 0)
    VIDIL_REQUIRE(seqs != nullptr, "logsoftmax_topk_penalty (num_beams=0, teacher-forced): null labels (seqs)");
    VIDIL_REQUIRE(logits && out_scores && out_index, "logsoftmax_topk_penalty (num_beams=0, teacher-forced): null pointer");
    VIDIL_REQUIRE(B > 0 && V > 0, "logsoftmax_topk_penalty (num_beams=0, teacher-forced): bad shape rows=%d V=%d", B, V);
    VIDIL_REQUIRE(ld_seqs >= 1, "logsoftmax_topk_penalty (num_beams=0, teacher-forced): ld_seqs=%d must be >= 1", ld_seqs);
    hipLaunchKernelGGL(tf_logprob_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, V, seqs, ld_seqs, out_scores,
                       out_index);
    VIDIL_CHECK_LAUNCH("logsoftmax_topk_penalty (teacher-forced)");
    return VIDIL_OK;
  }
  VIDIL_REQUIRE(seqs != nullptr, "logsoftmax_topk_penalty: null sequences");
  VIDIL_REQUIRE(cur_len >= 1 && cur_len <= MAXLEN && ld_seqs >= cur_len,
                "logsoftmax_topk_penalty: cur_len=%d must be in [1, %d] and <= ld_seqs=%d", cur_len, MAXLEN, ld_seqs);
  VIDIL_REQUIRE(penalty > 0.f, "logsoftmax_topk_penalty: penalty must be a strictly positive float");
  return launch_lsm_topk(logits, beam_scores, B, nb, beams_in_logits, V, ban_token, out_scores, out_index, seqs, cur_len,
                         ld_seqs, penalty, stream, "logsoftmax_topk_penalty");
}

static int check_state(const vidil_beam_state* st, int nb, int max_len, const char* who) {
  VIDIL_REQUIRE(st != nullptr, "%s: null state", who);
  VIDIL_REQUIRE(st->seqs && st->seqs_next && st->beam_scores && st->beam_idx && st->next_tok && st->done && st->n_hyp &&
                    st->hyp_score && st->hyp_len && st->hyp_tok && st->worst,
                "%s: null pointer in state", who);
  VIDIL_REQUIRE(nb >= 1 && nb <= MAXNB_WIDE, "%s: num_beams=%d not supported (1..16)", who, nb);
  VIDIL_REQUIRE(max_len >= 2 && max_len <= MAXLEN, "%s: max_len=%d not supported (2..64)", who, max_len);
  return VIDIL_OK;
}

extern "C" int vidil_beam_update(const vidil_beam_state* st, const float* cand_scores, const int32_t* cand_index,
                                 int32_t B, int32_t nb, int32_t V, int32_t cur_len, int32_t max_len, int32_t eos_id,
                                 int32_t pad_id, void* stream) {
  int rc = check_state(st, nb, max_len, "beam_update");
  if (rc) return rc;
  VIDIL_REQUIRE(cand_scores && cand_index && B > 0 && V > 0, "beam_update: bad args");
  VIDIL_REQUIRE(cur_len >= 1 && cur_len < max_len, "beam_update: cur_len=%d must be in [1,max_len)", cur_len);
  hipStream_t s = (hipStream_t)stream;
  if (st->n_done != nullptr) {
    hipError_t e = hipMemsetAsync(st->n_done, 0, sizeof(int32_t), s);
    if (e != hipSuccess) { vidil_set_error("beam_update: memset failed: %s", hipGetErrorString(e)); return VIDIL_ELAUNCH; }
  }
  if (nb > MAXNB) hipLaunchKernelGGL(beam_update_wide_kernel, dim3(B), dim3(64), 0, s, *st, cand_scores, cand_index, B, nb, V,
                                     cur_len, max_len, eos_id, pad_id);
  else
  hipLaunchKernelGGL(beam_update_kernel, dim3((B + 63) / 64), dim3(64), 0, s, *st, cand_scores, cand_index, B, nb, V,
                     cur_len, max_len, eos_id, pad_id);
  VIDIL_CHECK_LAUNCH("beam_update");
  return VIDIL_OK;
}

extern "C" int vidil_beam_finalize(const vidil_beam_state* st, int32_t B, int32_t nb, int32_t cur_len, int32_t max_len,
                                   int32_t eos_id, int32_t pad_id, int32_t* out_tokens, int32_t* out_len,
                                   float* out_score, void* stream) {
  int rc = check_state(st, nb, max_len, "beam_finalize");
  if (rc) return rc;
  VIDIL_REQUIRE(out_tokens && out_len && out_score && B > 0, "beam_finalize: bad args");
  VIDIL_REQUIRE(cur_len >= 1 && cur_len <= max_len, "beam_finalize: cur_len=%d", cur_len);
  hipLaunchKernelGGL(beam_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *st, B, nb, cur_len,
                     max_len, eos_id, pad_id, out_tokens, out_len, out_score);
  VIDIL_CHECK_LAUNCH("beam_finalize");
  return VIDIL_OK;
}
