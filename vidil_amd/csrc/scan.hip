// scan.hip — CLIP ontology scan: scores = img · txt^T per category with a fused
// per-frame top-k, so the [frames x 42,759] score matrix is never written to
// HBM or copied to the host (the reference does both:
// run_visual_tokenization.py:276,298-308).
//
// Exactness: top-k indices must be reproducible bit for bit, so the scan runs
// in f32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32), which is an exact
// k-ordered fmaf chain.  A lane of half hi holds k = 8c + 4*hi + j (j = MFMA
// step 0..3 of chunk c), so every score is
//     s = 0;  for c: for j in 0..3:  s = fma(t[8c+j],   f[8c+j],   s);
//                                    s = fma(t[8c+4+j], f[8c+4+j], s);
// which oracle/scan_ref.c restates literally.
//
// Work split: grid = (class chunks, frame tiles of 32).  A workgroup keeps its
// 32 frame rows in LDS (padded, conflict-free b128 reads) and streams CT class
// tiles (32 classes each) of ONE category from HBM/L2 straight into MFMA A
// operands; each lane keeps a sorted top-k for (its frame, its classes) in
// registers; lists are merged through LDS and one partial list per
// (chunk, frame) goes to the workspace; a second tiny kernel merges chunks.
//
// topk == 0 is the paired softmax-statistics form (the soft-target contrastive
// loss over batch + queue): the 32 rows of a workgroup are 16 VALUE rows and the
// 16 WEIGHT rows paired with them, a lane keeps online-softmax state (running
// maximum, sum of exponentials, and the sum weighted by the partner row's
// score) where the top-k form keeps its sorted list, and the (max, sum,
// weighted sum) states are merged in the same fixed order: 8 lists per row
// through LDS, then the chunks of a category in chunk order (one wave per
// pair and category: stats_merge_kernel).  No atomics.
//
// topk == VIDIL_SCAN_FORM_GRAD is the gradient form of that loss (grad_kernel,
// grad_merge_kernel below): the same 16 + 16 rows and the same score chains,
// the softmax-difference coefficient in registers, and a second contraction
// with the keys on v_mfma_f32_16x16x4_f32 into a [16 pairs x D] accumulator.
#include "common.h"

namespace {

constexpr int TOPK_MAX = 8;
constexpr int CT = 8;      // class tiles per workgroup
constexpr int MAXCAT = 8;

struct ScanP {
  const float* img;
  const float* txt;
  int NF, D, ncat, topk;
  int seg_start[MAXCAT], seg_len[MAXCAT];
  int chunk_prefix[MAXCAT + 1];  // chunks before category c
  float* part_s;   // [nchunks][NFpad][topk]
  int* part_i;
  int NFpad;
};

__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) {
  return s1 > s2 || (s1 == s2 && i1 < i2);
}

template <int TK>
__device__ __forceinline__ void insert(float (&ts)[TK], int (&ti)[TK], float s, int i) {
  if (better(s, i, ts[TK - 1], ti[TK - 1])) {
    ts[TK - 1] = s; ti[TK - 1] = i;
#pragma unroll
    for (int j = TK - 1; j > 0; --j) {
      if (better(ts[j], ti[j], ts[j - 1], ti[j - 1])) {
        const float a = ts[j]; ts[j] = ts[j - 1]; ts[j - 1] = a;
        const int b = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = b;
      }
    }
  }
}

template <int TK>
__global__ __launch_bounds__(256) void scan_kernel(const ScanP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = p.D;
  const int FROW = D + 4;  // floats per frame row in LDS
  float* Fs = (float*)smem;  // [32][FROW]; reused for the list merge afterwards

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int chunk = blockIdx.x, ftile = blockIdx.y;

  int cat = 0;
#pragma unroll
  for (int c = 1; c < MAXCAT; ++c)
    if (c < p.ncat && chunk >= p.chunk_prefix[c]) cat = c;
  const int tile0 = (chunk - p.chunk_prefix[cat]) * CT;            // first class tile within the category
  const int ntiles_cat = (p.seg_len[cat] + 31) / 32;
  const int seg_len = p.seg_len[cat];
  const float* txt = p.txt + (size_t)p.seg_start[cat] * D;

  // ---- stage the 32 frame rows ---------------------------------------------------
  {
    const int vec_per_row = D / 4;
    for (int q = tid; q < 32 * vec_per_row; q += 256) {
      const int r = q / vec_per_row, c = q - r * vec_per_row;
      const int f = ftile * 32 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < p.NF) v = *(const f32x4*)(p.img + (size_t)f * D + c * 4);
      *(f32x4*)(Fs + r * FROW + c * 4) = v;
    }
  }
  __syncthreads();

  float ts[TK];
  int ti[TK];
#pragma unroll
  for (int j = 0; j < TK; ++j) { ts[j] = -INFINITY; ti[j] = 0x7fffffff; }

  const float* frow = Fs + l31 * FROW + 4 * hi;
  for (int tt = wave; tt < CT; tt += 4) {
    const int tile = tile0 + tt;
    if (tile >= ntiles_cat) break;
    int cls = tile * 32 + l31;
    const int cls_ld = cls < seg_len ? cls : seg_len - 1;
    const float* trow = txt + (size_t)cls_ld * D + 4 * hi;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
      const f32x4 a = *(const f32x4*)(trow + c * 8);
      const f32x4 b = *(const f32x4*)(frow + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    // acc[r]: class = tile*32 + (r&3) + 8*(r>>2) + 4*hi ; frame = lane&31
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c2 = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (c2 < seg_len) insert<TK>(ts, ti, acc[r], c2);
    }
  }

  // ---- merge the 8 lists (4 waves x 2 halves) of each frame ------------------------
  __syncthreads();  // everyone is done reading Fs
  float* ms = (float*)smem;                       // [8][32][TK]
  int* mi = (int*)(smem + 8 * 32 * TK * 4);
  {
    const int slot = wave * 2 + hi;
#pragma unroll
    for (int j = 0; j < TK; ++j) {
      ms[(slot * 32 + l31) * TK + j] = ts[j];
      mi[(slot * 32 + l31) * TK + j] = ti[j];
    }
  }
  __syncthreads();
  if (tid < 32) {
    float bs[TK];
    int bi[TK];
#pragma unroll
    for (int j = 0; j < TK; ++j) { bs[j] = -INFINITY; bi[j] = 0x7fffffff; }
    for (int slot = 0; slot < 8; ++slot)
#pragma unroll
      for (int j = 0; j < TK; ++j) insert<TK>(bs, bi, ms[(slot * 32 + tid) * TK + j], mi[(slot * 32 + tid) * TK + j]);
    const size_t o = ((size_t)chunk * p.NFpad + ftile * 32 + tid) * p.topk;
#pragma unroll
    for (int j = 0; j < TK; ++j)
      if (j < p.topk) { p.part_s[o + j] = bs[j]; p.part_i[o + j] = bi[j]; }
  }
}

template <int TK>
__global__ void scan_merge_kernel(const ScanP p, int32_t* __restrict__ out_i, float* __restrict__ out_s) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.NF * p.ncat) return;
  const int f = g / p.ncat, cat = g - f * p.ncat;
  float bs[TK];
  int bi[TK];
#pragma unroll
  for (int j = 0; j < TK; ++j) { bs[j] = -INFINITY; bi[j] = 0x7fffffff; }
  for (int chunk = p.chunk_prefix[cat]; chunk < p.chunk_prefix[cat + 1]; ++chunk) {
    const size_t o = ((size_t)chunk * p.NFpad + f) * p.topk;
    for (int j = 0; j < p.topk; ++j) insert<TK>(bs, bi, p.part_s[o + j], p.part_i[o + j]);
  }
  for (int j = 0; j < p.topk; ++j) {
    out_i[((size_t)f * p.ncat + cat) * p.topk + j] = bi[j] == 0x7fffffff ? -1 : bi[j];
    out_s[((size_t)f * p.ncat + cat) * p.topk + j] = bs[j];
  }
}

// ---- paired softmax statistics (topk == 0) -----------------------------------------------------------------------------------
// State of one row over a set of classes: m = best score (the top-k order: score desc, index asc), i = its class,
// s = sum exp(x - m), t = sum exp(x - m) * y, x the row's own score and y the partner row's score of the same class.
struct Stat {
  float m, s, t;
  int i;
};

__device__ __forceinline__ float rescale(float m_old, float m_new) { return m_old == -INFINITY ? 0.f : expf(m_old - m_new); }

__device__ __forceinline__ void stat_merge(Stat& a, const Stat& b) {
  const bool take = better(b.m, b.i, a.m, a.i);
  const float m = take ? b.m : a.m;
  const float fa = rescale(a.m, m), fb = rescale(b.m, m);
  a.s = a.s * fa + b.s * fb;
  a.t = a.t * fa + b.t * fb;
  a.m = m;
  a.i = take ? b.i : a.i;
}

__global__ __launch_bounds__(256) void stats_kernel(const ScanP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = p.D;
  const int FROW = D + 4;
  float* Fs = (float*)smem;  // [32][FROW]: rows 0..15 value rows, 16..31 their weight rows; reused for the merge

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int chunk = blockIdx.x, ptile = blockIdx.y;
  const int P = p.NF >> 1;

  int cat = 0;
#pragma unroll
  for (int c = 1; c < MAXCAT; ++c)
    if (c < p.ncat && chunk >= p.chunk_prefix[c]) cat = c;
  const int tile0 = (chunk - p.chunk_prefix[cat]) * CT;
  const int ntiles_cat = (p.seg_len[cat] + 31) / 32;
  const int seg_len = p.seg_len[cat];
  const float* txt = p.txt + (size_t)p.seg_start[cat] * D;

  {
    const int vec_per_row = D / 4;
    for (int q = tid; q < 32 * vec_per_row; q += 256) {
      const int r = q / vec_per_row, c = q - r * vec_per_row;
      const int pair = ptile * 16 + (r & 15);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pair < P) v = *(const f32x4*)(p.img + (size_t)((r >> 4) * P + pair) * D + c * 4);
      *(f32x4*)(Fs + r * FROW + c * 4) = v;
    }
  }
  __syncthreads();

  Stat st = {-INFINITY, 0.f, 0.f, 0x7fffffff};
  const float* frow = Fs + l31 * FROW + 4 * hi;
  for (int tt = wave; tt < CT; tt += 4) {
    const int tile = tile0 + tt;
    if (tile >= ntiles_cat) break;
    const int cls = tile * 32 + l31;
    const int cls_ld = cls < seg_len ? cls : seg_len - 1;
    const float* trow = txt + (size_t)cls_ld * D + 4 * hi;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
      const f32x4 a = *(const f32x4*)(trow + c * 8);
      const f32x4 b = *(const f32x4*)(frow + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    // acc[r]: class = tile*32 + (r&3) + 8*(r>>2) + 4*hi ; row = lane&31 ; the partner row's score sits in lane ^ 16
    const float m_old = st.m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c2 = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (c2 < seg_len && better(acc[r], c2, st.m, st.i)) { st.m = acc[r]; st.i = c2; }
    }
    const float alpha = rescale(m_old, st.m);
    float s = st.s * alpha, t = st.t * alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c2 = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const float y = __shfl_xor(acc[r], 16);
      if (c2 < seg_len) {
        const float e = expf(acc[r] - st.m);
        s += e;
        t = fmaf(e, y, t);
      }
    }
    st.s = s; st.t = t;
  }

  // ---- merge the 8 states (4 waves x 2 halves) of each row, slot order -------------------------------------------------
  __syncthreads();  // everyone is done reading Fs
  f32x4* ms = (f32x4*)smem;  // [8][32] of (m, s, t, bits of i)
  {
    const f32x4 v = {st.m, st.s, st.t, __int_as_float(st.i)};
    ms[(wave * 2 + hi) * 32 + l31] = v;
  }
  __syncthreads();
  if (tid < 32) {
    Stat a = {-INFINITY, 0.f, 0.f, 0x7fffffff};
    for (int slot = 0; slot < 8; ++slot) {
      const f32x4 v = ms[slot * 32 + tid];
      const Stat b = {v[0], v[1], v[2], __float_as_int(v[3])};
      stat_merge(a, b);
    }
    const f32x4 v = {a.m, a.s, a.t, __int_as_float(a.i)};
    ((f32x4*)p.part_s)[(size_t)chunk * p.NFpad + ptile * 32 + tid] = v;
  }
}

// One wave per (pair, category).  Lane l merges the l-th run of ceil(n / 64) consecutive chunks of the category's n in chunk
// order; lanes 0 and 1 then merge the 64 run states of the value and of the weight row in lane order.  That is the chunk order
// in a fixed bracketing which depends on n alone (with n <= 64: plainly one chunk after the other); a thread walking all the
// chunks of the 57,600-entry queue by itself waits for 226 dependent loads.
__global__ __launch_bounds__(64) void stats_merge_kernel(const ScanP p, int32_t* __restrict__ out_i, float* __restrict__ out_s) {
  __shared__ f32x4 runs[2][64];
  const int g = blockIdx.x, lane = threadIdx.x;
  const int pair = g / p.ncat, cat = g - pair * p.ncat;
  const size_t row = (size_t)(pair >> 4) * 32 + (pair & 15);  // the value row; its weight row is 16 further
  const int c0 = p.chunk_prefix[cat], c1 = p.chunk_prefix[cat + 1];
  const int per = (c1 - c0 + 63) / 64;
  const int first = c0 + lane * per, last = first + per < c1 ? first + per : c1;
  Stat v = {-INFINITY, 0.f, 0.f, 0x7fffffff}, w = v;
  for (int chunk = first; chunk < last; ++chunk) {
    const f32x4* part = (const f32x4*)p.part_s + (size_t)chunk * p.NFpad + row;
    const f32x4 a = part[0], b = part[16];
    const Stat sa = {a[0], a[1], a[2], __float_as_int(a[3])}, sb = {b[0], b[1], b[2], __float_as_int(b[3])};
    stat_merge(v, sa);
    stat_merge(w, sb);
  }
  runs[0][lane] = f32x4{v.m, v.s, v.t, __int_as_float(v.i)};
  runs[1][lane] = f32x4{w.m, w.s, w.t, __int_as_float(w.i)};
  __syncthreads();
  if (lane < 2) {
    Stat a = {-INFINITY, 0.f, 0.f, 0x7fffffff};
    for (int l = 0; l < 64; ++l) {
      const f32x4 r = runs[lane][l];
      const Stat b = {r[0], r[1], r[2], __float_as_int(r[3])};
      stat_merge(a, b);
    }
    runs[lane][0] = f32x4{a.m, a.s, a.t, __int_as_float(a.i)};
  }
  __syncthreads();
  if (lane == 0) {
    const f32x4 a = runs[0][0], b = runs[1][0];
    float* o = out_s + (size_t)g * 5;
    o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1]; o[4] = b[2];
    const int i = __float_as_int(a[3]);
    out_i[g] = i == 0x7fffffff ? -1 : i;
  }
}

// ---- gradient form (topk == VIDIL_SCAN_FORM_GRAD): the mirror of the paired softmax statistics ------------------------------
// Per pair, with v_j / w_j the value and the weight row's scores (the chains of stats_kernel, bit for bit) over the classes of
// ALL segments:  c_j = cv exp(v_j - lv) - cw exp(w_j - lw),  G = sum_j c_j keys[j,:],  T = sum_j exp(v_j - lv) v_j,  C = sum_j c_j;
// a pair's HARD class h (a class of the first segment, or -1) is left out of G and C: the loss's gradient row is then
// G - C keys[h] = sum_{j != h} c_j (keys[j] - keys[h]), which never forms and cancels the dominant term c_h keys[h].
// A workgroup owns 16 pairs and one key split: GT consecutive class tiles of one segment, so the splits depend on the segment
// lengths alone.  A wave takes the split's tiles wave, wave + 4, ...: the 32x32x2 score MFMA as in stats_kernel, the coefficient
// in registers, then G[16 x D] += c[16 x 32] · keys[32 x D] on the 16x16x4 f32 MFMA.  Its A operand is the coefficient the lane
// already holds (lanes l and l ^ 16 form the same c; k-step s of lane group g = lane >> 4 takes class (s&3) + 16(s>>2) +
// 8(g&1) + 4(g>>1) of the tile, which is register (s&3) + 8(s>>2) + 4(g&1) of the score tile), so no coefficient moves between
// lanes or through LDS.  Its B operand is the key tile read a second time, 16 lanes to 256 contiguous bytes of a key row (the
// tile is 32 KB at D = 256 and was read by this wave just before; four waves' tiles beside the 16 + 16 staged rows exceed the
// 160 KB of LDS by 2.5 KB, so the second read goes to the caches, not to an LDS copy).  Output tile t of column group q holds
// column 64q + 4(lane & 15) + t: one b128 load feeds four MFMAs and a lane's four accumulator tiles are four adjacent columns.
// The four waves' accumulators are added in wave order through LDS, the partial goes to the workspace, and grad_merge_kernel
// adds the splits in split order.  No atomics.
constexpr int GT = 32;  // class tiles per key split (1024 classes)
constexpr int GRAD_DMAX = 256;  // 16 x 256 accumulators = 64 registers per lane

struct GradP {
  const float* rows;    // [2P][D]: value rows, then weight rows
  const float* consts;  // [5][P]: lv, lw, cv, cw, and the bits of the i32 hard class (in segment 0; -1: none)
  const float* keys;
  int P, Ppad, D, ncat, nsplits;
  int seg_start[MAXCAT], seg_len[MAXCAT];
  int split_prefix[MAXCAT + 1];  // splits before segment c
  float* part_g;  // [nsplits][Ppad][D]
  float* part_t;  // [nsplits][Ppad]
  float* part_c;  // [nsplits][Ppad]
};

template <int NQ>  // column groups of 64: D <= 64 NQ
__global__ __launch_bounds__(256) void grad_kernel(const GradP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int D = p.D, P = p.P;
  const int FROW = D + 4;
  float* Fs = (float*)smem;  // [32][FROW]: rows 0..15 value rows, 16..31 their weight rows; reused for the wave merge

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31, l15 = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, ptile = blockIdx.y;

  int cat = 0;
#pragma unroll
  for (int c = 1; c < MAXCAT; ++c)
    if (c < p.ncat && split >= p.split_prefix[c]) cat = c;
  const int tile0 = (split - p.split_prefix[cat]) * GT;
  const int seg_len = p.seg_len[cat];
  const int ntiles_cat = (seg_len + 31) / 32;
  const float* txt = p.keys + (size_t)p.seg_start[cat] * D;

  {
    const int vec_per_row = D / 4;
    for (int q = tid; q < 32 * vec_per_row; q += 256) {
      const int r = q / vec_per_row, c = q - r * vec_per_row;
      const int pair = ptile * 16 + (r & 15);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pair < P) v = *(const f32x4*)(p.rows + (size_t)((r >> 4) * P + pair) * D + c * 4);
      *(f32x4*)(Fs + r * FROW + c * 4) = v;
    }
  }
  // the lane's pair: its four constants (a pair past P has zero rows and zero coefficients)
  const int pair = ptile * 16 + l15;
  float lv = 0.f, lw = 0.f, cv = 0.f, cw = 0.f;
  int hard = -1;
  if (pair < P) {
    lv = p.consts[pair]; lw = p.consts[P + pair]; cv = p.consts[2 * P + pair]; cw = p.consts[3 * P + pair];
    hard = __float_as_int(p.consts[4 * P + pair]);
  }
  if (cat != 0) hard = -1;  // the hard class is a class of the first segment
  __syncthreads();

  f32x4 G[NQ * 4];
#pragma unroll
  for (int i = 0; i < NQ * 4; ++i) G[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float T = 0.f, C = 0.f;

  const float* frow = Fs + l31 * FROW + 4 * hi;
  const bool is_value = l31 < 16;
  for (int tt = wave; tt < GT; tt += 4) {
    const int tile = tile0 + tt;
    if (tile >= ntiles_cat) break;
    const int cls = tile * 32 + l31;
    const int cls_ld = cls < seg_len ? cls : seg_len - 1;
    const float* trow = txt + (size_t)cls_ld * D + 4 * hi;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
      const f32x4 a = *(const f32x4*)(trow + c * 8);
      const f32x4 b = *(const f32x4*)(frow + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    // acc[r]: class = tile*32 + (r&3) + 8*(r>>2) + 4*hi ; row = lane&31 ; the partner row's score sits in lane ^ 16.
    // Lanes l and l ^ 16 form the same coefficient of pair lane & 15 from (v, w) in the same order.
    f32x16 coef;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c2 = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      const float y = __shfl_xor(acc[r], 16);
      const float v = is_value ? acc[r] : y, w = is_value ? y : acc[r];
      const float ev = expf(v - lv), ew = expf(w - lw);
      const bool live = c2 < seg_len;
      coef[r] = live && c2 != hard ? cv * ev - cw * ew : 0.f;  // the hard class is left out of G and C, not of T
      C += coef[r];
      T += live ? ev * v : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int rs = (s & 3) + 8 * (s >> 2);
      const float a = (g & 1) ? coef[rs + 4] : coef[rs];
      const int j = tile * 32 + (s & 3) + 16 * (s >> 2) + 8 * (g & 1) + 4 * (g >> 1);
      const float* krow = txt + (size_t)(j < seg_len ? j : seg_len - 1) * D + 4 * l15;  // a masked class has a == 0
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        f32x4 b = {0.f, 0.f, 0.f, 0.f};
        if (64 * q + 4 * l15 < D) b = *(const f32x4*)(krow + 64 * q);
#pragma unroll
        for (int t = 0; t < 4; ++t) G[q * 4 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], G[q * 4 + t], 0, 0, 0);
      }
    }
  }

  // ---- add the four waves' accumulators in wave order; T: the 8 (wave, half) sums of a pair in slot order ---------------
  // G[q*4 + t][i]: pair 4g + i of the tile, column 64q + 4(lane & 15) + t
  float* Gs = (float*)smem;          // [16][D]
  float* Ts = Gs + 16 * D;           // [8][16]
  float* Cs = Ts + 8 * 16;           // [8][16]
  for (int w = 0; w < 4; ++w) {
    __syncthreads();  // (the first: everyone is done reading Fs)
    if (wave == w) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        if (64 * q + 4 * l15 < D) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            f32x4* dst = (f32x4*)(Gs + (4 * g + i) * D + 64 * q + 4 * l15);
            f32x4 v = {G[q * 4][i], G[q * 4 + 1][i], G[q * 4 + 2][i], G[q * 4 + 3][i]};
            if (w) v = *dst + v;
            *dst = v;
          }
        }
      }
      if (is_value) { Ts[(wave * 2 + hi) * 16 + l15] = T; Cs[(wave * 2 + hi) * 16 + l15] = C; }
    }
  }
  __syncthreads();
  {
    float* out = p.part_g + ((size_t)split * p.Ppad + ptile * 16) * D;
    for (int q = tid; q < 16 * D / 4; q += 256) ((f32x4*)out)[q] = ((const f32x4*)Gs)[q];
    if (tid < 16) {
      float t = 0.f;
      float c = 0.f;
      for (int slot = 0; slot < 8; ++slot) { t += Ts[slot * 16 + tid]; c += Cs[slot * 16 + tid]; }
      p.part_t[(size_t)split * p.Ppad + ptile * 16 + tid] = t;
      p.part_c[(size_t)split * p.Ppad + ptile * 16 + tid] = c;
    }
  }
}

// One block per pair: thread i adds columns 4i..4i+3 of the splits' partial gradients in split order, thread 0 the partial T and C as well.
__global__ __launch_bounds__(64) void grad_merge_kernel(const GradP p, float* __restrict__ out) {
  const int pair = blockIdx.x, i = threadIdx.x;
  if (4 * i < p.D) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.nsplits; ++s) a += *(const f32x4*)(p.part_g + ((size_t)s * p.Ppad + pair) * p.D + 4 * i);
    *(f32x4*)(out + (size_t)pair * p.D + 4 * i) = a;
  }
  if (i == 0) {
    float t = 0.f;
    float c = 0.f;
    for (int s = 0; s < p.nsplits; ++s) { t += p.part_t[(size_t)s * p.Ppad + pair]; c += p.part_c[(size_t)s * p.Ppad + pair]; }
    out[(size_t)p.P * p.D + pair] = t;
    out[(size_t)p.P * p.D + p.P + pair] = c;
  }
}

// Dense variant for the BLIP retrieval backend (--encoder_version blip needs the k_test = 128 best texts per frame,
// too many for per-lane register lists): the same exact-f32 score of every (frame, text row), written out.
__global__ __launch_bounds__(256) void scores_kernel(const float* __restrict__ img, const float* __restrict__ txt, int NF, int D,
                                                     int NC, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int FROW = D + 4;
  float* Fs = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int ftile = blockIdx.y;
  {
    const int vec_per_row = D / 4;
    for (int q = tid; q < 32 * vec_per_row; q += 256) {
      const int r = q / vec_per_row, c = q - r * vec_per_row;
      const int f = ftile * 32 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (f < NF) v = *(const f32x4*)(img + (size_t)f * D + c * 4);
      *(f32x4*)(Fs + r * FROW + c * 4) = v;
    }
  }
  __syncthreads();
  const float* frow = Fs + l31 * FROW + 4 * hi;
  const int f = ftile * 32 + l31;
  const int ntiles = (NC + 31) / 32;
  for (int tt = wave; tt < CT; tt += 4) {
    const int tile = blockIdx.x * CT + tt;
    if (tile >= ntiles) break;
    const int cls = tile * 32 + l31;
    const float* trow = txt + (size_t)(cls < NC ? cls : NC - 1) * D + 4 * hi;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
      const f32x4 a = *(const f32x4*)(trow + c * 8);
      const f32x4 b = *(const f32x4*)(frow + c * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
    }
    if (f < NF) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c2 = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (c2 < NC) out[(size_t)f * NC + c2] = acc[r];
      }
    }
  }
}

int total_chunks(int ncat, const int32_t* seg_len, int* prefix) {
  int n = 0;
  for (int c = 0; c < ncat; ++c) {
    if (prefix) prefix[c] = n;
    const int tiles = (seg_len[c] + 31) / 32;
    n += (tiles + CT - 1) / CT;
  }
  if (prefix) prefix[ncat] = n;
  return n;
}

// The gradient form behind vidil_scan_topk (pointers, NF, D and ncat were checked there).
int scan_grad(const float* img, const float* txt, int NF, int D, int ncat, const int32_t* seg_start_host,
              const int32_t* seg_len_host, void* partial, float* out, hipStream_t s) {
  VIDIL_REQUIRE(NF % 2 == 0,
                "scan_topk: the gradient form needs an even NF, NF/2 value rows then NF/2 weight rows (NF=%d)", NF);
  VIDIL_REQUIRE(D <= GRAD_DMAX, "scan_topk: the gradient form keeps 16 x D accumulators in registers and needs D <= %d (D=%d)",
                GRAD_DMAX, D);
  VIDIL_REQUIRE((uintptr_t)partial % 16 == 0, "scan_topk: the gradient form needs a 16-byte aligned workspace");
  VIDIL_REQUIRE((uintptr_t)out % 16 == 0, "scan_topk: the gradient form needs a 16-byte aligned out_score");
  GradP p;
  p.rows = img; p.keys = txt; p.P = NF / 2; p.D = D; p.ncat = ncat;
  p.consts = img + (size_t)NF * D;
  p.Ppad = (p.P + 15) / 16 * 16;
  for (int c = 0; c < MAXCAT; ++c) { p.seg_start[c] = 0; p.seg_len[c] = 0; }
  int n = 0;
  for (int c = 0; c < ncat; ++c) {
    VIDIL_REQUIRE(seg_len_host[c] > 0 && seg_start_host[c] >= 0 && seg_start_host[c] % 32 == 0,
                  "scan_topk: category %d: start=%d (must be a multiple of 32) len=%d", c, seg_start_host[c], seg_len_host[c]);
    p.seg_start[c] = seg_start_host[c];
    p.seg_len[c] = seg_len_host[c];
    p.split_prefix[c] = n;
    n += ((seg_len_host[c] + 31) / 32 + GT - 1) / GT;
  }
  for (int c = ncat; c <= MAXCAT; ++c) p.split_prefix[c] = n;
  p.nsplits = n;
  p.part_g = (float*)partial;
  p.part_t = p.part_g + (size_t)n * p.Ppad * D;
  p.part_c = p.part_t + (size_t)n * p.Ppad;
  const int ptiles = p.Ppad / 16;
  VIDIL_REQUIRE(ptiles <= 65535, "scan_topk: too many pairs in one call (%d)", p.P);
  int smem = 32 * (D + 4) * 4;
  if (smem < (16 * D + 2 * 8 * 16) * 4) smem = (16 * D + 2 * 8 * 16) * 4;
  const int nq = (D + 63) / 64;
  auto kern = nq == 1 ? grad_kernel<1> : nq == 2 ? grad_kernel<2> : nq == 3 ? grad_kernel<3> : grad_kernel<4>;
  hipLaunchKernelGGL(kern, dim3(n, ptiles), dim3(256), smem, s, p);
  VIDIL_CHECK_LAUNCH("scan_topk/grad");
  hipLaunchKernelGGL(grad_merge_kernel, dim3(p.P), dim3(64), 0, s, p, out);
  VIDIL_CHECK_LAUNCH("scan_topk/grad-merge");
  return VIDIL_OK;
}

}  // namespace

extern "C" int64_t vidil_scan_topk_ws_bytes(int32_t NF, int32_t NCpad, int32_t topk) {
  if (NF > 0 && NCpad > 0 && topk == VIDIL_SCAN_FORM_GRAD) {
    // one partial gradient row of 256 floats, one partial T and one partial C per (key split, pair padded to 16)
    const int64_t splits = (int64_t)NCpad / (GT * 32) + MAXCAT + 1;
    const int64_t ppad = ((int64_t)(NF + 1) / 2 + 15) / 16 * 16;
    return splits * ppad * (GRAD_DMAX + 2) * 4;
  }
  if (NF <= 0 || NCpad <= 0 || topk < 0) return 0;
  // upper bound on chunks: one per CT*32 classes plus one ragged chunk per category
  const int64_t chunks = (int64_t)NCpad / (CT * 32) + MAXCAT + 1;
  const int64_t nfpad = ((int64_t)NF + 31) / 32 * 32;
  if (topk == 0) return chunks * nfpad * 16;  // one (m, s, t, i) state per (chunk, row)
  return chunks * nfpad * topk * 8;
}

extern "C" int vidil_scan_topk(const float* img, const float* txt, int32_t NF, int32_t D, int32_t ncat,
                               const int32_t* seg_start_host, const int32_t* seg_len_host, int32_t topk, void* partial,
                               int32_t* out_index, float* out_score, void* stream) {
  VIDIL_REQUIRE(img && txt && seg_start_host && seg_len_host && partial && out_index && out_score, "scan_topk: null pointer");
  VIDIL_REQUIRE(NF > 0 && D >= 8 && D % 8 == 0 && D <= 1024, "scan_topk: NF=%d D=%d (D%%8==0, D<=1024)", NF, D);
  VIDIL_REQUIRE(ncat >= 1 && ncat <= MAXCAT, "scan_topk: ncat=%d (1..%d)", ncat, MAXCAT);
  if (topk == VIDIL_SCAN_FORM_GRAD)
    return scan_grad(img, txt, NF, D, ncat, seg_start_host, seg_len_host, partial, out_score, (hipStream_t)stream);
  VIDIL_REQUIRE(topk >= 0 && topk <= TOPK_MAX, "scan_topk: topk=%d (1..%d)", topk, TOPK_MAX);
  VIDIL_REQUIRE(topk != 0 || NF % 2 == 0,
                "scan_topk: topk == 0 (paired softmax statistics) needs an even NF, NF/2 value rows then NF/2 weight rows (NF=%d)", NF);
  ScanP p;
  p.img = img; p.txt = txt; p.NF = NF; p.D = D; p.ncat = ncat; p.topk = topk;
  for (int c = 0; c < MAXCAT; ++c) { p.seg_start[c] = 0; p.seg_len[c] = 0; }
  for (int c = 0; c < ncat; ++c) {
    VIDIL_REQUIRE(seg_len_host[c] > 0 && seg_start_host[c] >= 0 && seg_start_host[c] % 32 == 0,
                  "scan_topk: category %d: start=%d (must be a multiple of 32) len=%d", c, seg_start_host[c], seg_len_host[c]);
    p.seg_start[c] = seg_start_host[c];
    p.seg_len[c] = seg_len_host[c];
  }
  const int nchunks = total_chunks(ncat, seg_len_host, p.chunk_prefix);
  for (int c = ncat + 1; c <= MAXCAT; ++c) p.chunk_prefix[c] = nchunks;
  p.NFpad = (NF + 31) / 32 * 32;
  p.part_s = (float*)partial;
  p.part_i = (int*)((char*)partial + (size_t)nchunks * p.NFpad * topk * 4);
  hipStream_t s = (hipStream_t)stream;
  const int ftiles = p.NFpad / 32;
  VIDIL_REQUIRE(ftiles <= 65535, "scan_topk: too many frames in one call (%d)", NF);
  if (topk == 0) {  // NF = 2P rows in tiles of 16 + 16: ceil(P / 16) == NFpad / 32 tiles
    VIDIL_REQUIRE((uintptr_t)partial % 16 == 0, "scan_topk: topk == 0 needs a 16-byte aligned workspace");
    int smem = 32 * (D + 4) * 4;
    if (smem < 8 * 32 * 16) smem = 8 * 32 * 16;
    static int stats_attr_smem = 0;
    if (smem > stats_attr_smem) {
      if (hipFuncSetAttribute((const void*)stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) {
        vidil_set_error("scan_topk: hipFuncSetAttribute failed");
        return VIDIL_ELAUNCH;
      }
      stats_attr_smem = smem;
    }
    hipLaunchKernelGGL(stats_kernel, dim3(nchunks, ftiles), dim3(256), smem, s, p);
    VIDIL_CHECK_LAUNCH("scan_topk/stats");
    hipLaunchKernelGGL(stats_merge_kernel, dim3(NF / 2 * ncat), dim3(64), 0, s, p, out_index, out_score);
    VIDIL_CHECK_LAUNCH("scan_topk/stats-merge");
    return VIDIL_OK;
  }
  const int merge_bytes = 8 * 32 * TOPK_MAX * 8;
  int smem = 32 * (D + 4) * 4;
  if (smem < merge_bytes) smem = merge_bytes;
  auto kern = topk <= 5 ? scan_kernel<5> : scan_kernel<TOPK_MAX>;
  auto mkern = topk <= 5 ? scan_merge_kernel<5> : scan_merge_kernel<TOPK_MAX>;
  static int attr_smem = 0;
  if (smem > attr_smem) {
    hipError_t e1 = hipFuncSetAttribute((const void*)scan_kernel<5>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    hipError_t e2 = hipFuncSetAttribute((const void*)scan_kernel<TOPK_MAX>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      vidil_set_error("scan_topk: hipFuncSetAttribute failed");
      return VIDIL_ELAUNCH;
    }
    attr_smem = smem;
  }
  hipLaunchKernelGGL(kern, dim3(nchunks, ftiles), dim3(256), smem, s, p);
  VIDIL_CHECK_LAUNCH("scan_topk");
  const int nthreads = NF * ncat;
  hipLaunchKernelGGL(mkern, dim3((nthreads + 127) / 128), dim3(128), 0, s, p, out_index, out_score);
  VIDIL_CHECK_LAUNCH("scan_topk/merge");
  return VIDIL_OK;
}

extern "C" int vidil_scan_scores(const float* img, const float* txt, int32_t NF, int32_t D, int32_t NC, float* out,
                                 void* stream) {
  VIDIL_REQUIRE(img && txt && out, "scan_scores: null pointer");
  VIDIL_REQUIRE(NF > 0 && NC > 0 && D >= 8 && D % 8 == 0 && D <= 1024, "scan_scores: NF=%d NC=%d D=%d (D%%8==0, D<=1024)", NF, NC, D);
  const int ftiles = (NF + 31) / 32;
  VIDIL_REQUIRE(ftiles <= 65535, "scan_scores: too many frames in one call (%d)", NF);
  const int smem = 32 * (D + 4) * 4;
  static int attr_smem = 0;
  if (smem > attr_smem) {
    if (hipFuncSetAttribute((const void*)scores_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem) != hipSuccess) {
      vidil_set_error("scan_scores: hipFuncSetAttribute failed");
      return VIDIL_ELAUNCH;
    }
    attr_smem = smem;
  }
  const int chunks = ((NC + 31) / 32 + CT - 1) / CT;
  hipLaunchKernelGGL(scores_kernel, dim3(chunks, ftiles), dim3(256), smem, (hipStream_t)stream, img, txt, NF, D, NC, out);
  VIDIL_CHECK_LAUNCH("scan_scores");
  return VIDIL_OK;
}
