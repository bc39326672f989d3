// gemm_grad.hip — the two backward forms of vidil_gemm (include/vidil_hip.h):
//   VIDIL_EPI_GRAD_IN : out[m][n] = sum_{k<K} A[m][k] · W[k][n]   (dX = dY · W,   W stored as the forward's [Nout,Kin])
//   VIDIL_EPI_GRAD_W  : out[n][k] = sum_{m<M} A[m][n] · W[m][k]   (dW = dY^T · X, both operands [contraction][output])
// Both are  out[i][j] = sum_{c<L} P(i,c) · Q(c,j)  with an R x C output and a contraction of length L:
//   GRAD_IN : R = M, C = N, L = K; P = A as a ROW image [i][c], Q = W as a TRANSPOSED image [c][j];
//   GRAD_W  : R = N, C = K, L = M; P = A and Q = W both as transposed images [c][i] / [c][j].
//
// gfx950 design:
//   * 256 threads = 4 waves in a 2 x 2 grid over a BT x BT output tile (BT = 128 or 64), contraction step 64; every wave owns
//     (BT/2) x (BT/2) as 32x32 MFMA tiles (v_mfma_f32_32x32x16_{f16,bf16}, f32 accumulate).
//   * tiles are staged coalesced in their memory orientation, 16 B per lane, THROUGH REGISTERS with a select: a chunk outside
//     the call (contraction row >= the end of this block's range, output column >= the operand's row) is never dereferenced
//     (its load is pointed at the operand's first 16 bytes) and is replaced by zeros, so no value behind an edge — NaNs
//     included — reaches an MFMA.  The loads of step t+1 are issued before the MFMAs of step t and written into the other
//     of two LDS buffers after them: one barrier per step.
//   * an operand stored [contraction][output] is read with ds_read_b64_tr_b16 (two reads per 32x32x16 fragment); the 16-B
//     chunk index of its image is XORed with a function of the contraction row so that the four rows one 32-lane half reads
//     land on four different 64-B bank spans.  EXEC is all ones at every such read: no branch surrounds them, tiles are padded.
//   * a long contraction over few output tiles is split over blockIdx.y; partials go to the caller's f32 workspace and
//     grad_merge_kernel adds them in split order.  The tile and the split are functions of (M, N, K) alone.
#include "common.h"

namespace {

constexpr int GK = 64;              // contraction rows per step
constexpr int BIG_TILES = 64;       // the 128 x 128 tile from this many 128 x 128 tiles on
constexpr int TARGET_BLOCKS = 512;  // the split stops growing the grid here (a constant: never the CU count)
constexpr int MIN_SPLIT = 128;      // shortest contraction range worth a workgroup
constexpr int MAX_SPLIT = 16;

struct GradPlan { int R, C, L, bt, nsplit, split_len; };

GradPlan grad_plan(const vidil_gemm_args& a) {
  GradPlan g;
  if (a.epi == VIDIL_EPI_GRAD_IN) { g.R = a.M; g.C = a.N; g.L = a.K; }
  else { g.R = a.N; g.C = a.K; g.L = a.M; }
  const long t128 = (long)((g.R + 127) / 128) * ((g.C + 127) / 128);
  g.bt = t128 >= BIG_TILES ? 128 : 64;
  const long tiles = (long)((g.R + g.bt - 1) / g.bt) * ((g.C + g.bt - 1) / g.bt);
  long ns = (g.L + MIN_SPLIT - 1) / MIN_SPLIT;
  if (ns > TARGET_BLOCKS / tiles) ns = TARGET_BLOCKS / tiles;
  if (ns > MAX_SPLIT) ns = MAX_SPLIT;
  if (ns < 1) ns = 1;
  const long per = (g.L + ns - 1) / ns;
  g.split_len = (int)((per + GK - 1) / GK) * GK;
  g.nsplit = (g.L + g.split_len - 1) / g.split_len;
  return g;
}

// byte offset of 16-B chunk `ch` of contraction row `c` in a transposed image [GK][BT] (rows of 2 BT bytes)
template <int BT>
__device__ __forceinline__ int tr_off(int c, int ch) {
  const int x = BT == 128 ? (c & 3) << 2 : ((c >> 1) & 1) << 2;
  return c * (BT * 2) + ((ch ^ x) << 4);
}

template <typename T>
__device__ __forceinline__ typename Elt<T>::x8 tr_frag(const char* lo, const char* hi) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)lo);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)hi);
  const s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(typename Elt<T>::x8, v);
}

template <typename T, int FORM, int BT>
__global__ __launch_bounds__(256) void gemm_grad_kernel(const vidil_gemm_args p, const int split_len, const int nsplit) {
  using x8 = typename Elt<T>::x8;
  constexpr bool IN = FORM == VIDIL_EPI_GRAD_IN;
  constexpr int NCH = BT / 32;            // 16-B chunks per thread per operand per step
  constexpr int TT = BT / 64;             // 32x32 tiles per wave along each axis
  constexpr int IMG = GK * BT * 2;        // bytes of one operand image
  __shared__ __attribute__((aligned(16))) char smem[4 * IMG];   // two buffers of [P image | Q image]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int hi = lane >> 5;
  const int l31 = lane & 31;

  const int R = IN ? p.M : p.N, Cc = IN ? p.N : p.K, L = IN ? p.K : p.M;
  const int ldp = IN ? (p.lda > 0 ? p.lda : p.K) : (p.lda > 0 ? p.lda : p.N);   // row stride of A
  const int ldq = Cc;                                                           // W is dense
  const int tiles_c = (Cc + BT - 1) / BT;
  const int tiles_r = (R + BT - 1) / BT;
  // XCD-aware bijective remap of the block index (as gemm_kernel): consecutive logical tiles share a P panel and one L2
  int logical;
  {
    const int nblk = tiles_r * tiles_c;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int tile_r = logical / tiles_c;
  const int tile_c = logical - tile_r * tiles_c;
  const int i0 = tile_r * BT, j0 = tile_c * BT;
  const int split = blockIdx.y;
  const int c_lo = split * split_len;
  const int c_hi = min(L, c_lo + split_len);

  const T* __restrict__ A = (const T*)p.A;
  const T* __restrict__ W = (const T*)p.W;

  // ---- staging: global -> registers (select) -> LDS
  u32x4 rp[NCH], rq[NCH];
  auto fetch = [&](int kt) {
    const int cb = c_lo + kt * GK;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int q = i * 256 + tid;
      if constexpr (IN) {                       // P: row image [BT rows][GK], 8 chunks per row
        const int r = q >> 3, ch = q & 7;
        const int row = i0 + r, c = cb + ch * 8;
        const bool ok = row < R && c < c_hi;    // (K % 8 == 0, split_len % 64 == 0: a chunk is inside or outside as a whole)
        const T* src = ok ? A + (size_t)row * ldp + c : A;
        const u32x4 v = *(const u32x4*)src;
        rp[i] = ok ? v : u32x4{0, 0, 0, 0};
      } else {                                  // P: transposed image [GK][BT], BT/8 chunks per contraction row
        const int r = q / (BT / 8), ch = q % (BT / 8);
        const int c = cb + r, col = i0 + ch * 8;
        const bool ok = c < c_hi && col < ldp && col < ((R + 7) & ~7);   // (lda % 8 == 0: the chunk ends inside the row)
        const T* src = ok ? A + (size_t)c * ldp + col : A;
        const u32x4 v = *(const u32x4*)src;
        rp[i] = ok ? v : u32x4{0, 0, 0, 0};
      }
      {                                         // Q: transposed image [GK][BT]
        const int r = q / (BT / 8), ch = q % (BT / 8);
        const int c = cb + r, col = j0 + ch * 8;
        const bool ok = c < c_hi && col < Cc;   // (C % 8 == 0)
        const T* src = ok ? W + (size_t)c * ldq + col : W;
        const u32x4 v = *(const u32x4*)src;
        rq[i] = ok ? v : u32x4{0, 0, 0, 0};
      }
    }
  };
  auto commit = [&](int buf) {
    char* lp = smem + buf * 2 * IMG;
    char* lq = lp + IMG;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int q = i * 256 + tid;
      if constexpr (IN) {
        const int r = q >> 3, ch = q & 7;
        *(u32x4*)(lp + r * 128 + ((ch ^ ((r >> 1) & 7)) << 4)) = rp[i];
      } else {
        *(u32x4*)(lp + tr_off<BT>(q / (BT / 8), q % (BT / 8))) = rp[i];
      }
      *(u32x4*)(lq + tr_off<BT>(q / (BT / 8), q % (BT / 8))) = rq[i];
    }
  };

  f32x16 acc[TT][TT];
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // transposed read: the 16-lane group g = lane>>4 takes contraction rows 8 (g>>1) + 4 t + (0..3) of a 16-row k-step and the
  // output columns 16 (g&1) + (0..15) of a 32-column tile; lane 4 q + pp of the group addresses row q, columns 4 pp .. 4 pp + 3
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int tr_row = 8 * (g >> 1) + tq;                 // + 16 ks + 4 t
  const int tr_col = 16 * (g & 1) + 4 * tp;             // + the tile's first column
  const int sw = (lane >> 1) & 7;                       // row image: ((row >> 1) & 7) with row = 32 x + (lane & 31)

  const int nk = (c_hi - c_lo + GK - 1) / GK;
  fetch(0);
  commit(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;       // (block-uniform)
    if (more) fetch(kt + 1);
    const char* lp = smem + (kt & 1) * 2 * IMG;
    const char* lq = lp + IMG;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      x8 pf[TT], qf[TT];
#pragma unroll
      for (int i = 0; i < TT; ++i) {
        if constexpr (IN) {
          pf[i] = *(const x8*)(lp + (wm * (BT / 2) + i * 32 + l31) * 128 + (((ks * 2 + hi) ^ sw) << 4));
        } else {
          const int col = wm * (BT / 2) + i * 32 + tr_col;
          const int c = ks * 16 + tr_row;
          pf[i] = tr_frag<T>(lp + tr_off<BT>(c, col >> 3) + (col & 7) * 2, lp + tr_off<BT>(c + 4, col >> 3) + (col & 7) * 2);
        }
      }
#pragma unroll
      for (int j = 0; j < TT; ++j) {
        const int col = wn * (BT / 2) + j * 32 + tr_col;
        const int c = ks * 16 + tr_row;
        qf[j] = tr_frag<T>(lq + tr_off<BT>(c, col >> 3) + (col & 7) * 2, lq + tr_off<BT>(c + 4, col >> 3) + (col & 7) * 2);
      }
#pragma unroll
      for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) acc[i][j] = Elt<T>::mfma32(pf[i], qf[j], acc[i][j]);
    }
    if (more) commit((kt + 1) & 1);
    __syncthreads();
  }

  // ---------------------------------------------------------------- epilogue
  // acc[i][j][r] : row = i0 + wm*BT/2 + i*32 + (r&3) + 8*(r>>2) + 4*hi,  col = j0 + wn*BT/2 + j*32 + (lane&31)
  const bool direct = nsplit == 1;
  float* __restrict__ dst = direct ? (float*)p.out : (float*)p.q + (size_t)split * R * Cc;
  const size_t ldd = direct ? (size_t)p.ldo : (size_t)Cc;
#pragma unroll
  for (int j = 0; j < TT; ++j) {
    const int col = j0 + wn * (BT / 2) + j * 32 + l31;
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i0 + wm * (BT / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (row < R && col < Cc) {
          float v = acc[i][j][r];
          if (direct && p.resid != nullptr) v += p.resid[(size_t)row * ldd + col];   // (resid may alias out: same lane, read first)
          dst[(size_t)row * ldd + col] = v;
        }
      }
  }
}

// out[r][c] = ((part_0 + part_1) + ... + part_{n-1}) (+ resid[r][c]): the partials in split order, one thread per element
__global__ __launch_bounds__(256) void gemm_grad_merge_kernel(const float* __restrict__ ws, float* out, const float* resid,
                                                              const int R, const int Cc, const int ldo, const int nsplit) {
  const size_t total = (size_t)R * Cc;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  float v = ws[e];
  for (int s = 1; s < nsplit; ++s) v += ws[(size_t)s * total + e];
  const size_t o = (e / Cc) * (size_t)ldo + (e % Cc);
  if (resid != nullptr) v += resid[o];
  out[o] = v;
}

template <typename T, int FORM, int BT>
int launch_grad(const vidil_gemm_args& a, const GradPlan& g, hipStream_t s) {
  const int tiles = ((g.R + BT - 1) / BT) * ((g.C + BT - 1) / BT);
  hipLaunchKernelGGL((gemm_grad_kernel<T, FORM, BT>), dim3(tiles, g.nsplit), dim3(256), 0, s, a, g.split_len, g.nsplit);
  VIDIL_CHECK_LAUNCH("gemm_grad");
  if (g.nsplit > 1) {
    const size_t total = (size_t)g.R * g.C;
    hipLaunchKernelGGL(gemm_grad_merge_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)a.q,
                       (float*)a.out, a.resid, g.R, g.C, a.ldo, g.nsplit);
    VIDIL_CHECK_LAUNCH("gemm_grad merge");
  }
  return VIDIL_OK;
}

template <typename T>
int launch_form(const vidil_gemm_args& a, const GradPlan& g, hipStream_t s) {
  if (a.epi == VIDIL_EPI_GRAD_IN)
    return g.bt == 128 ? launch_grad<T, VIDIL_EPI_GRAD_IN, 128>(a, g, s) : launch_grad<T, VIDIL_EPI_GRAD_IN, 64>(a, g, s);
  return g.bt == 128 ? launch_grad<T, VIDIL_EPI_GRAD_W, 128>(a, g, s) : launch_grad<T, VIDIL_EPI_GRAD_W, 64>(a, g, s);
}

}  // namespace

int vidil_gemm_grad_check(const vidil_gemm_args& a) {
  const bool in = a.epi == VIDIL_EPI_GRAD_IN;
  const char* f = in ? "gemm/grad_in" : "gemm/grad_w";
  VIDIL_REQUIRE(a.dtype == VIDIL_DT_F16 || a.dtype == VIDIL_DT_BF16, "%s: f16 or bf16 operands only (dtype=%d; no fp8 form)", f, a.dtype);
  VIDIL_REQUIRE(a.bias == nullptr, "%s: no bias (the bias gradient is a column sum of dY)", f);
  VIDIL_REQUIRE(a.act == VIDIL_ACT_NONE, "%s: no activation (act=%d)", f, a.act);
  VIDIL_REQUIRE(!a.ln_fold && !a.out16 && !a.out16_split3 && !a.ln_stats_out && !a.rln_gamma && !a.rln_beta && !a.split_k,
                "%s: ln_fold / out16 / out16_split3 / ln_stats_out / rln / split_k do not apply to the backward forms", f);
  VIDIL_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "%s: bad shape M=%d N=%d K=%d", f, a.M, a.N, a.K);
  VIDIL_REQUIRE((long long)a.M * a.N < (1LL << 31) && (long long)a.N * a.K < (1LL << 31) && (long long)a.M * a.K < (1LL << 31),
                "%s: M=%d N=%d K=%d: an operand or the output exceeds 2^31 elements", f, a.M, a.N, a.K);
  VIDIL_REQUIRE(a.K % 8 == 0, "%s: K=%d must be a multiple of 8", f, a.K);
  if (in) {
    VIDIL_REQUIRE(a.N % 8 == 0, "%s: N=%d must be a multiple of 8 (W is dense [K,N])", f, a.N);
    VIDIL_REQUIRE(a.lda == 0 || (a.lda >= a.K && a.lda % 8 == 0), "%s: lda=%d must be 0 or >= K=%d and a multiple of 8", f, a.lda, a.K);
    VIDIL_REQUIRE(a.out && a.ldo >= a.N, "%s: bad out / ldo=%d < N=%d", f, a.ldo, a.N);
  } else {
    VIDIL_REQUIRE(a.lda == 0 ? a.N % 8 == 0 : (a.lda >= a.N && a.lda % 8 == 0),
                  "%s: lda=%d must be >= N=%d and a multiple of 8 (0 = N, then N %% 8 == 0)", f, a.lda, a.N);
    VIDIL_REQUIRE(a.out && a.ldo >= a.K, "%s: bad out / ldo=%d < K=%d", f, a.ldo, a.K);
  }
  VIDIL_REQUIRE(((uintptr_t)a.A & 15) == 0 && ((uintptr_t)a.W & 15) == 0, "%s: operands must be 16-B aligned", f);
  VIDIL_REQUIRE(((uintptr_t)a.out & 15) == 0 && ((uintptr_t)a.resid & 3) == 0, "%s: out must be 16-B aligned (resid 4-B)", f);
  return VIDIL_OK;
}

int vidil_gemm_grad_launch(const vidil_gemm_args& a, hipStream_t s) {
  const GradPlan g = grad_plan(a);
  if (g.nsplit > 1)
    VIDIL_REQUIRE(a.q != nullptr && ((uintptr_t)a.q & 15) == 0,
                  "%s: this shape splits its contraction %d ways: `q` must point at a 16-B aligned f32 workspace of %lld bytes",
                  a.epi == VIDIL_EPI_GRAD_IN ? "gemm/grad_in" : "gemm/grad_w", g.nsplit, 4LL * g.nsplit * g.R * g.C);
  if (a.dtype == VIDIL_DT_BF16) return launch_form<bf16>(a, g, s);
  return launch_form<f16>(a, g, s);
}

void vidil_gemm_grad_kernel_name(const vidil_gemm_args& a, char* buf, int n) {
  const GradPlan g = grad_plan(a);
  snprintf(buf, n, "gemm_grad_kernel<%s, %d, %d>", a.dtype == VIDIL_DT_BF16 ? "__bf16" : "_Float16", a.epi, g.bt);
}
