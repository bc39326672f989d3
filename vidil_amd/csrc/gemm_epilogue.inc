// gemm_epilogue.inc — the epilogue of one wave's 128 x 64 output tile, textually included by the 256x256 kernel
// (gemm256.hip; the experimental kernels under tools/experiments/ carry adapted copies) at the point where the accumulators
// are final.  (A function taking the accumulator array by reference made hipcc keep the 128 accumulator registers in
// scratch memory — 628 B per lane — so the body is shared as text, not as a function.)
//
// Names expected in scope: p (vidil_gemm_args), acc[4][2] (f32x16; with VIDIL_EPI_VIEW16 also acc16[8][4] (f32x4)), m_w / n_w (first row / column of the wave's tile),
// ep (char*: the wave's private 8-KiB LDS scratch), st_s[4] / st_ss[4] (FOLD: rstd and mean*rstd per row tile),
// lane, hi, l31, M, N, the template parameters T, TO (aliased as f16 / f16x4 / f16x8), EPI, ACT, FOLD, STATS, RLN
// (residual LayerNorm: st_s / st_ss then describe the RESIDUAL rows) and ESZ = sizeof(T).  Early exits use `break`: the includer wraps this text in do { ... } while (0).
//
// Accumulator layout (v_mfma_f32_32x32x* with SWAPPED operands, D = W_frag · A_frag^T):
//   acc[it][j][rq*4+e]: row = m_w + it*32 + l31 ; col = n_w + j*32 + rq*8 + hi*4 + e
// so a lane owns 4 consecutive output columns of one row, and every store path first transposes through `ep` so that
// global stores are 16 B per lane and 128-256 B contiguous per row.
//
// ACCUMULATOR VIEW.  The store paths below never index the accumulators themselves: a pass (32 rows x 64 columns of the wave's
// tile) is the lane's EIGHT column quads, in two groups g of four (k), each with a row and a column-quad index (0..15) in
// the pass — quadrow(it, g, q4) yields the four values of a group, vw_row(g) / vw_cq(g, k) say where they belong:
//   32x32 form (V16 = false):  g = j, k = rq:  row l31,                 column quad g*8 + k*2 + hi      (8 bias quads per lane)
//   16x16 form (V16 = true):   g = 16-row tile of the pass, k = nj:  row g*16 + (lane & 15),  column quad k*4 + (lane >> 4)
//                              (acc16[2*it + g][k]: v_mfma_f32_16x16x32, gemm_epilogue.h Mma16; 4 bias quads per lane)
// The includer selects the second form with VIDIL_EPI_VIEW16 (a constant expression) and provides `acc16` beside `acc` and, for
// FOLD, st16_s[4] / st16_ss[4]: the row statistics of the OTHER row a lane has in this view (row l31 ^ 16 of row tile `it`, fetched
// by lane permute; group g of the lane is row g*16 + (lane & 15)).  The bias AND column-sum quads follow vw_cq.  Everything behind
// the transposition through `ep` (residual, residual LayerNorm, row partials, 16-bit copy) works in the post-transposition lane
// layout and does not depend on the view.
// Per-element arithmetic and its order are the same in both forms.
  if (n_w >= N) break;

#ifdef VIDIL_EPI_VIEW16
  constexpr bool V16 = VIDIL_EPI_VIEW16;
  static_assert(!V16 || ESZ == 2, "the 16x16 accumulator view: 16-bit operands");
#else
  constexpr bool V16 = false;
#endif
  const int l15 = lane & 15, kq = lane >> 4;
  auto vw_row = [&](int g) {
    if constexpr (V16) return g * 16 + l15;
    else return l31;
  };
  auto vw_cq = [&](int g, int k) {
    if constexpr (V16) return k * 4 + kq;
    else return g * 8 + k * 2 + hi;
  };
  // (FOLD in the 16x16 form: st_s / st_ss describe row l31 = (kq & 1) * 16 + l15 of a row tile, the includer's st16_s / st16_ss row l31 ^ 16)
#ifdef VIDIL_EPI_VIEW16
  const bool own_row[2] = {(kq & 1) == 0, (kq & 1) == 1};
#endif
  constexpr int NBG = V16 ? 1 : 2;    // groups of bias quads a lane holds: the 16x16 form's columns do not depend on g

#ifdef VIDIL_EPI_NIT
  constexpr int NIT = VIDIL_EPI_NIT;   // 32-row tiles of the wave's block (gemm4w.hip: 4, or 2 in its 128-row-tile form)
#else
  constexpr int NIT = 4;
#endif
#ifdef VIDIL_EPI_LAZY
  // LAZY form (gemm4w.hip: the accumulators live in AGPRs; transforming all 128 of them up front would need as many
  // VGPRs at once): the lane's 8 bias / column-sum / scale quads are loaded here and applied, with the activation, when a
  // store pass asks for a quad.  Same arithmetic per element as the eager form below, so the two kernels agree bit for bit.
  // (loads WITHOUT a per-lane bounds branch — the column is clamped into the row instead; quads past N are never stored,
  //  so what they hold does not matter: a load inside an exec-masked block makes the compiler wait with vmcnt(0) where the
  //  block ends, one full memory latency per load and, worse, a drain of everything else in flight)
  f32x4 q_b[2][4], q_c[2][4];
  const bool has_bias = p.bias != nullptr;   // (uniform)
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
      q_b[j][rq] = f32x4{0.f, 0.f, 0.f, 0.f};
      q_c[j][rq] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#ifdef VIDIL_EPI_BIAS_LDS
  constexpr bool VEC_LDS = EPI == VIDIL_EPI_F16 || EPI == VIDIL_EPI_HEADS || EPI == VIDIL_EPI_ARENA || EPI == VIDIL_EPI_F8;
#else
  constexpr bool VEC_LDS = false;
#endif
  if constexpr (VEC_LDS) {
#ifdef VIDIL_EPI_BIAS_LDS
    // (gemm4w.hip: the vectors were fetched into LDS by one DMA instruction during the last K-tile — `epb` points at this
    //  64-column half's bias quads, the column sums lie 512 B further — so the epilogue starts with 16 ds_read_b128 of a
    //  few dozen cycles instead of 16 global loads and an `s_waitcnt vmcnt(0)`)
    if (has_bias) {
#pragma unroll
      for (int j = 0; j < NBG; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) q_b[j][rq] = *(const f32x4*)(epb + vw_cq(j, rq) * 4 * 4);
    }
    if constexpr (FOLD || ESZ == 1) {     // (the folded LayerNorm's column sums, or the fp8 weights' per-column scales)
#pragma unroll
      for (int j = 0; j < NBG; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) q_c[j][rq] = *(const f32x4*)(epb + 512 + vw_cq(j, rq) * 4 * 4);
    }
#endif
  } else {
    if (has_bias) {
#pragma unroll
      for (int j = 0; j < NBG; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int col = n_w + vw_cq(j, rq) * 4;
          q_b[j][rq] = *(const f32x4*)(p.bias + (col + 4 <= N ? col : N - 4));
        }
    }
    if constexpr (FOLD || ESZ == 1) {
      const float* const cvec = FOLD ? p.ln_colsum : p.w_scale;
#pragma unroll
      for (int j = 0; j < NBG; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int col = n_w + vw_cq(j, rq) * 4;
          q_c[j][rq] = *(const f32x4*)(cvec + (col + 4 <= N ? col : N - 4));
        }
    }
  }
  // The four quads (rq = 0..3) of accumulator tile (it, j) at once: packed-f32 arithmetic, two columns per instruction,
  // the 8 pairs in lockstep — with one wave per SIMD the epilogue is VALU-issue bound and nothing else fills the
  // dependent-issue gaps of a serial chain (and nothing runs on the matrix pipe that a packed instruction could slow down).
  auto quadrow = [&](int it, int j, f32x4 (&q4)[4]) {
    f32x2 w[8];
#pragma unroll
    for (int pi = 0; pi < 8; ++pi) {
      const int rq = pi >> 1, e = (pi & 1) * 2;
#ifdef VIDIL_EPI_VIEW16
      if constexpr (V16) w[pi] = f32x2{acc16[it * 2 + j][rq][e], acc16[it * 2 + j][rq][e + 1]};
      else
#endif
        w[pi] = f32x2{acc[it][j][rq * 4 + e], acc[it][j][rq * 4 + e + 1]};
      const f32x2 b2 = {q_b[V16 ? 0 : j][rq][e], q_b[V16 ? 0 : j][rq][e + 1]};
      if constexpr (FOLD) {
        const f32x2 c2 = {q_c[V16 ? 0 : j][rq][e], q_c[V16 ? 0 : j][rq][e + 1]};
#ifdef VIDIL_EPI_VIEW16
        if constexpr (V16) w[pi] = pk_fma(w[pi], pk_splat(own_row[j] ? st_s[it] : st16_s[it]), pk_fma(pk_splat(-(own_row[j] ? st_ss[it] : st16_ss[it])), c2, b2));
        else
#endif
          w[pi] = pk_fma(w[pi], pk_splat(st_s[it]), pk_fma(pk_splat(-st_ss[it]), c2, b2));
      } else if constexpr (ESZ == 1) {
        const f32x2 c2 = {q_c[j][rq][e], q_c[j][rq][e + 1]};
        w[pi] = pk_fma(w[pi], c2, b2);
      } else {
        w[pi] = w[pi] + b2;   // (zeros without a bias: x + 0 == x exactly — an accumulator that started from +0 is never -0)
      }
    }
    if constexpr (ACT == VIDIL_ACT_GELU_ERF && EPI != VIDIL_EPI_F32) {
      gelu_fast2p_n<TO, 8>(w);
    } else if constexpr (ACT != VIDIL_ACT_NONE) {
#pragma unroll
      for (int pi = 0; pi < 8; ++pi) w[pi] = ACT == VIDIL_ACT_GELU_ERF ? gelu_erf2(w[pi]) : quick_gelu2(w[pi]);
    }
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) q4[rq] = f32x4{w[rq * 2][0], w[rq * 2][1], w[rq * 2 + 1][0], w[rq * 2 + 1][1]};
  };
#else
  if constexpr (FOLD) {
    // y = rstd * acc + (b' - (mean * rstd) * colsum): LayerNorm applied to the accumulators (see the kernel comment)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int col = n_w + j * 32 + rq * 8 + hi * 4;
        if (col + 4 <= N) {
          const f32x4 c4 = *(const f32x4*)(p.ln_colsum + col);
          f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
          if (p.bias != nullptr) b4 = *(const f32x4*)(p.bias + col);
#pragma unroll
          for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[it][j][rq * 4 + e] = __builtin_fmaf(acc[it][j][rq * 4 + e], st_s[it], __builtin_fmaf(-st_ss[it], c4[e], b4[e]));
        }
      }
  } else if constexpr (ESZ == 1) {
    // fp8 weights are stored as W / w_scale[n] (check_args: w_scale is required): scale the accumulators back, then the bias
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int col = n_w + j * 32 + rq * 8 + hi * 4;
        if (col + 4 <= N) {
          const f32x4 w4 = *(const f32x4*)(p.w_scale + col);
          f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
          if (p.bias != nullptr) b4 = *(const f32x4*)(p.bias + col);
#pragma unroll
          for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[it][j][rq * 4 + e] = __builtin_fmaf(acc[it][j][rq * 4 + e], w4[e], b4[e]);
        }
      }
  } else
  // bias folded into the accumulators once (4 consecutive columns per register quad)
  if (p.bias != nullptr) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        const int col = n_w + j * 32 + rq * 8 + hi * 4;
        if (col + 4 <= N) {
          const f32x4 b4 = *(const f32x4*)(p.bias + col);
#pragma unroll
          for (int it = 0; it < 4; ++it)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[it][j][rq * 4 + e] += b4[e];
        }
      }
  }
  // activation in place, two accumulators per packed-f32 instruction
  if constexpr (ACT != VIDIL_ACT_NONE) {
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          f32x2 v = {acc[it][j][r], acc[it][j][r + 1]};
          // (erf-GELU: the transcendental-free form where the value is about to be rounded to 16 bits or fewer)
          v = ACT == VIDIL_ACT_GELU_ERF ? (EPI == VIDIL_EPI_F32 ? gelu_erf2(v) : gelu_fast2<TO>(v)) : quick_gelu2(v);
          acc[it][j][r] = v[0];
          acc[it][j][r + 1] = v[1];
        }
  }
  auto quadrow = [&](int it, int j, f32x4 (&q4)[4]) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) q4[rq] = f32x4{acc[it][j][rq * 4 + 0], acc[it][j][rq * 4 + 1], acc[it][j][rq * 4 + 2], acc[it][j][rq * 4 + 3]};
  };
#endif

  int part = 0, head = 0;
  if constexpr (EPI == VIDIL_EPI_HEADS || EPI == VIDIL_EPI_ARENA) {
    const int hd = p.H * 64;
    part = p.part0 + n_w / hd;
    head = (n_w % hd) >> 6;
  }

  if constexpr (EPI == VIDIL_EPI_HEADS) {
    if (part == 2 && p.kv_tiled) {
      // V in fragment tiles (common.h vtile_off).  A lane's accumulator row is one KEY, but the layout keeps the 4
      // keys {4q .. 4q+3} of a dimension d side by side (8 B): each block of 32 keys goes through the wave's LDS
      // scratch as [key][d] (rows padded to 136 B), then lane d collects runs of 4 tile-aligned keys of one image
      // and stores them as 8 B; keys cut off by the block or the image boundary are stored one by one.
      constexpr int ROWB = 136;
      const size_t img_stride = (size_t)p.H * p.Tk_cap * 64;
      f16* const vbase = (f16*)p.vt + (size_t)head * p.Tk_cap * 64;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int mb = m_w + it * 32;
        const int rows = M - mb < 32 ? M - mb : 32;   // wave-uniform
        if (rows <= 0) break;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 q4[4];
          quadrow(it, j, q4);
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const f32x4 q = q4[rq];
            const f16x4 v = {Elt<TO>::from_f32(q[0]), Elt<TO>::from_f32(q[1]), Elt<TO>::from_f32(q[2]), Elt<TO>::from_f32(q[3])};
            if constexpr (V16) *(f16x4*)(ep + vw_row(j) * ROWB + vw_cq(j, rq) * 4 * 2) = v;
            else *(f16x4*)(ep + l31 * ROWB + (j * 32 + rq * 8 + hi * 4) * 2) = v;
          }
        }
        int b = mb / p.T, t = mb - b * p.T;
        for (int r = 0; r < rows;) {
          const int tt = p.t_off + t;
          f16* dst = vbase + (size_t)b * img_stride + vtile_off(tt, lane);
          const char* src = ep + r * ROWB + lane * 2;
          if ((tt & 3) == 0 && r + 4 <= rows && t + 4 <= p.T) {
            const f16x4 v = {*(const f16*)src, *(const f16*)(src + ROWB), *(const f16*)(src + 2 * ROWB),
                             *(const f16*)(src + 3 * ROWB)};
            *(f16x4*)dst = v;
            r += 4;
            t += 4;
          } else {
            *dst = *(const f16*)src;
            r += 1;
            t += 1;
          }
          if (t >= p.T) { t -= p.T; ++b; }
        }
      }
      break;
    }
    if (part == 2 && p.NP != 0) {   // (NP == 0: V stays row-major and takes the 16-B store path of K below)
      // V^T: element (row m, column d) goes to VT[b][h][d][t_off+t]; consecutive lanes = consecutive t
      if constexpr (V16) {      // (the lane's row depends on the group: one (image, token) per group)
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const int m = m_w + it * 32 + vw_row(g);
            if (m < M) {
              const int b = m / p.T, t = m - b * p.T;
              f16* dst = (f16*)p.vt + (((size_t)b * p.H + head) * 64) * (size_t)p.NP + vt_pos(p.t_off + t);
              f32x4 q4[4];
              quadrow(it, g, q4);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                const f32x4 q = q4[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[(size_t)(vw_cq(g, k) * 4 + e) * p.NP] = Elt<TO>::from_f32(q[e]);
              }
            }
          }
        }
        break;
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int m = m_w + it * 32 + l31;
        if (m < M) {
          const int b = m / p.T, t = m - b * p.T;
          f16* dst = (f16*)p.vt + (((size_t)b * p.H + head) * 64) * (size_t)p.NP + vt_pos(p.t_off + t);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            f32x4 q4[4];
            quadrow(it, j, q4);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
              const f32x4 q = q4[rq];
#pragma unroll
              for (int e = 0; e < 4; ++e) dst[(size_t)(j * 32 + rq * 8 + hi * 4 + e) * p.NP] = Elt<TO>::from_f32(q[e]);
            }
          }
        }
      }
      break;
    }
  }

  if constexpr (EPI == VIDIL_EPI_F8) {
    // ---- fp8 rows of 64 columns (64 B), two passes of 64 rows: [64][64] bytes, 16-B chunk index XOR ((row>>2)&3) ----
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int it = pass * 2 + i;
        const int row = i * 32 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 q4[4];
          quadrow(it, j, q4);
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const int cb = j * 32 + rq * 8 + hi * 4;      // first of 4 consecutive columns = byte offset in the row
            const f32x4 q = q4[rq];
            *(uint32_t*)(ep + row * 64 + ((((cb >> 4) ^ ((row >> 2) & 3)) << 4) | (cb & 15))) = pack4_fp8(q[0], q[1], q[2], q[3]);
          }
        }
      }
      const int ch = lane & 3;
#ifdef VIDIL_EPI_LAZY
      // (gemm4w.hip: raw buffer stores on a descriptor over the wave's rows — see the 16-bit path below)
      const uint32_t pitch8 = (uint32_t)p.ldo;
      const int rows_w8 = M - m_w < 32 * NIT ? M - m_w : 32 * NIT;
      const __amdgpu_buffer_rsrc_t r_o8 = uniform_rsrc((char*)p.out + (size_t)m_w * p.ldo + n_w, (rows_w8 > 0 ? (uint32_t)rows_w8 : 0u) * pitch8);
      uint32_t vo8 = n_w + ch * 16 + 16 <= N ? (uint32_t)(pass * 64 + (lane >> 2)) * pitch8 + (uint32_t)ch * 16u : 0x80000000u;
#pragma unroll
      for (int iter = 0; iter < 4; ++iter) {
        const int row = iter * 16 + (lane >> 2);
        const u32x4 v = *(const u32x4*)(ep + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4));
        __builtin_amdgcn_raw_buffer_store_b128(v, r_o8, vo8, 0, 0);
        vo8 += 16u * pitch8;
      }
#else
#pragma unroll
      for (int iter = 0; iter < 4; ++iter) {
        const int row = iter * 16 + (lane >> 2);
        const i32x4 v = *(const i32x4*)(ep + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4));
        const int m = m_w + pass * 64 + row;
        const int col = n_w + ch * 16;
        if (m < M && col + 16 <= N) *(i32x4*)((char*)p.out + (size_t)m * p.ldo + col) = v;
      }
#endif
    }
  } else if constexpr (EPI == VIDIL_EPI_F16 || EPI == VIDIL_EPI_HEADS || EPI == VIDIL_EPI_ARENA) {
    // ---- f16 rows of 64 columns, two passes of 64 rows: [64][64] halfs, 16-B chunk index XOR (row&7) ------
    const float scale = ((EPI == VIDIL_EPI_HEADS || EPI == VIDIL_EPI_ARENA) && part == 0) ? p.q_scale : 1.0f;
#ifdef VIDIL_EPI_LAZY
    // One wave per SIMD: a two-buffer pipeline over the four 32-row tiles (4 KiB of LDS each) with NO exposed LDS latency —
    //   step it:  ds_read of tile it-1 (written a whole step ago)  |  quads of tile it: bias / fold / activation / convert
    //             (the long VALU part: the reads land under it)      |  ds_write of tile it  |  global stores of tile it-1
    // LDS operations of one wave execute in order and the scratch is private, so no wait separates a tile's writes from
    // its reads one step later; the only wait is the (long satisfied) one in front of the stores.
    {
      const int ch = lane & 7;
      auto compute_write = [&](int it, char* buf) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 q4[4];
          quadrow(it, j, q4);
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const f32x4 q = q4[rq];
            const f32x2 q01 = f32x2{q[0], q[1]} * pk_splat(scale), q23 = f32x2{q[2], q[3]} * pk_splat(scale);   // (two v_pk_mul_f32; x * 1 is exact)
            const f16x4 v = {Elt<TO>::from_f32(q01[0]), Elt<TO>::from_f32(q01[1]), Elt<TO>::from_f32(q23[0]), Elt<TO>::from_f32(q23[1])};
            // (16-byte chunk = column quad >> 1, its half = column quad & 1)
            if constexpr (V16) *(f16x4*)(buf + (j * 16 + l15) * 128 + (((rq * 2 + (kq >> 1)) ^ (l15 & 7)) << 4) + (kq & 1) * 8) = v;
            else *(f16x4*)(buf + l31 * 128 + (((j * 4 + rq) ^ (l31 & 7)) << 4) + hi * 8) = v;
          }
        }
      };
      auto read_rows = [&](const char* buf, f16x8 (&v4)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = i * 8 + (lane >> 3);
          v4[i] = *(const f16x8*)(buf + row * 128 + ((ch ^ (row & 7)) << 4));
        }
      };
      // uniform description of the destination (the per-head scatter: one division per 32-row tile, rows 8 apart stepped)
      f16* hb = nullptr;
      int cap = 0, toff = 0;
      bool tiled = false;
      size_t img = 0;
      if constexpr (EPI == VIDIL_EPI_HEADS) {
        if (part == 0) { hb = (f16*)p.q; cap = p.Tq_cap; toff = 0; tiled = false; }
        else { hb = (f16*)(part == 1 ? p.k : p.vt); cap = p.Tk_cap; toff = p.t_off; tiled = p.kv_tiled != 0; }
        hb += (size_t)head * cap * 64;
        img = (size_t)p.H * cap * 64;
      }
      if constexpr (EPI == VIDIL_EPI_ARENA) {   // rows of H*64 with all heads of a token side by side (include/vidil_hip.h)
        hb = (f16*)(part == 0 ? p.q : part == 1 ? p.k : p.vt) + head * 64;
      }
      const bool colok = n_w + ch * 8 + 8 <= N;
      // EPI_F16: raw buffer stores on a descriptor over this wave's block of rows (see the f32 path below: a 32-bit lane
      // offset stepped by one v_add per store, the hardware's range check as the bounds test — rows past M lie beyond
      // num_records, a lane whose columns lie past N carries an offset of 2^31 — instead of an exec-mask save / branch /
      // restore and a 64-bit multiply-add per store: ten issue slots per store became two)
      __amdgpu_buffer_rsrc_t r_o16;
      uint32_t vo_o16 = 0, step_o16 = 0;
      if constexpr (EPI == VIDIL_EPI_F16) {
        const uint32_t pitch = (uint32_t)p.ldo * (uint32_t)sizeof(f16);
        const int rows_w = M - m_w < 32 * NIT ? M - m_w : 32 * NIT;
        r_o16 = uniform_rsrc((char*)p.out + ((size_t)m_w * p.ldo + n_w) * sizeof(f16), (rows_w > 0 ? (uint32_t)rows_w : 0u) * pitch);
        vo_o16 = colok ? (uint32_t)(lane >> 3) * pitch + (uint32_t)ch * 16u : 0x80000000u;
        step_o16 = 8u * pitch;
      }
      // EPI_HEADS: the per-head scatter through a descriptor as well — base = this (part, head)'s plane at the block's
      // first image, a 32-bit offset = image * plane + token row (row-major or fragment-tiled), 2^31 for rows past M /
      // columns past N (num_records = 2^31: a select instead of an exec-mask branch per store).  The (image, token) of the
      // lane's row is divided out ONCE per 128 x 64 block and stepped from there (8 rows per store, 32 per tile).
      __amdgpu_buffer_rsrc_t r_hd;
      int hs_b = 0, hs_t = 0, hs_b0 = 0;
      uint32_t img_b = 0;
      if constexpr (EPI == VIDIL_EPI_HEADS) {
        const int b0 = m_w / p.T;                                   // (uniform)
        hs_b0 = b0;
        r_hd = uniform_rsrc((char*)(hb + (size_t)b0 * img), 0x80000000u);
        const int m0l = m_w + (lane >> 3);
        const int bb = m0l / p.T;
        hs_t = m0l - bb * p.T;
        hs_b = bb - b0;
        img_b = (uint32_t)(img * sizeof(f16));
      }
      auto store_rows = [&](int it, f16x8 (&v4)[4]) {
        const int m_first = m_w + it * 32 + (lane >> 3);
        if constexpr (EPI == VIDIL_EPI_F16) {
          // (called for it = 0, 1, .. in order: the offset simply runs on)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v4[i]), r_o16, vo_o16, 0, 0);
            vo_o16 += step_o16;
          }
        } else if constexpr (EPI == VIDIL_EPI_HEADS) {
          // (called for it = 0, 1, .. in order: four steps of 8 rows leave (hs_b, hs_t) at the next tile's first row; the
          //  uniform choices — row-major or fragment-tiled rows, sequences shorter than a step — are made once per tile)
          auto rows4 = [&](auto tiled_tag) {
            constexpr bool TILED = decltype(tiled_tag)::value;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int m = m_first + i * 8;
              const uint32_t e = TILED ? (uint32_t)ktile_off(toff + hs_t, ch * 8) : (uint32_t)(toff + hs_t) * 64u + (uint32_t)ch * 8u;
              uint32_t off = (uint32_t)hs_b * img_b + e * (uint32_t)sizeof(f16);
              off = (m < M && colok) ? off : 0x80000000u;
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v4[i]), r_hd, off, 0, 0);
              hs_t += 8;
              const bool wrap = hs_t >= p.T;
              hs_t = wrap ? hs_t - p.T : hs_t;
              hs_b = wrap ? hs_b + 1 : hs_b;
            }
          };
          // (sequences shorter than a step of 8 rows never reach this form: vidil_gemm256.hip routes HEADS problems with T < 8
          //  to the 8-wave kernel, whose eager epilogue divides per store)
          if (tiled) {
            rows4(std::true_type{});
          } else {
            rows4(std::false_type{});
          }
        } else {
          // (the divisor made opaque: the reciprocal of p.T is tile-invariant, and hoisted out of the tile loop it is spilled across
          //  the main loop — its reload here is a VMEM load waited for with vmcnt(0); see inv_k in gemm4w.hip)
          int tdiv = p.T;
          asm volatile("" : "+s"(tdiv));
          int b = m_first / tdiv, t = m_first - b * tdiv;
          const size_t hd = (size_t)p.H * 64;
          // (the lane's column offset as a 64-bit value formed HERE: as `+ ch * 8` its zero upper half is a constant the compiler
          //  keeps in a register from the top of the kernel, and the pair was spilled across the main loop as a unit)
          uint32_t coff_hi;
          asm volatile("v_mov_b32 %0, 0" : "=v"(coff_hi));
          const size_t coff = ((size_t)coff_hi << 32) | (uint32_t)(ch * 8);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = m_first + i * 8;
            if (m < M && colok) {
              f16* d = hb + (part == 0 ? (size_t)m : (size_t)(p.t_off + t) * p.arena_rows + (size_t)b * p.slot_stride) * hd + coff;
              *(f16x8*)d = v4[i];
            }
            t += 8;
            while (t >= p.T) { t -= p.T; ++b; }
          }
        }
      };
      // (ONE 4-KiB buffer: the reads of tile it-1 are ISSUED before the writes of tile it, and the LDS operations of a wave
      //  execute in order — the reads return the old contents; the other 4 KiB of the wave's scratch hold the bias /
      //  column-sum vectors of VIDIL_EPI_BIAS_LDS)
      f16x8 vr[4];
      compute_write(0, ep);
#pragma unroll
      for (int it = 1; it < NIT; ++it) {
        read_rows(ep, vr);
        __builtin_amdgcn_sched_barrier(0);
        compute_write(it, ep);
        __builtin_amdgcn_sched_barrier(0);
        store_rows(it - 1, vr);
        __builtin_amdgcn_sched_barrier(0);
      }
      read_rows(ep, vr);
      store_rows(NIT - 1, vr);
    }
#else
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int it = pass * 2 + i;
        const int row = i * 32 + l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 q4[4];
          quadrow(it, j, q4);
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const f32x4 q = q4[rq];
            const f16x4 v = {Elt<TO>::from_f32(q[0] * scale), Elt<TO>::from_f32(q[1] * scale), Elt<TO>::from_f32(q[2] * scale),
                             Elt<TO>::from_f32(q[3] * scale)};
            *(f16x4*)(ep + row * 128 + (((j * 4 + rq) ^ (row & 7)) << 4) + hi * 8) = v;
          }
        }
      }
      const int ch = lane & 7;
#pragma unroll 4
      for (int iter = 0; iter < 8; ++iter) {
        const int row = iter * 8 + (lane >> 3);
        const f16x8 v = *(const f16x8*)(ep + row * 128 + ((ch ^ (row & 7)) << 4));
        const int m = m_w + pass * 64 + row;
        const int col = n_w + ch * 8;
        if (m < M && col + 8 <= N) {
          if constexpr (EPI == VIDIL_EPI_F16) {
            *(f16x8*)((f16*)p.out + (size_t)m * p.ldo + col) = v;
          } else if constexpr (EPI == VIDIL_EPI_ARENA) {
            const int b = m / p.T, t = m - b * p.T;
            const size_t hd = (size_t)p.H * 64;
            f16* base = (f16*)(part == 0 ? p.q : part == 1 ? p.k : p.vt) + head * 64 + ch * 8;
            *(f16x8*)(base + (part == 0 ? (size_t)m : (size_t)(p.t_off + t) * p.arena_rows + (size_t)b * p.slot_stride) * hd) = v;
          } else {
            const int b = m / p.T, t = m - b * p.T;
            const size_t bh = (size_t)b * p.H + head;
            if (part == 0) {
              *(f16x8*)((f16*)p.q + (bh * p.Tq_cap + t) * 64 + ch * 8) = v;
            } else {
              f16* kv = (f16*)(part == 1 ? p.k : p.vt);
              if (p.kv_tiled) {   // K in fragment tiles: the lane's 8 columns are one 16-B slot of its key's row
                *(f16x8*)(kv + bh * p.Tk_cap * 64 + ktile_off(p.t_off + t, ch * 8)) = v;
              } else {
                *(f16x8*)(kv + (bh * p.Tk_cap + p.t_off + t) * 64 + ch * 8) = v;
              }
            }
          }
        }
      }
    }
#endif
  } else {
    // ---- f32 rows of 64 columns, four passes of 32 rows: [32][64] floats, chunk XOR (row&7) ------------
    f32x4 rln_g = {1.f, 1.f, 1.f, 1.f}, rln_b = {0.f, 0.f, 0.f, 0.f};
    if constexpr (RLN) {
      const int col = n_w + (lane & 15) * 4;
      if (col + 4 <= N) {
        rln_g = *(const f32x4*)(p.rln_gamma + col);
        rln_b = *(const f32x4*)(p.rln_beta + col);
      }
    }
    if constexpr (EPI == VIDIL_EPI_F32) {
      // Round 4: the epilogue of a one-wave-per-SIMD kernel costs its INSTRUCTION COUNT (one issue slot of ~4-5 cycles per
      // instruction of any kind, nobody else on the SIMD to fill them, the matrix pipe idle throughout): the round-3 form of
      // this path executed ~5,800 instructions per 256 x 256 tile — 29 k cycles, as long as a K = 768 main loop — of which
      // only ~1,500 were arithmetic on the tile; the rest were per-access bounds tests (exec-mask save / branch / restore),
      // 64-bit address multiplies, clamps, selects and a 16-lane DPP reduction per row and statistic.  Here:
      //   * every global access is a RAW BUFFER instruction on a descriptor over this wave's block of rows: a 32-bit lane
      //     offset (stepped with one v_add per row group), no 64-bit address arithmetic, and the hardware's range check
      //     as the bounds test — rows past M lie beyond num_records, a lane whose columns lie past N carries an offset of
      //     2^31: loads return 0 and stores are dropped, so the path is branch-free for full and ragged tiles alike;
      //   * the per-row LayerNorm partials of a pass — 8 rows x (sum, sum of squares) per lane, each to be summed over the
      //     16 lanes that hold the row's 64 columns — go through ONE 16 x 16 reduce-scatter (row16_reduce_scatter: 15
      //     DPP adds) instead of 16 all-reduces (64 DPP moves + 64 adds), and are written by one store instruction.
#ifndef VIDIL_EPI_F32_AHEAD
#define VIDIL_EPI_F32_AHEAD 1
#endif
      constexpr int AH = VIDIL_EPI_F32_AHEAD;      // passes of residual rows in flight ahead of the one being stored (developer sweep: 2 spills)
      const int ch = lane & 15;
      const uint32_t pitch = (uint32_t)p.ldo * 4u;
      const int rows_w = M - m_w < 32 * NIT ? M - m_w : 32 * NIT;                    // (uniform; <= 0 for a block past the end)
      const uint32_t nrows = rows_w > 0 ? (uint32_t)rows_w : 0u;
      const size_t e0 = (size_t)m_w * p.ldo + n_w;                                   // first element of the block
      const bool has_res = p.resid != nullptr, has16 = p.out16 != nullptr;           // (uniform)
      // out16_split3 (parity precision mode, round 5; plain instantiations only): the 16-bit copy is the NEXT compensated GEMM's
      // operand row [hi | lo | hi] (three planes ldo16 / 3 apart: hi = T16(v), lo = T16(v - hi)), and `out` may be NULL — the f32
      // rows are then not written at all (an empty descriptor drops the stores): fc1 + GELU hands its result to fc2 without the
      // f32 round trip through vidil_split3_f32 (8.7 GB written + read back per ViT block at 3,584 frames)
      const bool s3 = !STATS && !RLN && p.out16_split3 != 0;                          // (uniform)
      const bool s3_third = p.out16_split3 != 2;    // (2: planes hi | lo only — the consumer is a split_k launch in the K-loop form, which never reads plane 2)
      const uint32_t pl16 = (uint32_t)(p.ldo16 / 3) * 2u;
      const __amdgpu_buffer_rsrc_t r_out = uniform_rsrc((char*)p.out + e0 * 4, p.out != nullptr ? nrows * pitch : 0u);
      const __amdgpu_buffer_rsrc_t r_res = uniform_rsrc((const char*)(has_res ? p.resid : (const float*)p.out) + e0 * 4, has_res ? nrows * pitch : 0u);
      const uint32_t pitch16 = (uint32_t)p.ldo16 * 2u;
      const __amdgpu_buffer_rsrc_t r_16 = uniform_rsrc((char*)p.out16 + (has16 ? ((size_t)m_w * p.ldo16 + n_w) * 2 : 0), has16 ? nrows * pitch16 : 0u);
      const bool colok = n_w + ch * 4 + 4 <= N;
      // lane offsets of row (lane >> 4) of a pass; + 4 rows per step.  (2^31 + anything a block can add stays >= 2^31 > num_records)
      const uint32_t vo0 = colok ? (uint32_t)(lane >> 4) * pitch + (uint32_t)ch * 16u : 0x80000000u;
      const uint32_t vo16_0 = colok ? (uint32_t)(lane >> 4) * pitch16 + (uint32_t)ch * 8u : 0x80000000u;
      f32x4 addb[AH + 1][8];
      // ONE running offset per stream (residual loads, f32 stores, 16-bit stores), advanced by 4 rows per access and simply
      // continuing from pass to pass: offsets formed as `first + pass * 32 * pitch` made the compiler keep a dozen
      // multiples of the three pitches in SGPRs across the whole tile loop — and the kernel has none to spare: they were
      // spilled to lanes of a VGPR taken from the main loop, which then reloaded a fragment address from scratch (with
      // an `s_waitcnt vmcnt(0)`) in EVERY iteration: +16 % on the residual-LayerNorm instantiation (measured)
      uint32_t vo_ld = vo0, vo_st = vo0, vo16 = vo16_0;
      const uint32_t step = 4u * pitch, step16 = 4u * pitch16;
      auto load_rows = [&](f32x4 (&a8)[8]) {
#pragma unroll
        for (int iter = 0; iter < 8; ++iter) {
          a8[iter] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_res, vo_ld, 0, 0));
          vo_ld += step;
        }
      };
      // (no uniform branch on has_res / has16 either: without a residual the descriptor is empty and the loads return 0;
      //  branches cut the pass into basic blocks and the register allocator then spilled the rows in flight)
#pragma unroll
      for (int a = 0; a < AH; ++a)
        if (a < NIT) load_rows(addb[a]);
#pragma unroll
      for (int pass = 0; pass < NIT; ++pass) {
        if (pass + AH < NIT) load_rows(addb[(pass + AH) % (AH + 1)]);
        {
          const int it = pass;
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int lr = vw_row(j);
            f32x4 q4[4];
            quadrow(it, j, q4);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) *(f32x4*)(ep + lr * 256 + ((vw_cq(j, rq) ^ (lr & 7)) << 4)) = q4[rq];
          }
        }
        f32x4 vrow[8];
#pragma unroll
        for (int iter = 0; iter < 8; ++iter) {
          const int lr = iter * 4 + (lane >> 4);
          vrow[iter] = *(const f32x4*)(ep + lr * 256 + ((ch ^ (lr & 7)) << 4));
        }
        // RLN: row lr's statistics live in lane lr (st_s / st_ss are per MFMA row l31) — all 16 lane permutes of the pass
        // are issued together, ahead of the loop (one LDS round trip per pass, not one per row)
        float rs8[8], mrs8[8];
        if constexpr (RLN) {
#pragma unroll
          for (int iter = 0; iter < 8; ++iter) {
            const int lr = iter * 4 + (lane >> 4);
            rs8[iter] = __shfl(st_s[pass], lr, 64);
            mrs8[iter] = __shfl(st_ss[pass], lr, 64);
          }
        }
        float part[16];   // STATS: [0..7] row sums, [8..15] row sums of squares of this lane's 4 columns, rows iter*4 + (lane >> 4)
#pragma unroll
        for (int iter = 0; iter < 8; ++iter) {
          f32x4 v = vrow[iter];
          {
            f32x4 ad = addb[pass % (AH + 1)][iter];
            if constexpr (RLN) {
              // the residual row is the RAW sum of the previous post-LN block: normalise it here
              const float rs = rs8[iter], mrs = mrs8[iter];
#pragma unroll
              for (int e = 0; e < 4; ++e) ad[e] = __builtin_fmaf(__builtin_fmaf(ad[e], rs, -mrs), rln_g[e], rln_b[e]);
            }
            v += ad;
          }
          if constexpr (STATS) {   // LN-fold producer — this lane's share of (sum, sum of squares) of the row's 64 columns
            part[iter] = (v[0] + v[1]) + (v[2] + v[3]);
            part[8 + iter] = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
          }
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r_out, vo_st, 0, 0);
          if (STATS || has16) {   // the raw stream in the operand type, for the LN-folded consumer GEMM (a producer of row partials always writes it)
            const f16x4 h4 = {Elt<TO>::from_f32(v[0]), Elt<TO>::from_f32(v[1]), Elt<TO>::from_f32(v[2]), Elt<TO>::from_f32(v[3])};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h4), r_16, vo16, 0, 0);
            if constexpr (!STATS && !RLN) {
              if (s3) {
                const f16x4 l4 = {Elt<TO>::from_f32(v[0] - (float)h4[0]), Elt<TO>::from_f32(v[1] - (float)h4[1]),
                                  Elt<TO>::from_f32(v[2] - (float)h4[2]), Elt<TO>::from_f32(v[3] - (float)h4[3])};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, l4), r_16, vo16 + pl16, 0, 0);
                // (no branch: a lane offset of 2^31 is past every descriptor's range — the store is dropped by the range check)
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, h4), r_16, s3_third ? vo16 + 2u * pl16 : 0x80000000u, 0, 0);
              }
            }
          }
          vo_st += step;
          vo16 += step16;
        }
        if constexpr (STATS) {
          // lane i of every 16 now gets value i summed over the 16: (sum | sum of squares) of row (i & 7) * 4 + (lane >> 4)
          const float tot = row16_reduce_scatter(part, lane);
          const int m = m_w + pass * 32 + (lane & 7) * 4 + (lane >> 4);
          if (m < M) p.ln_stats_out[((size_t)m * (N >> 6) + (n_w >> 6)) * 2 + ((lane >> 3) & 1)] = tot;   // (one store per pass)
        }
      }
    } else {
#ifdef VIDIL_EPI_LAZY
    // One wave per SIMD: nobody covers a global-load latency for this wave, so the residual / position rows are fetched
    // ONE PASS AHEAD (two register sets), raw — the residual LayerNorm is applied where the row is consumed, after the LDS
    // round trip, not right behind the load (that would stall on the load's latency once per pass).
#ifndef VIDIL_EPI_AHEAD
#define VIDIL_EPI_AHEAD 1      // passes of residual rows in flight ahead of the one being stored (developer sweep: 1 or 2)
#endif
    constexpr int AH = VIDIL_EPI_AHEAD;
    f32x4 addb[AH + 1][8];
    // (no per-lane bounds branch around the loads either: row and column are clamped into the matrix — rows / columns
    //  past the end are never stored — so the compiler sees straight-line loads and waits for them with COUNTED vmcnt)
    auto load_rows = [&](int pass, f32x4 (&a8)[8]) {
      const int ch = lane & 15;
      const int col = n_w + ch * 4;
      const int colc = col + 4 <= N ? col : N - 4;
#pragma unroll
      for (int iter = 0; iter < 8; ++iter) a8[iter] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (EPI != VIDIL_EPI_F32 || p.resid != nullptr) {   // (uniform)
#pragma unroll
        for (int iter = 0; iter < 8; ++iter) {
          const int lr = iter * 4 + (lane >> 4);
          const int m = m_w + pass * 32 + lr;
          const int mc = m < M ? m : M - 1;
          if constexpr (EPI == VIDIL_EPI_F32) {
            a8[iter] = *(const f32x4*)(p.resid + (size_t)mc * p.ldo + colc);
          } else {  // EPI_PATCH
            const int t = mc % p.tpi;
            a8[iter] = *(const f32x4*)(p.pos + (size_t)(t + 1) * N + colc);
          }
        }
      }
    };
#pragma unroll
    for (int a = 0; a < AH; ++a)
      if (a < NIT) load_rows(a, addb[a]);
#pragma unroll
    for (int pass = 0; pass < NIT; ++pass) {
      if (pass + AH < NIT) load_rows(pass + AH, addb[(pass + AH) % (AH + 1)]);
      {
        const int it = pass;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int lr = vw_row(j);
          f32x4 q4[4];
          quadrow(it, j, q4);
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) *(f32x4*)(ep + lr * 256 + ((vw_cq(j, rq) ^ (lr & 7)) << 4)) = q4[rq];
        }
      }
      const int ch = lane & 15;
      f32x4 vrow[8];
#pragma unroll
      for (int iter = 0; iter < 8; ++iter) {
        const int lr = iter * 4 + (lane >> 4);
        vrow[iter] = *(const f32x4*)(ep + lr * 256 + ((ch ^ (lr & 7)) << 4));
      }
      // RLN: row lr's statistics live in lane lr (st_s / st_ss are per MFMA row l31) — all 16 lane permutes of the pass
      // are issued together, ahead of the loop (one LDS round trip per pass, not one per row)
      float rs8[8], mrs8[8];
      if constexpr (RLN) {
#pragma unroll
        for (int iter = 0; iter < 8; ++iter) {
          const int lr = iter * 4 + (lane >> 4);
          rs8[iter] = __shfl(st_s[pass], lr, 64);
          mrs8[iter] = __shfl(st_ss[pass], lr, 64);
        }
      }
#pragma unroll
      for (int iter = 0; iter < 8; ++iter) {
        const int lr = iter * 4 + (lane >> 4);
        f32x4 v = vrow[iter];
        f32x4 ad = addb[pass % (AH + 1)][iter];
        if constexpr (RLN) {
          // the residual row is the RAW sum of the previous post-LN block: normalise it here
          const float rs = rs8[iter], mrs = mrs8[iter];
#pragma unroll
          for (int e = 0; e < 4; ++e) ad[e] = __builtin_fmaf(__builtin_fmaf(ad[e], rs, -mrs), rln_g[e], rln_b[e]);
        }
        const int m = m_w + pass * 32 + lr;
        const int col = n_w + ch * 4;
        const bool ok = m < M && col + 4 <= N;
        if (ok) v += ad;
        if constexpr (EPI == VIDIL_EPI_F32 && STATS) {
          {   // LN-fold producer — (sum, sum of squares) of this row's 64 columns
            const f32x4 z = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            const float s = row16_sum((z[0] + z[1]) + (z[2] + z[3]));
            const float ss = row16_sum((z[0] * z[0] + z[1] * z[1]) + (z[2] * z[2] + z[3] * z[3]));
            if (ch == 0 && m < M) *(f32x2*)(p.ln_stats_out + ((size_t)m * (N >> 6) + (n_w >> 6)) * 2) = f32x2{s, ss};
          }
        }
        if (ok) {
          if constexpr (EPI == VIDIL_EPI_F32) {
            *(f32x4*)((float*)p.out + (size_t)m * p.ldo + col) = v;
            if (p.out16 != nullptr) {   // the raw stream in the operand type, for the LN-folded consumer GEMM
              const f16x4 h4 = {Elt<TO>::from_f32(v[0]), Elt<TO>::from_f32(v[1]), Elt<TO>::from_f32(v[2]), Elt<TO>::from_f32(v[3])};
              *(f16x4*)((f16*)p.out16 + (size_t)m * p.ldo16 + col) = h4;
            }
          } else {  // EPI_PATCH
            const int b = m / p.tpi;
            *(f32x4*)((float*)p.out + ((size_t)m + b + 1) * p.ldo + col) = v;
          }
        }
      }
    }
#else
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      // residual / position rows of this pass: all 8 loads of a lane go out before the LDS round trip, so
      // their latency is paid once per pass (the dependent load -> add -> store chain paid it per group)
      f32x4 add[8];
      {
        const int ch = lane & 15;
        const int col = n_w + ch * 4;
#pragma unroll
        for (int iter = 0; iter < 8; ++iter) {
          const int lr = iter * 4 + (lane >> 4);
          const int m = m_w + pass * 32 + lr;
          add[iter] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (m < M && col + 4 <= N) {
            if constexpr (EPI == VIDIL_EPI_F32) {
              if (p.resid != nullptr) add[iter] = *(const f32x4*)(p.resid + (size_t)m * p.ldo + col);
            } else {  // EPI_PATCH
              const int t = m % p.tpi;
              add[iter] = *(const f32x4*)(p.pos + (size_t)(t + 1) * N + col);
            }
          }
          if constexpr (RLN) {
            // the residual row is the RAW sum of the previous post-LN block: normalise it here.  Row lr's statistics
            // live in lane lr (st_s / st_ss are per MFMA row l31) — fetched by every lane, outside the bounds test.
            const float rs = __shfl(st_s[pass], lr, 64), mrs = __shfl(st_ss[pass], lr, 64);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              add[iter][e] = __builtin_fmaf(__builtin_fmaf(add[iter][e], rs, -mrs), rln_g[e], rln_b[e]);
          }
        }
      }
      {
        const int it = pass;
        const int lr = l31;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 q4[4];
          quadrow(it, j, q4);
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) *(f32x4*)(ep + lr * 256 + (((j * 8 + rq * 2 + hi) ^ (lr & 7)) << 4)) = q4[rq];
        }
      }
      const int ch = lane & 15;
#ifdef VIDIL_EPI_LAZY
      f32x4 vrow[8];
#pragma unroll
      for (int iter = 0; iter < 8; ++iter) {
        const int lr = iter * 4 + (lane >> 4);
        vrow[iter] = *(const f32x4*)(ep + lr * 256 + ((ch ^ (lr & 7)) << 4));
      }
#endif
#pragma unroll
      for (int iter = 0; iter < 8; ++iter) {
        const int lr = iter * 4 + (lane >> 4);
#ifdef VIDIL_EPI_LAZY
        f32x4 v = vrow[iter];
#else
        f32x4 v = *(const f32x4*)(ep + lr * 256 + ((ch ^ (lr & 7)) << 4));
#endif
        const int m = m_w + pass * 32 + lr;
        const int col = n_w + ch * 4;
        const bool ok = m < M && col + 4 <= N;
        if (ok) v += add[iter];
        if constexpr (EPI == VIDIL_EPI_F32 && STATS) {
          {   // LN-fold producer — (sum, sum of squares) of this row's 64 columns
            const f32x4 z = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            const float s = row16_sum((z[0] + z[1]) + (z[2] + z[3]));
            const float ss = row16_sum((z[0] * z[0] + z[1] * z[1]) + (z[2] * z[2] + z[3] * z[3]));
            if (ch == 0 && m < M) *(f32x2*)(p.ln_stats_out + ((size_t)m * (N >> 6) + (n_w >> 6)) * 2) = f32x2{s, ss};
          }
        }
        if (ok) {
          if constexpr (EPI == VIDIL_EPI_F32) {
            *(f32x4*)((float*)p.out + (size_t)m * p.ldo + col) = v;
            if (p.out16 != nullptr) {   // the raw stream in the operand type, for the LN-folded consumer GEMM
              const f16x4 h4 = {Elt<TO>::from_f32(v[0]), Elt<TO>::from_f32(v[1]), Elt<TO>::from_f32(v[2]), Elt<TO>::from_f32(v[3])};
              *(f16x4*)((f16*)p.out16 + (size_t)m * p.ldo16 + col) = h4;
            }
          } else {  // EPI_PATCH
            const int b = m / p.tpi;
            *(f32x4*)((float*)p.out + ((size_t)m + b + 1) * p.ldo + col) = v;
          }
        }
      }
    }
#endif
    }
  }
