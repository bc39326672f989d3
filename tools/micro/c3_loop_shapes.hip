// Developer microbenchmark: the compensated (C3) GEMM iteration's instruction mix of gemm4w.hip in the two MFMA shapes,
// v_mfma_f32_32x32x16 (what the library issues) and v_mfma_f32_16x16x32.  One wave per SIMD, a 128 x 128 block per wave,
// every fragment re-read by ds_read_b128 from an LDS image in the kernel's layout (128-byte rows [hi 64 B | lo 64 B], 16-byte
// slot XOR (row >> 1) & 7), three products per 32 columns (hi.hi, hi.lo, lo.hi), random f16 operands (lo = 2^-11 of hi), two
// images alternating like the kernel's ring, no global traffic and no barrier in the loop.  The chip holds its clock down
// under such a loop and the clock it holds depends on the shape, so both wall time and wave cycles are printed; zeros or
// trivial operands would rank the shapes by cycles only.
// Second question, printed at the end (a sample, not a proof): is ONE 16x16x32 accumulation bit-equal to TWO chained
// 32x32x16 over the same 32 k, on random f16 / bf16 data?
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/micro/c3_loop_shapes.bin tools/micro/c3_loop_shapes.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

typedef _Float16 f16;
typedef __bf16 bf16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CHECK(x)                                                                                   \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; }    \
  } while (0)

template <class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

constexpr int SLOT = 16384;            // one half-tile: 128 rows x 128 B
constexpr int BUF = 4 * SLOT;          // A0, A1, W0, W1
constexpr int LDS_BYTES = 2 * BUF;     // two images

__device__ __forceinline__ void fill_image(char* smem) {
  // logical 16-byte slot s of row r lives at physical slot s ^ ((r >> 1) & 7); logical slots 0-3 = hi plane, 4-7 = lo plane
  unsigned h = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 12345u;
  for (int c = threadIdx.x; c < LDS_BYTES / 16; c += 256) {
    const int row = (c >> 3) & 127, phys = c & 7;
    const int logical = phys ^ ((row >> 1) & 7);
    const float scale = logical < 4 ? 1.0f / 1024.0f : 1.0f / (1024.0f * 2048.0f);
    f16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      h = h * 1664525u + 1013904223u;
      v[e] = (f16)(((int)(h >> 8) % 2048 - 1024) * scale);
    }
    *(f16x8*)(smem + c * 16) = v;
  }
  __syncthreads();
}

// SHAPE 32: the library's C3 iteration (gemm4w.hip iteration_c3, TM = 4) without its barriers and DMA pieces: 96 MFMAs of
// 32 cycles, 32 fragment reads.  SHAPE 16: the same products as 192 MFMAs of 16 cycles, 32 fragment reads.
template <int SHAPE>
__global__ __launch_bounds__(256) void c3_loop(float* out, unsigned long long* stamps, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  fill_image(smem);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wave >> 1, wc2 = wave & 1;
  int cb = 0;
  unsigned long long t0 = 0, r0 = 0, t1 = 0, r1 = 0;
  float s = 0.f;
  if constexpr (SHAPE == 32) {
    const int hi = lane >> 5, l31 = lane & 31, sw = (l31 >> 1) & 7;
    const int a_off = grp * SLOT + l31 * 128, w_off = (2 + wc2) * SLOT + l31 * 128;
    f32x16 acc[4][4];
    f16x8 fa[4][4], fw[4][4];
    static_for<16>([&](auto t) {
      constexpr int n = decltype(t)::value;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n >> 2][n & 3][r] = 0.f;
    });
    auto read_frag = [&](const char* buf, int ks, int r) {
      if (r < 4) fw[ks][r] = *(const f16x8*)(buf + w_off + r * 4096 + (((ks * 2 + hi) ^ sw) << 4));
      else fa[ks][r - 4] = *(const f16x8*)(buf + a_off + (r - 4) * 4096 + (((ks * 2 + hi) ^ sw) << 4));
    };
    static_for<16>([&](auto t) {
      constexpr int f = decltype(t)::value;
      read_frag(smem, f / 8, f % 8);
    });
    t0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
      const char* const buf = smem + cb * BUF;
      const char* const nbuf = smem + (cb ^ 1) * BUF;
      static_for<96>([&](auto t) {
        constexpr int n = decltype(t)::value;
        constexpr int pr = n / 16, i = (n >> 2) % 4, j = n & 3;
        constexpr int ka = pr == 0 ? 0 : pr == 1 ? 1 : pr == 2 ? 0 : pr == 3 ? 1 : pr == 4 ? 2 : 3;
        constexpr int kw = pr == 0 ? 0 : pr == 1 ? 1 : pr == 2 ? 2 : pr == 3 ? 3 : pr == 4 ? 0 : 1;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[kw][j], fa[ka][i], acc[i][j], 0, 0, 0);
        if constexpr (n < 4) read_frag(buf, 1, n);
        if constexpr (n >= 4 && n < 20) read_frag(buf, 2 + (n - 4) / 8, (n - 4) % 8);
        if constexpr (n >= 64 && n < 72) read_frag(nbuf, (n - 64) / 4, 4 + (n - 64) % 4);
        if constexpr (n >= 80 && n < 84) read_frag(nbuf, 0, n - 80);
        __builtin_amdgcn_sched_barrier(0);
      });
      cb ^= 1;
    }
    t1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    static_for<16>([&](auto t) {
      constexpr int n = decltype(t)::value;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += acc[n >> 2][n & 3][r];
    });
  } else {
    const int kq = lane >> 4, l15 = lane & 15, sw = (l15 >> 1) & 7;
    // (16-row tiles: 2 KiB apart; a wave's 128 rows of A / of W are the 8 tiles of its half-tile)
    const int a_off = grp * SLOT + l15 * 128, w_off = (2 + wc2) * SLOT + l15 * 128;
    f32x4 acc[8][8];
    f16x8 fa[2][8], fw[2][8];    // [plane][16-row tile]
    static_for<64>([&](auto t) {
      constexpr int n = decltype(t)::value;
      acc[n >> 3][n & 7] = f32x4{0.f, 0.f, 0.f, 0.f};
    });
    auto read_a = [&](const char* buf, int pl, int t) { fa[pl][t] = *(const f16x8*)(buf + a_off + t * 2048 + (((pl * 4 + kq) ^ sw) << 4)); };
    auto read_w = [&](const char* buf, int pl, int t) { fw[pl][t] = *(const f16x8*)(buf + w_off + t * 2048 + (((pl * 4 + kq) ^ sw) << 4)); };
    static_for<8>([&](auto t) {
      constexpr int f = decltype(t)::value;
      read_a(smem, 0, f);
      read_w(smem, 0, f);
    });
    t0 = __builtin_amdgcn_s_memtime();
    r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
      const char* const buf = smem + cb * BUF;
      const char* const nbuf = smem + (cb ^ 1) * BUF;
      static_for<192>([&](auto t) {
        constexpr int n = decltype(t)::value;
        constexpr int pr = n / 64, nj = (n >> 3) & 7, mi = n & 7;
        constexpr int pa = pr == 2 ? 1 : 0, pw = pr == 1 ? 1 : 0;
        {
          // (as in the library: the instruction itself, accumulator pinned to the AGPRs — through the builtin hipcc spreads the
          //  64 four-register accumulators over both register files and moves them about: 588 v_accvgpr copies per iteration)
          f32x4& c_ = acc[mi][nj];
          const f16x8& w_ = fw[pw][nj];
          const f16x8& a_ = fa[pa][mi];
          asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c_) : "v"(w_), "v"(a_));
        }
        if constexpr (n == 0) read_w(buf, 0, 7);                                   // (deferred: feeds the last MFMAs of the iteration before)
        if constexpr (n >= 1 && n < 9) read_w(buf, 1, n - 1);
        if constexpr (n >= 9 && n < 17) read_a(buf, 1, n - 9);
        if constexpr (n >= 128 && n < 136) read_a(nbuf, 0, n - 128);
        if constexpr (n >= 136 && (n - 136) % 8 == 0) read_w(nbuf, 0, (n - 136) / 8);
        __builtin_amdgcn_sched_barrier(0);
      });
      cb ^= 1;
    }
    t1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");      // (the compiler does not see the MFMAs: their results are read below)
    static_for<64>([&](auto t) {
      constexpr int n = decltype(t)::value;
      s += acc[n >> 3][n & 7][0] + acc[n >> 3][n & 7][1] + acc[n >> 3][n & 7][2] + acc[n >> 3][n & 7][3];
    });
  }
  if (s == 12345.678f) out[0] = s;
  if (lane == 0) {      // stamps go to a buffer of their own
    stamps[(blockIdx.x * 4 + wave) * 2] = t1 - t0;
    stamps[(blockIdx.x * 4 + wave) * 2 + 1] = r1 - r0;
  }
}

template <int SHAPE>
int run(int iters, int nblk, float* d_out, unsigned long long* d_st) {
  auto kern = c3_loop<SHAPE>;
  CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), LDS_BYTES, 0, d_out, d_st, iters / 4);    // warm: the clock settles under load
  CHECK(hipDeviceSynchronize());
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(256), LDS_BYTES, 0, d_out, d_st, iters);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<unsigned long long> st(nblk * 8);
  CHECK(hipMemcpy(st.data(), d_st, st.size() * 8, hipMemcpyDeviceToHost));
  std::vector<double> cyc, ghz;
  for (int w = 0; w < nblk * 4; ++w) {
    cyc.push_back((double)st[w * 2]);
    ghz.push_back(st[w * 2 + 1] ? (double)st[w * 2] / (double)st[w * 2 + 1] * 0.1 : 0.0);
  }
  std::sort(cyc.begin(), cyc.end());
  std::sort(ghz.begin(), ghz.end());
  const double flop = (double)nblk * 4 * iters * 3.0 * 2.0 * 128 * 128 * 32;
  printf("  %s: wall %8.2f ms  %7.1f TFLOP/s | wave cycles (median) %.4e = %.1f per iteration | in-kernel clock %.3f GHz\n",
         SHAPE == 32 ? "32x32x16" : "16x16x32", ms, flop / ms / 1e9, cyc[cyc.size() / 2], cyc[cyc.size() / 2] / iters, ghz[ghz.size() / 2]);
  CHECK(hipEventDestroy(e0));
  CHECK(hipEventDestroy(e1));
  return 0;
}

// ---- bit-equality sample: D = C + A[32 x 32k] . B[32 x 32k]^T, two chained 32x32x16 against four 16x16x32 -----------------
template <typename T> struct Op;
template <> struct Op<f16> {
  typedef f16x8 x8;
  static __device__ f32x16 m32(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
  static __device__ f32x4 m16(x8 a, x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct Op<bf16> {
  typedef bf16x8 x8;
  static __device__ f32x16 m32(x8 a, x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
  static __device__ f32x4 m16(x8 a, x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// one wave per tile; A, B: [tile][32 rows][32 k] of T, C: [tile][32][32] f32 (or none); D32 / D16: [tile][32][32] f32
template <typename T>
__global__ __launch_bounds__(64) void shape_bits(const T* A, const T* B, const float* C, float* D32, float* D16) {
  typedef typename Op<T>::x8 x8;
  const int lane = threadIdx.x;
  const size_t tb = (size_t)blockIdx.x * 1024;
  {
    const int row = lane & 31, h = lane >> 5;
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = C ? C[tb + ((r >> 2) * 8 + h * 4 + (r & 3)) * 32 + row] : 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const x8 a = *(const x8*)(A + tb + row * 32 + st * 16 + h * 8);
      const x8 b = *(const x8*)(B + tb + row * 32 + st * 16 + h * 8);
      c = Op<T>::m32(a, b, c);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) D32[tb + ((r >> 2) * 8 + h * 4 + (r & 3)) * 32 + row] = c[r];
  }
  {
    const int row = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        f32x4 c;
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = C ? C[tb + (ti * 16 + kq * 4 + r) * 32 + tj * 16 + row] : 0.f;
        const x8 a = *(const x8*)(A + tb + (ti * 16 + row) * 32 + kq * 8);
        const x8 b = *(const x8*)(B + tb + (tj * 16 + row) * 32 + kq * 8);
        c = Op<T>::m16(a, b, c);
#pragma unroll
        for (int r = 0; r < 4; ++r) D16[tb + (ti * 16 + kq * 4 + r) * 32 + tj * 16 + row] = c[r];
      }
  }
}

template <typename T>
int bits_sample(const char* name) {
  const int tiles = 4096;
  const size_t n = (size_t)tiles * 1024;
  std::vector<T> a(n), b(n);
  std::vector<float> c(n), d32(n), d16(n);
  unsigned h = 777u;
  auto rnd = [&]() { h = h * 1664525u + 1013904223u; return ((int)(h >> 8) % 65536 - 32768) / 32768.0f; };
  for (size_t i = 0; i < n; ++i) {
    // mantissas and exponents both vary, so that products need rounding when they are added
    const float ea = (float)(1 << ((h >> 3) & 7)), eb = (float)(1 << ((h >> 13) & 7));
    a[i] = (T)(rnd() / ea);
    b[i] = (T)(rnd() / eb);
    c[i] = rnd() * 4.0f;
  }
  T *dA, *dB;
  float *dC, *dD32, *dD16;
  CHECK(hipMalloc(&dA, n * sizeof(T)));
  CHECK(hipMalloc(&dB, n * sizeof(T)));
  CHECK(hipMalloc(&dC, n * 4));
  CHECK(hipMalloc(&dD32, n * 4));
  CHECK(hipMalloc(&dD16, n * 4));
  CHECK(hipMemcpy(dA, a.data(), n * sizeof(T), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dB, b.data(), n * sizeof(T), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dC, c.data(), n * 4, hipMemcpyHostToDevice));
  for (int with_c = 0; with_c < 2; ++with_c) {
    hipLaunchKernelGGL(shape_bits<T>, dim3(tiles), dim3(64), 0, 0, dA, dB, with_c ? dC : (const float*)nullptr, dD32, dD16);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(d32.data(), dD32, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(d16.data(), dD16, n * 4, hipMemcpyDeviceToHost));
    size_t diff = 0;
    double maxd = 0.0;
    for (size_t i = 0; i < n; ++i) {
      if (memcmp(&d32[i], &d16[i], 4) != 0) {
        ++diff;
        maxd = std::max(maxd, (double)fabsf(d32[i] - d16[i]));
      }
    }
    printf("  %s, C %s: %zu of %zu elements differ in bits (max |d| %.3e): one 16x16x32 is %s two chained 32x32x16 on this sample\n", name,
           with_c ? "random" : "zero", diff, n, maxd, diff ? "NOT bit-equal to" : "bit-equal to");
  }
  CHECK(hipFree(dA));
  CHECK(hipFree(dB));
  CHECK(hipFree(dC));
  CHECK(hipFree(dD32));
  CHECK(hipFree(dD16));
  return 0;
}

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int nblk = prop.multiProcessorCount;      // one workgroup of 4 waves per CU
  const int iters = 450000;                       // >= 0.5 s per arm: 96 x 32 = 192 x 16 = 3,072 matrix-pipe cycles per iteration
  float* d_out;
  unsigned long long* d_st;
  CHECK(hipMalloc(&d_out, 4));
  CHECK(hipMalloc(&d_st, (size_t)nblk * 4 * 2 * 8));
  printf("C3 iteration, one wave per SIMD, 128 x 128 per wave, fragments from LDS, random f16 (%d workgroups, %d iterations):\n", nblk, iters);
  for (int rep = 0; rep < 3; ++rep) {
    printf(" repetition %d\n", rep);
    if (run<32>(iters, nblk, d_out, d_st)) return 1;
    if (run<16>(iters, nblk, d_out, d_st)) return 1;
  }
  printf("one 16x16x32 against two chained 32x32x16 over the same 32 k:\n");
  if (bits_sample<f16>("f16")) return 1;
  if (bits_sample<bf16>("bf16")) return 1;
  CHECK(hipFree(d_out));
  CHECK(hipFree(d_st));
  return 0;
}
