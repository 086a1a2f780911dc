// Int4 weight-only linear for decode-sized batches, gfx950:
//   y[M,N] = x[M,K] . w_hat^T,   w_hat[n,k] = float(scale[n, k/128]) * q[n,k]
// x, y bf16; q in [-8,7], 4 bits; scale bf16, one per group of 128 k.
//
// Packed format (ops.quantize_w4 writes it, ops.dequantize_w4 inverts it):
//   qweight int32 [N, K/8], word w of row n holds k = 8w .. 8w+7 — words in
//   natural order, no interleave across a row.  A weight is stored as the
//   unsigned nibble u = q + 8.  Inside a word, k offset j sits at nibble
//   position  j/2  for even j  and  4 + j/2  for odd j:
//       bits  3..0  k+0     bits 19..16  k+1
//       bits  7..4  k+2     bits 23..20  k+3
//       bits 11..8  k+4     bits 27..24  k+5
//       bits 15..12 k+6     bits 31..28  k+7
//   so (word >> 4i) & 0x000F000F is the pair (k+2i, k+2i+1) already in the
//   two halves of a dword, which is where a bf16x8 fragment wants them.
//   scales bf16 [N, K/128].
//
// Integer-to-bf16 route: the exponent-bias form.  0x4300 | u is the bf16
// value 128 + u = 136 + q, so one v_lshrrev and one v_and_or_b32 make two B
// operands — 7 VALU instructions per 8 weights.  gfx950 has no packed
// int4/int8 -> bf16 convert; the direct route (v_bfe_i32, v_cvt_f32_i32,
// v_cvt_pk_bf16_f32) costs 20 per 8 weights, which at one wave per SIMD is
// more VALU time than the weight bytes take to arrive.  The bias leaves in
// fp32, once per group: with P_g = sum_k x * (136 + q) and X_g = sum_k x
// over the group,
//       y += s_g * (P_g - 136 * X_g).
// X_g comes from a third MFMA per k-step against a fragment of ones, which
// lands it in the C layout (row = register, the same in every column) with
// no cross-lane traffic.  The scale multiplies the group's fp32 sum; no
// scale * q product is ever rounded to bf16.
//
// Shape: moe_gemm_kernel's.  A block is ONE wave owning a 32-row M-tile by
// 64 columns (two 32x32 C fragments).  A chunk is one group, 128 k: per lane
// two 16 B loads per N-tile (8 words = 64 weights of its row), eight 16 B
// loads of x, two scales.  The MFMA k order within a chunk is the kernel's
// own: lane half hi5 owns k = hi5*64 .. hi5*64+63 of the chunk, step s
// takes its k 8s..8s+7, for A and B alike — that is what lets the words be
// read as plain 16 B runs (layouts: attention_mfma32.h).  Loads of chunk
// i+1 are issued before the MFMAs of chunk i.
//
// Split-K: K's groups are cut into S contiguous slices; slice z's wave
// writes fp32 partials to ws[z][M][N] and w4_reduce_kernel sums z ascending
// and rounds to bf16 once.  S = 1 writes bf16 from the GEMM epilogue.  S is
// a function of (N, K) only (linear_w4_plan), there are no float atomics and
// a row's sums never see another row: the result of a row is bitwise
// reproducible and independent of M and of the M-tile it falls into.
#include "attention_mfma32.h"

#define W4_BM 32
#define W4_G 128           // quantization group = K-chunk
#define W4_BIAS 136.f      // 128 from the exponent trick + 8 from u = q + 8
// waves the split rule aims for (profiles/linear_w4.txt)
#define W4_TARGET_WAVES 512

struct W4Frags {
  bf16x8 a[8];
  i32x4 b0[2], b1[2];
  unsigned short s0, s1;
};

DEV_INLINE void w4_load(W4Frags& f, const short* pa, const int* p0,
                        const int* p1, const unsigned short* ps0,
                        const unsigned short* ps1, int ch, short keep) {
  const int* w0 = p0 + ch * (W4_G / 8);
  const int* w1 = p1 + ch * (W4_G / 8);
  f.b0[0] = *(const i32x4*)w0;
  f.b0[1] = *(const i32x4*)(w0 + 4);
  f.b1[0] = *(const i32x4*)w1;
  f.b1[1] = *(const i32x4*)(w1 + 4);
  f.s0 = ps0[ch];
  f.s1 = ps1[ch];
  const short* a = pa + ch * W4_G;
  // keep is all ones, or zero on a row past M: a mask, not a select, so the
  // load itself stays unconditional
#pragma unroll
  for (int s = 0; s < 8; ++s) f.a[s] = *(const bf16x8*)(a + s * 8) & keep;
}

// one packed word -> the bf16 fragment {136+q(k+0), ..., 136+q(k+7)}
DEV_INLINE bf16x8 w4_unpack(int word) {
  const unsigned w = (unsigned)word;
  union {
    unsigned d[4];
    bf16x8 v;
  } u;
  u.d[0] = (w & 0x000F000Fu) | 0x43004300u;
  u.d[1] = ((w >> 4) & 0x000F000Fu) | 0x43004300u;
  u.d[2] = ((w >> 8) & 0x000F000Fu) | 0x43004300u;
  u.d[3] = ((w >> 12) & 0x000F000Fu) | 0x43004300u;
  return u.v;
}

// one group: biased products P and row sums X by MFMA, then
// acc += scale * (P - 136 X) in fp32
DEV_INLINE void w4_mma(const W4Frags& f, f32x16& acc0, f32x16& acc1) {
  const short one = 0x3F80;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};
  f32x16 p0, p1, xs;
#pragma unroll
  for (int r = 0; r < 16; ++r) p0[r] = p1[r] = xs[r] = 0.f;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    bf16x8 b0 = w4_unpack(f.b0[s >> 2][s & 3]);
    bf16x8 b1 = w4_unpack(f.b1[s >> 2][s & 3]);
    p0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[s], b0, p0, 0, 0, 0);
    p1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[s], b1, p1, 0, 0, 0);
    xs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[s], ones, xs, 0, 0, 0);
  }
  const float s0 = bf2f((short)f.s0), s1 = bf2f((short)f.s1);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc0[r] = __builtin_fmaf(s0, __builtin_fmaf(-W4_BIAS, xs[r], p0[r]),
                             acc0[r]);
    acc1[r] = __builtin_fmaf(s1, __builtin_fmaf(-W4_BIAS, xs[r], p1[r]),
                             acc1[r]);
  }
}

// grid = mtiles * (N/64) * S, M-tile fastest so the waves that share a
// weight tile run together.  cps = groups per slice.  S == 1: Y bf16 [M,N];
// S > 1: WS f32 [S,M,N].  Left alone the allocator takes 296 registers (one
// wave per SIMD); asked for two waves it fits 242 without a spill, and the
// second wave is what hides a chunk's load latency.
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2)))
void w4_gemm_kernel(
    const short* __restrict__ X, const int* __restrict__ QW,
    const unsigned short* __restrict__ SC, short* __restrict__ Y,
    float* __restrict__ WS, int M, int N, int K, int mtiles, int S, int cps) {
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int ntiles = N / 64;
  const int mtile = blockIdx.x % mtiles;
  const int rest = blockIdx.x / mtiles;
  const int nb = rest % ntiles, z = rest / ntiles;
  const int nch = K / W4_G;
  const int ch0 = z * cps;
  const int ch1 = ch0 + cps < nch ? ch0 + cps : nch;

  const int row = mtile * W4_BM + l31;
  const short keep = row < M ? -1 : 0;
  const size_t a_row = row < M ? (size_t)row : 0;
  const int n0 = nb * 64, n1 = n0 + 32;
  const short* pa = X + a_row * K + hi5 * 64;
  const int* p0 = QW + (size_t)(n0 + l31) * (K / 8) + hi5 * 8;
  const int* p1 = QW + (size_t)(n1 + l31) * (K / 8) + hi5 * 8;
  const unsigned short* ps0 = SC + (size_t)(n0 + l31) * nch;
  const unsigned short* ps1 = SC + (size_t)(n1 + l31) * nch;

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;

  // two register sets in turn, groups ascending: f0 holds group c, f1 c + 1
  W4Frags f0, f1;
  w4_load(f0, pa, p0, p1, ps0, ps1, ch0, keep);
  int c = ch0;
  for (; c + 2 < ch1; c += 2) {
    w4_load(f1, pa, p0, p1, ps0, ps1, c + 1, keep);
    w4_mma(f0, acc0, acc1);
    w4_load(f0, pa, p0, p1, ps0, ps1, c + 2, keep);
    w4_mma(f1, acc0, acc1);
  }
  if (c + 1 < ch1) {
    w4_load(f1, pa, p0, p1, ps0, ps1, c + 1, keep);
    w4_mma(f0, acc0, acc1);
    w4_mma(f1, acc0, acc1);
  } else {
    w4_mma(f0, acc0, acc1);
  }

  // C fragment: register r of this lane is row c_row(r, hi5), column l31
  if (S == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int m = mtile * W4_BM + c_row(r, hi5);
      if (m < M) {
        short* yrow = Y + (size_t)m * N + l31;
        yrow[n0] = f2bf(acc0[r]);
        yrow[n1] = f2bf(acc1[r]);
      }
    }
  } else {
    float* ws = WS + (size_t)z * M * N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int m = mtile * W4_BM + c_row(r, hi5);
      if (m < M) {
        float* wrow = ws + (size_t)m * N + l31;
        wrow[n0] = acc0[r];
        wrow[n1] = acc1[r];
      }
    }
  }
}

// y = bf16(ws[0] + ws[1] + ... + ws[S-1]), slices in ascending order
__global__ __launch_bounds__(256) void w4_reduce_kernel(
    const float* __restrict__ WS, short* __restrict__ Y, long long n4,
    int S) {
  long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += stride) {
    f32x4 acc = *(const f32x4*)&WS[i * 4];
    for (int z = 1; z < S; ++z) {
      f32x4 p = *(const f32x4*)&WS[((long long)z * n4 + i) * 4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += p[q];
    }
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = f2bf(acc[q]);
    *(bf16x4*)&Y[i * 4] = o;
  }
}

// ---------------------------------------------------------------- launchers

static bool w4_shape_ok(long long M, int N, int K) {
  return M >= 1 && M < (1ll << 31) && N >= 64 && N % 64 == 0 && K >= W4_G &&
         K % W4_G == 0;
}

// The number of K slices of a call, 0 for a shape the kernel does not
// support.  splits <= 0 asks for the rule: the smallest S that gives one
// M-tile W4_TARGET_WAVES waves, at most one slice per group — a function of
// (N, K) only, so a row's result does not depend on M.  splits > 0 (tests
// and the benchmark sweep) is taken as given.  Either way S is normalised
// so that no slice is empty.
extern "C" int linear_w4_plan(long long M, int N, int K, int splits) {
  if (!w4_shape_ok(M, N, K)) return 0;
  const int nch = K / W4_G, ntiles = N / 64;
  int S = splits > 0 ? splits : (W4_TARGET_WAVES + ntiles - 1) / ntiles;
  if (S > nch) {
    if (splits > 0) return 0;
    S = nch;
  }
  const int cps = (nch + S - 1) / S;
  return (nch + cps - 1) / cps;
}

// x bf16 [M,K], qweight int32 [N,K/8], scales bf16 [N,K/128], y bf16 [M,N];
// ws f32 [S,M,N] with S = linear_w4_plan(M, N, K, splits), unused when
// S == 1.  Returns 0 once launched, non-zero (nothing launched) otherwise.
extern "C" int linear_w4_bf16(const void* x, const void* qweight,
                              const void* scales, float* ws, void* y,
                              long long M, int N, int K, int splits,
                              hipStream_t stream) {
  const int S = linear_w4_plan(M, N, K, splits);
  if (S < 1 || (S > 1 && ws == nullptr)) return 1;
  const int nch = K / W4_G;
  const int cps = (nch + S - 1) / S;
  const long long mtiles = (M + W4_BM - 1) / W4_BM;
  const long long blocks = mtiles * (N / 64) * S;
  if (blocks >= (1ll << 31)) return 1;
  hipLaunchKernelGGL(w4_gemm_kernel, dim3((unsigned)blocks), dim3(WAVE), 0,
                     stream, (const short*)x, (const int*)qweight,
                     (const unsigned short*)scales, (short*)y, ws, (int)M, N,
                     K, (int)mtiles, S, cps);
  if (S > 1) {
    const long long n4 = M * (N / 4);
    int grid = (int)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256);
    hipLaunchKernelGGL(w4_reduce_kernel, dim3(grid), dim3(256), 0, stream,
                       (const float*)ws, (short*)y, n4, S);
  }
  return 0;
}
