// FP8 W8A8 linear for decode- and serving-sized batches, gfx950:
//   y[m,n] = bf16(xscale[m] * wscale[n] * sum_k xq[m,k] * qweight[n,k])
// xq, qweight OCP e4m3 (torch.float8_e4m3fn), xscale, wscale fp32, y bf16.
//
// Format (ops.quantize_fp8 writes the weight side, fp8_quant_rows_kernel the
// activation side at run time, "W8A8 dynamic"):
//   qweight fp8 [N, K], row-major, plain bytes, no interleave;
//   wscale  f32 [N], one per output channel, w_hat[n,k] = wscale[n] * q[n,k];
//   xq      fp8 [M, K], xscale f32 [M], one per row (token).
//
// Row quantization, pinned so that a reference matches it bit for bit:
//   amax  = max |x[m,:]|                       (exact: a max of bf16 values)
//   scale = amax / 448 in fp32, 1 when amax == 0
//   q     = rne_e4m3(float(x) / scale)         (a correctly rounded fp32
//           division, then v_cvt_pk_fp8_f32, round to nearest even)
// The file is built without fast-math flags, so `/` is the correctly rounded
// division.  The quotient is clamped to +-448 before the convert; for finite
// rows that changes no result (|x| / scale <= 448 * (1 + 2^-22), which
// rounds to 448 anyway), it only keeps the convert away from its
// out-of-range encoding.
//
// MFMA: the K=64 form ships, v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3
// selected for both operands (cbsz = blgp = 0) and unit block scales (E8M0
// 127 in every scale byte).  A lane's operand is 32 bytes, so a 128-k chunk
// is two MFMAs per 32x32 fragment instead of the eight that
// v_mfma_f32_32x32x16_fp8_fp8 needs, at twice the K=16 form's rate per
// issued instruction; scripts/probe_mfma_fp8.cpp checks both forms on the
// device, the K=16 form was the fallback and is not built.
//
// Data path: a weight byte goes from HBM to the matrix unit with no VALU
// instruction.  A block is ONE wave owning MT 32-row M-tiles by 64 columns
// (two 32x32 C fragments per M-tile; layout: c_row() in attention_mfma32.h).
// A chunk is 128 k.  The k order inside a chunk is the kernel's own: lane
// half hi5 owns bytes hi5*64 .. hi5*64+63 of its row's chunk, the first
// MFMA takes the lower 32 of them and the second the upper 32, for A and B
// alike.  The only operand-layout fact this needs is that A and B map
// (lane half, register, byte) to the same k, which the probe confirms; a dot
// product does not care which k that is.  So a lane reads its share as four
// plain 16 B loads per row per chunk, and the loaded registers are the MFMA
// operands.  Loads of chunk i+1 are issued before the MFMAs of chunk i (two
// register sets in turn, w4_gemm_kernel's pipeline).
//
// MT: with MT = 2 a wave holds two M-tiles (64 rows, 64 accumulators)
// against one set of B fragments, so a weight tile is fetched once per 64
// rows instead of once per 32.  It ships: the launcher takes MT = 2 for
// M > 32 and MT = 1 up to 32 rows.  Measured on the four Llama-3-8B
// projections (profiles/linear_fp8.txt, "one vs two M-tiles"): at M = 128
// and 256 MT = 2 is 13 to 20 % faster on all four (gate_up M = 256: 153
// against 181 us); at M = 64 it wins on gate_up and down (50 / 56, 29 / 33
// us), is level on qkv (19.1 / 19.2) and loses on o_proj (16.5 / 15.3).  A
// row's sums are the same MFMAs in the same order under both.
//
// Scales touch fp32 values only: the accumulator is the exact-operand fp32
// sum, and (acc * xscale[m]) * wscale[n], in that order, is rounded to bf16
// once — in the GEMM epilogue for S = 1, in fp8_reduce_kernel for S > 1.
//
// Split-K: as linear_w4.hip.  K's chunks are cut into S contiguous slices,
// slice z's wave writes raw fp32 partials to ws[z][M][N] and
// fp8_reduce_kernel sums z ascending.  S is a function of (N, K) only
// (linear_fp8_plan), there are no float atomics and a row's sums never see
// another row: the result of a row is bitwise reproducible and independent
// of M, of MT and of the tile it falls into.  Nothing here allocates or
// synchronises, so a call captures into a graph.
#include "attention_mfma32.h"  // f32x16, c_row

#define FP8_CH 128  // k per chunk
#define FP8_BM 32   // rows per M-tile
// waves per row of M-tiles the split rule aims for: linear_w4's target,
// re-swept (profiles/linear_fp8.txt, "fp8 gemm splits sweep").  512 gives
// S = 6, 8, 2, 8 on the four Llama-3-8B projections, each the fastest
// candidate of its sweep or within 6 % of it at M = 1 and M = 32; 1024 and
// 256 each lose more than that somewhere (o_proj M = 32: 16.3 us at 1024
// waves against 13.4; down M = 1: 30.3 us at 256 against 22.9).
#define FP8_TARGET_WAVES 512
#define FP8_QT 256  // threads of a quantize block
#define FP8_QV 8    // 16 B vectors of x a quantize thread keeps in registers
#define FP8_UNIT_SCALE 0x7F7F7F7F  // E8M0 127 = 2^0 in every byte

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef unsigned char fp8_t;

// ------------------------------------------------------- row quantization

// max of the eight |bf16| of a vector, as the bf16's own bits (the order of
// non-negative bf16 values is the order of their bit patterns)
DEV_INLINE unsigned fp8_absmax8(bf16x8 v, unsigned m) {
  union {
    bf16x8 v;
    unsigned d[4];
  } u;
  u.v = v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned d = u.d[i] & 0x7FFF7FFFu;
    m = max(m, max(d >> 16, d & 0xFFFFu));
  }
  return m;
}

// eight bf16 -> eight e4m3 of x / scale, one 8 B store
DEV_INLINE void fp8_quant8(bf16x8 v, float scale, fp8_t* dst) {
  float q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    q[i] = __builtin_amdgcn_fmed3f(bf2f(v[i]) / scale, -448.f, 448.f);
  i32x2 o = {0, 0};
  o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], o[0], false);
  o[0] = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], o[0], true);
  o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], o[1], false);
  o[1] = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], o[1], true);
  *(i32x2*)dst = o;
}

// One workgroup per row.  REG: the row fits FP8_QT * FP8_QV vectors (K <=
// 16384) and stays in registers between the max and the quantization, so x
// is read once; otherwise the second pass reads it again.
template <bool REG>
DEV_INLINE void fp8_quant_row(const short* __restrict__ X,
                              fp8_t* __restrict__ XQ, float* __restrict__ XS,
                              int K, size_t row) {
  __shared__ unsigned red[FP8_QT / WAVE];
  const int tid = threadIdx.x, nv = K / 8;
  const bf16x8* xr = (const bf16x8*)(X + row * K);
  fp8_t* qr = XQ + row * K;

  bf16x8 v[FP8_QV];
  unsigned mx = 0;
  if (REG) {
#pragma unroll
    for (int i = 0; i < FP8_QV; ++i) {
      const int j = i * FP8_QT + tid;
      v[i] = j < nv ? xr[j] : bf16x8_zero();
      mx = fp8_absmax8(v[i], mx);
    }
  } else {
    for (int j = tid; j < nv; j += FP8_QT) mx = fp8_absmax8(xr[j], mx);
  }
#pragma unroll
  for (int s = 1; s < WAVE; s <<= 1)
    mx = max(mx, (unsigned)__shfl_xor((int)mx, s, WAVE));
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = mx;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < FP8_QT / WAVE; ++w) mx = max(mx, red[w]);

  const float amax = bf2f((short)mx);
  const float scale = amax == 0.f ? 1.f : amax / 448.f;
  if (tid == 0) XS[row] = scale;
  if (REG) {
#pragma unroll
    for (int i = 0; i < FP8_QV; ++i) {
      const int j = i * FP8_QT + tid;
      if (j < nv) fp8_quant8(v[i], scale, qr + (size_t)j * 8);
    }
  } else {
    for (int j = tid; j < nv; j += FP8_QT)
      fp8_quant8(xr[j], scale, qr + (size_t)j * 8);
  }
}

template <bool REG>
__global__ __launch_bounds__(FP8_QT) void fp8_quant_rows_kernel(
    const short* __restrict__ X, fp8_t* __restrict__ XQ,
    float* __restrict__ XS, int K) {
  fp8_quant_row<REG>(X, XQ, XS, K, blockIdx.x);
}

// The same rows, with the row count on the device: the grid covers the most
// rows there can be and a block past *ntiles * tile_rows exits (the whole
// block: the test is uniform, so the barrier inside is safe).  For the MoE
// lane's h, whose tile count only the align kernel knows (moe_mxfp4.hip).
template <bool REG>
__global__ __launch_bounds__(FP8_QT) void fp8_quant_rows_tiles_kernel(
    const short* __restrict__ X, fp8_t* __restrict__ XQ,
    float* __restrict__ XS, int K, const int* __restrict__ ntiles,
    int tile_rows) {
  if (blockIdx.x >= (unsigned)(*ntiles * tile_rows)) return;
  fp8_quant_row<REG>(X, XQ, XS, K, blockIdx.x);
}

// ------------------------------------------------------------------- GEMM

// one chunk's operands of a lane: 64 B of each of its MT x rows and of its
// two weight rows, as loaded
template <int MT>
struct Fp8Frags {
  i32x4 a[MT][4];
  i32x4 b[2][4];
};

// pa[t] / pb[f]: this lane's row of M-tile t / N-fragment f, + hi5*64
template <int MT>
DEV_INLINE void fp8_load(Fp8Frags<MT>& f, const fp8_t* const* pa,
                         const fp8_t* const* pb, int ch) {
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const i32x4* w = (const i32x4*)(pb[n] + (size_t)ch * FP8_CH);
#pragma unroll
    for (int q = 0; q < 4; ++q) f.b[n][q] = w[q];
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const i32x4* a = (const i32x4*)(pa[t] + (size_t)ch * FP8_CH);
#pragma unroll
    for (int q = 0; q < 4; ++q) f.a[t][q] = a[q];
  }
}

DEV_INLINE i32x8 fp8_operand(i32x4 lo, i32x4 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// one chunk: two K=64 MFMAs per fragment, the lower 32 B of every lane's
// share first
template <int MT>
DEV_INLINE void fp8_mma(const Fp8Frags<MT>& f, f32x16 (&acc)[MT][2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const i32x8 b = fp8_operand(f.b[n][2 * h], f.b[n][2 * h + 1]);
#pragma unroll
      for (int t = 0; t < MT; ++t)
        acc[t][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
            fp8_operand(f.a[t][2 * h], f.a[t][2 * h + 1]), b, acc[t][n],
            0 /* A: e4m3 */, 0 /* B: e4m3 */, 0, FP8_UNIT_SCALE, 0,
            FP8_UNIT_SCALE);
    }
  }
}

// grid = mtiles * (N/64) * S, M-tile fastest so the waves that share a
// weight tile run together; an M-tile here is MT * 32 rows.  cps = chunks
// per slice.  S == 1: Y bf16 [M,N], scaled; S > 1: WS f32 [S,M,N], raw sums.
template <int MT>
__global__ __launch_bounds__(WAVE) void fp8_gemm_kernel(
    const fp8_t* __restrict__ XQ, const float* __restrict__ XS,
    const fp8_t* __restrict__ QW, const float* __restrict__ WSC,
    short* __restrict__ Y, float* __restrict__ WS, int M, int N, int K,
    int mtiles, int S, int cps) {
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int ntiles = N / 64;
  const int mtile = blockIdx.x % mtiles;
  const int rest = blockIdx.x / mtiles;
  const int nb = rest % ntiles, z = rest / ntiles;
  const int nch = K / FP8_CH;
  const int ch0 = z * cps;
  const int ch1 = ch0 + cps < nch ? ch0 + cps : nch;
  const int m0 = mtile * (MT * FP8_BM);
  const int n0 = nb * 64;

  // a row past M reads row 0: its sums land in C rows that are never stored
  const fp8_t* pa[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int row = m0 + t * FP8_BM + l31;
    pa[t] = XQ + (size_t)(row < M ? row : 0) * K + hi5 * 64;
  }
  const fp8_t* const pb[2] = {QW + (size_t)(n0 + l31) * K + hi5 * 64,
                              QW + (size_t)(n0 + 32 + l31) * K + hi5 * 64};

  f32x16 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][0][r] = acc[t][1][r] = 0.f;

  // all chunks [ch0, ch1) ascending through two register sets in turn
  Fp8Frags<MT> f0, f1;
  fp8_load<MT>(f0, pa, pb, ch0);
  int c = ch0;
  for (; c + 2 < ch1; c += 2) {
    fp8_load<MT>(f1, pa, pb, c + 1);
    fp8_mma<MT>(f0, acc);
    fp8_load<MT>(f0, pa, pb, c + 2);
    fp8_mma<MT>(f1, acc);
  }
  if (c + 1 < ch1) {
    fp8_load<MT>(f1, pa, pb, c + 1);
    fp8_mma<MT>(f0, acc);
    fp8_mma<MT>(f1, acc);
  } else {
    fp8_mma<MT>(f0, acc);
  }

  // C fragment: register r of this lane is row c_row(r, hi5), column l31
  if (S == 1) {
    const float w0 = WSC[n0 + l31], w1 = WSC[n0 + 32 + l31];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + t * FP8_BM + c_row(r, hi5);
        if (m < M) {
          const float xs = XS[m];
          short* yrow = Y + (size_t)m * N + n0 + l31;
          yrow[0] = f2bf((acc[t][0][r] * xs) * w0);
          yrow[32] = f2bf((acc[t][1][r] * xs) * w1);
        }
      }
    }
  } else {
    float* ws = WS + (size_t)z * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + t * FP8_BM + c_row(r, hi5);
        if (m < M) {
          float* wrow = ws + (size_t)m * N + n0 + l31;
          wrow[0] = acc[t][0][r];
          wrow[32] = acc[t][1][r];
        }
      }
    }
  }
}

// y[m,n] = bf16(((ws[0] + ws[1] + ... + ws[S-1]) * xscale[m]) * wscale[n]),
// slices in ascending order; n4 = M * N/4 groups of four columns
__global__ __launch_bounds__(256) void fp8_reduce_kernel(
    const float* __restrict__ WS, const float* __restrict__ XS,
    const float* __restrict__ WSC, short* __restrict__ Y, long long n4,
    int N4, int S) {
  long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += stride) {
    f32x4 acc = *(const f32x4*)&WS[i * 4];
    for (int z = 1; z < S; ++z) {
      f32x4 p = *(const f32x4*)&WS[((long long)z * n4 + i) * 4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += p[q];
    }
    const float xs = XS[i / N4];
    const f32x4 w = *(const f32x4*)&WSC[(i % N4) * 4];
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = f2bf((acc[q] * xs) * w[q]);
    *(bf16x4*)&Y[i * 4] = o;
  }
}

// ---------------------------------------------------------------- launchers

static bool fp8_shape_ok(long long M, int N, int K) {
  return M >= 1 && M < (1ll << 31) && N >= 64 && N % 64 == 0 &&
         K >= FP8_CH && K % FP8_CH == 0;
}

// The number of K slices of a call, 0 for a shape the kernel does not
// support.  splits <= 0 asks for the rule: the smallest S that gives one
// row of M-tiles FP8_TARGET_WAVES waves, at most one slice per chunk — a
// function of (N, K) only, so a row's result does not depend on M.
// splits > 0 (tests and the benchmark sweep) is taken as given.  Either way
// S is normalised so that no slice is empty.
extern "C" int linear_fp8_plan(long long M, int N, int K, int splits) {
  if (!fp8_shape_ok(M, N, K)) return 0;
  const int nch = K / FP8_CH, ntiles = N / 64;
  int S = splits > 0 ? splits : (FP8_TARGET_WAVES + ntiles - 1) / ntiles;
  if (S > nch) {
    if (splits > 0) return 0;
    S = nch;
  }
  const int cps = (nch + S - 1) / S;
  return (nch + cps - 1) / cps;
}

// x bf16 [M,K] -> xq fp8 [M,K], xscale f32 [M].  Returns 0 once launched,
// non-zero (nothing launched) for an unsupported shape.
extern "C" int fp8_quant_rows_bf16(const void* x, void* xq, float* xscale,
                                   long long M, int K, hipStream_t stream) {
  if (M < 1 || M >= (1ll << 31) || K < FP8_CH || K % FP8_CH != 0) return 1;
  if (K / 8 <= FP8_QT * FP8_QV)
    hipLaunchKernelGGL(fp8_quant_rows_kernel<true>, dim3((unsigned)M),
                       dim3(FP8_QT), 0, stream, (const short*)x, (fp8_t*)xq,
                       xscale, K);
  else
    hipLaunchKernelGGL(fp8_quant_rows_kernel<false>, dim3((unsigned)M),
                       dim3(FP8_QT), 0, stream, (const short*)x, (fp8_t*)xq,
                       xscale, K);
  return 0;
}

// fp8_quant_rows_bf16 over the first *ntiles * tile_rows rows of x, a count
// read on the device; max_rows bounds it and sizes the grid.
extern "C" int fp8_quant_rows_tiles_bf16(const void* x, void* xq,
                                         float* xscale, long long max_rows,
                                         int K, const int* ntiles,
                                         int tile_rows, hipStream_t stream) {
  if (max_rows < 1 || max_rows >= (1ll << 31) || K < FP8_CH ||
      K % FP8_CH != 0 || tile_rows < 1)
    return 1;
  if (K / 8 <= FP8_QT * FP8_QV)
    hipLaunchKernelGGL(fp8_quant_rows_tiles_kernel<true>,
                       dim3((unsigned)max_rows), dim3(FP8_QT), 0, stream,
                       (const short*)x, (fp8_t*)xq, xscale, K, ntiles,
                       tile_rows);
  else
    hipLaunchKernelGGL(fp8_quant_rows_tiles_kernel<false>,
                       dim3((unsigned)max_rows), dim3(FP8_QT), 0, stream,
                       (const short*)x, (fp8_t*)xq, xscale, K, ntiles,
                       tile_rows);
  return 0;
}

template <int MT>
static int fp8_gemm_launch(const fp8_t* xq, const float* xscale,
                           const fp8_t* qweight, const float* wscale,
                           float* ws, short* y, long long M, int N, int K,
                           int S, hipStream_t stream) {
  const int nch = K / FP8_CH;
  const int cps = (nch + S - 1) / S;
  const long long mtiles = (M + MT * FP8_BM - 1) / (MT * FP8_BM);
  const long long blocks = mtiles * (N / 64) * S;
  if (blocks >= (1ll << 31)) return 1;
  hipLaunchKernelGGL(fp8_gemm_kernel<MT>, dim3((unsigned)blocks), dim3(WAVE),
                     0, stream, xq, xscale, qweight, wscale, y, ws, (int)M, N,
                     K, (int)mtiles, S, cps);
  return 0;
}

// xq fp8 [M,K], xscale f32 [M], qweight fp8 [N,K], wscale f32 [N], y bf16
// [M,N]; ws f32 [S,M,N] with S = linear_fp8_plan(M, N, K, splits), unused
// when S == 1.  mt = 0 takes the M-tile rule (two M-tiles per wave above 32
// rows); 1 or 2 forces it (tests and the benchmark only).  Returns 0 once
// launched, non-zero (nothing launched) otherwise.
extern "C" int linear_fp8_bf16(const void* xq, const float* xscale,
                               const void* qweight, const float* wscale,
                               float* ws, void* y, long long M, int N, int K,
                               int splits, int mt, hipStream_t stream) {
  const int S = linear_fp8_plan(M, N, K, splits);
  if (S < 1 || (S > 1 && ws == nullptr) || mt < 0 || mt > 2) return 1;
  if (mt == 0) mt = M > FP8_BM ? 2 : 1;
  const int rc =
      mt == 2 ? fp8_gemm_launch<2>((const fp8_t*)xq, xscale,
                                   (const fp8_t*)qweight, wscale, ws,
                                   (short*)y, M, N, K, S, stream)
              : fp8_gemm_launch<1>((const fp8_t*)xq, xscale,
                                   (const fp8_t*)qweight, wscale, ws,
                                   (short*)y, M, N, K, S, stream);
  if (rc) return rc;
  if (S > 1) {
    const long long n4 = M * (N / 4);
    int grid = (int)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256);
    hipLaunchKernelGGL(fp8_reduce_kernel, dim3(grid), dim3(256), 0, stream,
                       (const float*)ws, xscale, wscale, (short*)y, n4, N / 4,
                       S);
  }
  return 0;
}
