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
//
// Prefill: fp8_gemm_tiled_kernel<WM>, the workgroup-tiled form of the same
// product for hundreds to thousands of rows, where the rows kernel's
// one-wave tiles re-read both operands from global memory too often.
//   Work split.  256 threads = 4 waves own a BM x 128 output tile over all
// of K (no split-K), BM = WM * 64.  The waves form a 2 x 2 grid: wave w owns
// rows (w & 1) * WM * 32 .. and columns (w >> 1) * 64 .., WM x 2 C fragments.
// WM = 2 is the 128 x 128 tile (64 accumulators), WM = 4 the 256 x 128 tile
// (128 accumulators).  Per chunk a wave reads (WM + 2) * 4 KB from LDS for
// WM * 4 MFMAs: 16 KB for 8, 24 KB for 16.
//   Data movement.  Per 128-k chunk the workgroup stages BM rows of xq and
// 128 rows of qweight, 128 B each, global -> registers -> LDS (16 B per
// thread per load, eight threads per row, so a row's 128 B are one coalesced
// request); the weight rows go through fp8_stage_load_w alone.  Two LDS
// stages: chunk i + 1's global loads are issued before chunk i's MFMAs and
// written to the other stage after them, one barrier per chunk.  Two stages
// are 64 KB (WM = 2) or 96 KB (WM = 4), taken as dynamic LDS.
//   LDS image.  A tile is [rows][128 B], pitch 128 B with no padding; the
// 16 B unit u of row r sits at unit (u ^ r ^ (r >> 3)) & 7 (fp8_tile_off).
// A lane's MFMA operand is units hi5*4 + 2h, hi5*4 + 2h + 1 of its row (the
// rows kernel's in-chunk convention: half hi5 owns bytes hi5*64 .. +63, the
// lower 32 first), read as two 16 B reads.  Across 8 consecutive rows the
// XOR spreads one unit column over all eight 16 B slots of the 128 B pitch,
// and the r >> 3 term moves rows r and r + 8 (same 256 B phase) apart, so 16
// consecutive rows reading the same unit touch 16 distinct 16 B slots of
// the 64 banks.  The staging writes cover whole rows and are conflict-free
// under any permutation inside a row.
//   Edges.  A row past M reads row M - 1, a weight row past N row N - 1;
// neither is stored.  N % 128 == 64: the waves of the dead column half take
// part in staging and barriers and skip their MFMAs and stores.
//   Epilogue.  The product is computed transposed, weights as the MFMA's A
// and x as its B, so C register 4g + j of a lane is column
// 8g + 4*hi5 + j of row l31: four consecutive n, stored as one 8 B bf16x4
// ((acc * xscale[m]) * wscale[n], one rounding, as the rows kernel).  A row's
// sum is the same MFMAs over the same bytes in ascending chunk order
// whatever M, WM or the tile it falls into.
//   Block order: M-tile fastest, so the workgroups that share a weight tile
// are launched together and find it in L2.
#include "attention_mfma32.h"  // f32x16, c_row

#include <atomic>

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

// ------------------------------------------------- tiled GEMM (prefill)

#define FP8_TN 128        // columns of a workgroup tile
#define FP8_TTHREADS 256  // 4 waves, 2 x 2

// byte offset of 16 B unit `unit` of row `row` in a [rows][128 B] LDS tile
DEV_INLINE int fp8_tile_off(int row, int unit) {
  return row * FP8_CH + (((unit ^ row ^ (row >> 3)) & 7) << 4);
}

// one chunk of a workgroup's operands in flight: thread t holds unit t & 7
// of rows (t >> 3) + 32 * i
template <int WM>
struct Fp8Stage {
  i32x4 x[WM * 2];
  i32x4 w[FP8_TN / 32];
};

// the weight side of a stage, the one place that knows the weight format
DEV_INLINE void fp8_stage_load_w(i32x4 (&w)[FP8_TN / 32],
                                 const fp8_t* const* pw, int ch) {
#pragma unroll
  for (int i = 0; i < FP8_TN / 32; ++i)
    w[i] = *(const i32x4*)(pw[i] + (size_t)ch * FP8_CH);
}

template <int WM>
DEV_INLINE void fp8_stage_load(Fp8Stage<WM>& s, const fp8_t* const* px,
                               const fp8_t* const* pw, int ch) {
  fp8_stage_load_w(s.w, pw, ch);
#pragma unroll
  for (int i = 0; i < WM * 2; ++i)
    s.x[i] = *(const i32x4*)(px[i] + (size_t)ch * FP8_CH);
}

// stage image: x tile [WM*64][128 B], then the weight tile [128][128 B]
template <int WM>
DEV_INLINE void fp8_stage_write(const Fp8Stage<WM>& s, char* stage, int tid) {
  const int u = tid & 7, r0 = tid >> 3;
#pragma unroll
  for (int i = 0; i < WM * 2; ++i)
    *(i32x4*)(stage + fp8_tile_off(r0 + 32 * i, u)) = s.x[i];
  char* wt = stage + WM * 64 * FP8_CH;
#pragma unroll
  for (int i = 0; i < FP8_TN / 32; ++i)
    *(i32x4*)(wt + fp8_tile_off(r0 + 32 * i, u)) = s.w[i];
}

DEV_INLINE i32x8 fp8_lds_operand(const char* tile, int row, int unit) {
  return fp8_operand(*(const i32x4*)(tile + fp8_tile_off(row, unit)),
                     *(const i32x4*)(tile + fp8_tile_off(row, unit + 1)));
}

// one chunk of one wave from a stage: xrow / wrow are this lane's row of the
// wave's first x / weight fragment.  acc[t][f] is C^T: weights are A.
template <int WM>
DEV_INLINE void fp8_tile_mma(const char* stage, int xrow, int wrow, int hi5,
                             f32x16 (&acc)[WM][2]) {
  const char* wt = stage + WM * 64 * FP8_CH;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int unit = hi5 * 4 + h * 2;
    const i32x8 w0 = fp8_lds_operand(wt, wrow, unit);
    const i32x8 w1 = fp8_lds_operand(wt, wrow + 32, unit);
#pragma unroll
    for (int t = 0; t < WM; ++t) {
      const i32x8 x = fp8_lds_operand(stage, xrow + 32 * t, unit);
      acc[t][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          w0, x, acc[t][0], 0 /* A: e4m3 */, 0 /* B: e4m3 */, 0,
          FP8_UNIT_SCALE, 0, FP8_UNIT_SCALE);
      acc[t][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          w1, x, acc[t][1], 0, 0, 0, FP8_UNIT_SCALE, 0, FP8_UNIT_SCALE);
    }
  }
}

// grid = mtiles * ceil(N / 128), M-tile fastest; dynamic LDS = two stages of
// (WM * 64 + 128) * 128 B
template <int WM>
__global__ __launch_bounds__(FP8_TTHREADS) void fp8_gemm_tiled_kernel(
    const fp8_t* __restrict__ XQ, const float* __restrict__ XS,
    const fp8_t* __restrict__ QW, const float* __restrict__ WSC,
    short* __restrict__ Y, int M, int N, int K, int mtiles) {
  extern __shared__ __attribute__((aligned(16))) char fp8_lds[];
  constexpr int BM = WM * 64;
  constexpr int STAGE = (BM + FP8_TN) * FP8_CH;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int l31 = lane & 31, hi5 = lane >> 5;
  const int m0 = (blockIdx.x % mtiles) * BM;
  const int n0 = (blockIdx.x / mtiles) * FP8_TN;
  const int nch = K / FP8_CH;

  // staging sources: clamped rows are read and never stored
  const int u = tid & 7, r0 = tid >> 3;
  const fp8_t* px[WM * 2];
  const fp8_t* pw[FP8_TN / 32];
#pragma unroll
  for (int i = 0; i < WM * 2; ++i) {
    const int row = m0 + r0 + 32 * i;
    px[i] = XQ + (size_t)(row < M ? row : M - 1) * K + u * 16;
  }
#pragma unroll
  for (int i = 0; i < FP8_TN / 32; ++i) {
    const int row = n0 + r0 + 32 * i;
    pw[i] = QW + (size_t)(row < N ? row : N - 1) * K + u * 16;
  }

  const int xrow = (wave & 1) * (WM * 32) + l31;  // in the x tile
  const int wrow = (wave >> 1) * 64 + l31;        // in the weight tile
  const int nw = n0 + (wave >> 1) * 64;           // the wave's first column
  const bool live = nw < N;                       // wave-uniform

  f32x16 acc[WM][2];
#pragma unroll
  for (int t = 0; t < WM; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][0][r] = acc[t][1][r] = 0.f;

  // prologue: chunk 0 into stage 0.  Body, nch - 1 trips: chunk c + 1's
  // loads fly over chunk c's MFMAs and land in the stage chunk c - 1 used,
  // which every wave left before the previous barrier.  Tail: the last
  // chunk's MFMAs.
  Fp8Stage<WM> s;
  fp8_stage_load<WM>(s, px, pw, 0);
  fp8_stage_write<WM>(s, fp8_lds, tid);
  __syncthreads();
  int c = 0;
  for (; c + 1 < nch; ++c) {
    fp8_stage_load<WM>(s, px, pw, c + 1);
    if (live) fp8_tile_mma<WM>(fp8_lds + (c & 1) * STAGE, xrow, wrow, hi5, acc);
    fp8_stage_write<WM>(s, fp8_lds + ((c + 1) & 1) * STAGE, tid);
    __syncthreads();
  }
  if (!live) return;
  fp8_tile_mma<WM>(fp8_lds + (c & 1) * STAGE, xrow, wrow, hi5, acc);

  // C^T fragment f of M-fragment t: registers 4g .. 4g+3 of this lane are
  // columns nw + 32f + 8g + 4*hi5 .. +3 of row m
  f32x4 wsc[2][4];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      wsc[f][g] = *(const f32x4*)&WSC[nw + 32 * f + 8 * g + 4 * hi5];
#pragma unroll
  for (int t = 0; t < WM; ++t) {
    const int m = m0 + (wave & 1) * (WM * 32) + 32 * t + l31;
    if (m < M) {
      const float xs = XS[m];
      short* yrow = Y + (size_t)m * N + nw + 4 * hi5;
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          bf16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            o[j] = f2bf((acc[t][f][4 * g + j] * xs) * wsc[f][g][j]);
          *(bf16x4*)(yrow + 32 * f + 8 * g) = o;
        }
    }
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

// ------------------------------------------------------ tiled GEMM launcher

// The tile of a call: 1 = 128 x 128, 2 = 256 x 128; either gives a row the
// same bits.  The rule has no threshold: 128 x 128 for every shape.  Measured
// on the four Llama-3-8B projections at M = 256 .. 8192
// (profiles/linear_fp8_tiled.txt, "fp8tile1" against "fp8tile2"), the
// 128 x 128 tile is the faster on all 24 rows, by 19 to 43 % from 2048 rows
// up (gate_up M = 8192: 1322 against 1698 us; o_proj M = 2048: 57 against
// 71 us).  The 256 x 128 tile's 128 accumulators and 96 KB of LDS leave one
// wave per SIMD, so nothing covers a wave's LDS reads and barrier waits; it
// stays built for the benchmark and the tests.
static int fp8_tile_rule(long long M, int N, int K) {
  (void)M;
  (void)N;
  (void)K;
  return 1;
}

template <int WM>
static int fp8_tiled_launch(const fp8_t* xq, const float* xscale,
                            const fp8_t* qweight, const float* wscale,
                            short* y, long long M, int N, int K,
                            hipStream_t stream) {
  constexpr int BM = WM * 64;
  constexpr int LDS = 2 * (BM + FP8_TN) * FP8_CH;
  const long long mtiles = (M + BM - 1) / BM;
  const long long blocks = mtiles * ((N + FP8_TN - 1) / FP8_TN);
  if (blocks >= (1ll << 31)) return 1;
  // the LDS ceiling of this instantiation, raised once per device
  static std::atomic<unsigned long long> raised{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
  if (!(raised.load(std::memory_order_relaxed) >> dev & 1)) {
    if (hipFuncSetAttribute((const void*)fp8_gemm_tiled_kernel<WM>,
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            LDS) != hipSuccess)
      return 1;
    raised.fetch_or(1ull << dev, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(fp8_gemm_tiled_kernel<WM>, dim3((unsigned)blocks),
                     dim3(FP8_TTHREADS), LDS, stream, xq, xscale, qweight,
                     wscale, y, (int)M, N, K, (int)mtiles);
  return 0;
}

// The operands of linear_fp8_bf16, no workspace.  tile = 0 takes
// fp8_tile_rule; 1 / 2 force the 128 x 128 / 256 x 128 tile (tests and the
// benchmark only).  Returns 0 once launched, non-zero (nothing launched)
// for an unsupported shape or a grid out of range.
extern "C" int linear_fp8_tiled_bf16(const void* xq, const float* xscale,
                                     const void* qweight, const float* wscale,
                                     void* y, long long M, int N, int K,
                                     int tile, hipStream_t stream) {
  if (!fp8_shape_ok(M, N, K) || tile < 0 || tile > 2) return 1;
  if (tile == 0) tile = fp8_tile_rule(M, N, K);
  return tile == 2
             ? fp8_tiled_launch<4>((const fp8_t*)xq, xscale,
                                   (const fp8_t*)qweight, wscale, (short*)y,
                                   M, N, K, stream)
             : fp8_tiled_launch<2>((const fp8_t*)xq, xscale,
                                   (const fp8_t*)qweight, wscale, (short*)y,
                                   M, N, K, stream);
}
