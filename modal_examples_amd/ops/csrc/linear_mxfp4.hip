// MXFP4 weight linear (W4A8, OCP MX block scales) for decode- and
// serving-sized batches, gfx950:
//   y[m,n] = bf16(xscale[m] * sum_k xq[m,k] * w_hat[n,k])
//   w_hat[n,k] = e2m1(qweight[n,k]) * 2^(wscale[n, k/32] - 127)
// xq OCP e4m3 [M,K] with xscale fp32 [M] (fp8_quant_rows_kernel of
// linear_fp8.hip, unchanged), y bf16 [M,N].
//
// Format (ops.quantize_mxfp4 writes it; the OCP MX layout, which is also
// torch.float4_e2m1fn_x2's):
//   qweight u8 [N, K/2], row-major, element 2j in the low nibble of byte j;
//   wscale  u8 [N, K/32], E8M0, one byte per block of 32 consecutive k.
// Byte 255 (NaN) is never written by the quantizer and its result here is
// undefined.
//
// MFMA: v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = 0 (A: e4m3, 32 bytes a
// lane) and blgp = 4 (B: e2m1, 16 bytes a lane).  A B lane's share of one
// instruction is 32 consecutive k of one row — one MX block — and the
// instruction multiplies that share by 2^(byte - 127) of a scale byte the
// lane supplies.  So the weight goes from HBM to the matrix unit as loaded:
// no decode VALU and no scale multiply.  What this file relies on, each
// checked on the device by scripts/probe_mfma_mxfp4.cpp (named by its
// output line):
//   "pairing + decode"   of the instruction's 64 k, nibble i of B's 16
//                        bytes in lane half h (low nibble of byte i/2
//                        first) is k = 32h + i: the plain OCP layout is the
//                        B operand, nothing is repacked.  Byte j of A's 32
//                        bytes is k = 16h + j for j < 16 and 32 + 16h +
//                        (j - 16) above: an A lane holds two runs of 16 k,
//                        NOT the block its B partner holds;
//   "decode, code by .." the 16 codes are +-{0, .5, 1, 1.5, 2, 3, 4, 6};
//   "scale lane, op_sel" byte op_sel of lane l's scale register applies to
//                        that lane's 32 k of row l & 31 and nothing else;
//   "scale decode"       the byte means 2^(byte - 127), no clipping at
//                        +-30, with A's byte at 127 a unit scale;
//   "upper four B .."    registers 4..7 of the builtin's B operand are
//                        ignored for fp4 (they are left undefined here).
// The C layout is c_row() (attention_mfma32.h), as probe_mfma_fp8.cpp shows.
//
// Work split: linear_fp8.hip's skeleton.  A block is ONE wave owning MT
// 32-row M-tiles by 64 columns (two 32x32 C fragments per M-tile); K's
// chunks go through two register sets in turn, the loads of chunk i+1
// issued before the MFMAs of chunk i.
//
// Chunk depth: 128 k ships.  On the weight side lane half h owns k = 64h ..
// 64h+63 of its row's chunk: 32 contiguous weight bytes (two 16 B loads,
// one per MFMA) and TWO contiguous scale bytes, wscale[n][ch*4 + 2h +
// {0,1}], one aligned 16-bit load whose bytes op_sel 0 and 1 pick.  MFMA j
// (0, 1) of a chunk therefore multiplies MX blocks j (lane half 0) and 2 + j
// (lane half 1): its 64 k are chunk k 32j .. 32j+31 and 64+32j .. 64+32j+31,
// which a dot product does not mind.  By the A layout above, lane half h of
// an x row then needs chunk bytes 32j+16h .. +15 in registers 0..3 and
// 64+32j+16h .. +15 in registers 4..7: over both MFMAs the four 16 B loads
// at 16h + 32q, q = 0..3, with MFMA j taking loads j and 2 + j.  The two
// lane halves of a row read the chunk's 128 B line between them, and no
// byte is moved by a VALU instruction.  Registers of one set: MT*16 (x) + 2*8
// (weights) + 2 (scales) = 34 / 50 for MT = 1 / 2, so two sets and the
// 32 / 64 accumulators stay far inside the 256 registers of two waves per
// SIMD.  The 256-deep alternative (four 16 B weight loads, one dword of four
// scale bytes, op_sel 0..3) doubles the x side to MT*32 registers a set:
// with MT = 2 two sets alone are 2 * (64 + 16 + 2) = 164 beside 64
// accumulators and the addresses, which does not fit two waves per SIMD
// without spilling, and it needs a 128-k tail body because K is a multiple
// of 128 only.  It was decided against on that register budget and was not
// built, so no time is reported for it.
//
// The A side is 32 B per lane per MFMA against 16 B of B: x is now the
// larger operand per lane.  It comes from L2 (M * K bytes shared by every
// column tile) while the weights stream from HBM once per MT*32 rows.  MT
// was measured again for this ratio on the four Llama-3-8B projections
// (profiles/linear_mxfp4.txt, "one vs two M-tiles"): at M = 32 one M-tile
// wins on all four (gate_up 31.1 against 34.9 us); at M = 64 two win on qkv,
// gate_up and down (17.2 / 17.8, 42.4 / 48.9, 23.7 / 28.5 us) and are level
// on o_proj (14.9 / 14.7); at 128 and 256 two win on all four by 7 to 29 %.
// So the launcher takes MT = 2 for M > 32 — the fp8 kernel's rule, arrived
// at from this kernel's own numbers.  A row's sums are the same MFMAs in the
// same order under both.
//
// Scale: the accumulator is the exact-operand fp32 sum with the block
// scales applied by the matrix unit, and acc * xscale[m] is rounded to bf16
// once — in the GEMM epilogue for S = 1, in mxfp4_reduce_kernel for S > 1.
//
// Split-K: as linear_fp8.hip.  K's chunks are cut into S contiguous slices,
// slice z's wave writes raw fp32 partials to ws[z][M][N] and
// mxfp4_reduce_kernel sums z ascending.  S is a function of (N, K) only
// (linear_mxfp4_plan), there are no float atomics and a row's sums never
// see another row: the result of a row is bitwise reproducible and
// independent of M, of MT and of the tile it falls into.  Rows past M read
// row 0 and are never stored; K is a whole number of chunks, so there is no
// K tail to read past.  Nothing here allocates or synchronises, so a call
// captures into a graph.
#include "mxfp4_mma.h"  // MxFrags, mx_load, mx_mma, mx_chunks: the chunk recipe

// waves per row of M-tiles the split rule aims for, swept for this byte
// volume (profiles/linear_mxfp4.txt, "mxfp4 gemm splits sweep").  512 gives
// S = 6, 8, 2, 8 on the four Llama-3-8B projections: the fastest candidate
// at M = 1 and M = 32 on qkv, gate_up and down, and within 7 % of S = 4 on
// o_proj (10.0 / 9.8, 12.0 / 11.2 us).  256 loses 16 % on qkv and 18 % on
// down at M = 1 (12.5 / 10.8, 21.0 / 17.8 us); 1024 loses 7 to 27 %.
#define MX_TARGET_WAVES 512

// grid = mtiles * (N/64) * S, M-tile fastest so the waves that share a
// weight tile run together; an M-tile here is MT * 32 rows.  cps = chunks
// per slice.  S == 1: Y bf16 [M,N], scaled; S > 1: WS f32 [S,M,N], raw sums.
template <int MT>
__global__ __launch_bounds__(WAVE) void mxfp4_gemm_kernel(
    const mx_u8* __restrict__ XQ, const float* __restrict__ XS,
    const mx_u8* __restrict__ QW, const mx_u8* __restrict__ WSC,
    short* __restrict__ Y, float* __restrict__ WS, int M, int N, int K,
    int mtiles, int S, int cps) {
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int ntiles = N / 64;
  const int mtile = blockIdx.x % mtiles;
  const int rest = blockIdx.x / mtiles;
  const int nb = rest % ntiles, z = rest / ntiles;
  const int nch = K / MX_CH;
  const int ch0 = z * cps;
  const int ch1 = ch0 + cps < nch ? ch0 + cps : nch;
  const int m0 = mtile * (MT * MX_BM);
  const int n0 = nb * 64;

  // a row past M reads row 0: its sums land in C rows that are never stored
  const mx_u8* pa[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int row = m0 + t * MX_BM + l31;
    pa[t] = XQ + (size_t)(row < M ? row : 0) * K + hi5 * 16;
  }
  const size_t r0 = n0 + l31, r1 = n0 + 32 + l31;
  const mx_u8* const pb[2] = {QW + r0 * (K / 2) + hi5 * 32,
                              QW + r1 * (K / 2) + hi5 * 32};
  const mx_u8* const ps[2] = {WSC + r0 * (K / 32) + hi5 * 2,
                              WSC + r1 * (K / 32) + hi5 * 2};

  f32x16 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][0][r] = acc[t][1][r] = 0.f;

  // all chunks [ch0, ch1) ascending through two register sets in turn
  mx_chunks<MT>(acc, pa, pb, ps, ch0, ch1);

  // C fragment: register r of this lane is row c_row(r, hi5), column l31
  if (S == 1) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + t * MX_BM + c_row(r, hi5);
        if (m < M) {
          const float xs = XS[m];
          short* yrow = Y + (size_t)m * N + n0 + l31;
          yrow[0] = f2bf(acc[t][0][r] * xs);
          yrow[32] = f2bf(acc[t][1][r] * xs);
        }
      }
    }
  } else {
    float* ws = WS + (size_t)z * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + t * MX_BM + c_row(r, hi5);
        if (m < M) {
          float* wrow = ws + (size_t)m * N + n0 + l31;
          wrow[0] = acc[t][0][r];
          wrow[32] = acc[t][1][r];
        }
      }
    }
  }
}

// y[m,n] = bf16((ws[0] + ws[1] + ... + ws[S-1]) * xscale[m]), slices in
// ascending order; n4 = M * N/4 groups of four columns
__global__ __launch_bounds__(256) void mxfp4_reduce_kernel(
    const float* __restrict__ WS, const float* __restrict__ XS,
    short* __restrict__ Y, long long n4, int N4, int S) {
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
    bf16x4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = f2bf(acc[q] * xs);
    *(bf16x4*)&Y[i * 4] = o;
  }
}

// ---------------------------------------------------------------- launchers

static bool mx_shape_ok(long long M, int N, int K) {
  return M >= 1 && M < (1ll << 31) && N >= 64 && N % 64 == 0 &&
         K >= MX_CH && K % MX_CH == 0;
}

// The number of K slices of a call, 0 for a shape the kernel does not
// support.  splits <= 0 asks for the rule: the smallest S that gives one
// row of M-tiles MX_TARGET_WAVES waves, at most one slice per chunk — a
// function of (N, K) only, so a row's result does not depend on M.
// splits > 0 (tests and the benchmark sweep) is taken as given.  Either way
// S is normalised so that no slice is empty.
extern "C" int linear_mxfp4_plan(long long M, int N, int K, int splits) {
  if (!mx_shape_ok(M, N, K)) return 0;
  const int nch = K / MX_CH, ntiles = N / 64;
  int S = splits > 0 ? splits : (MX_TARGET_WAVES + ntiles - 1) / ntiles;
  if (S > nch) {
    if (splits > 0) return 0;
    S = nch;
  }
  const int cps = (nch + S - 1) / S;
  return (nch + cps - 1) / cps;
}

template <int MT>
static int mx_gemm_launch(const mx_u8* xq, const float* xscale,
                          const mx_u8* qweight, const mx_u8* wscale,
                          float* ws, short* y, long long M, int N, int K,
                          int S, hipStream_t stream) {
  const int nch = K / MX_CH;
  const int cps = (nch + S - 1) / S;
  const long long mtiles = (M + MT * MX_BM - 1) / (MT * MX_BM);
  const long long blocks = mtiles * (N / 64) * S;
  if (blocks >= (1ll << 31)) return 1;
  hipLaunchKernelGGL(mxfp4_gemm_kernel<MT>, dim3((unsigned)blocks),
                     dim3(WAVE), 0, stream, xq, xscale, qweight, wscale, y,
                     ws, (int)M, N, K, (int)mtiles, S, cps);
  return 0;
}

// xq fp8 [M,K], xscale f32 [M], qweight u8 [N,K/2], wscale u8 [N,K/32], y
// bf16 [M,N]; ws f32 [S,M,N] with S = linear_mxfp4_plan(M, N, K, splits),
// unused when S == 1.  mt = 0 takes the M-tile rule (two M-tiles per wave
// above 32 rows); 1 or 2 forces it (tests and the benchmark only).  Returns
// 0 once launched, non-zero (nothing launched) otherwise.
extern "C" int linear_mxfp4_bf16(const void* xq, const float* xscale,
                                 const void* qweight, const void* wscale,
                                 float* ws, void* y, long long M, int N,
                                 int K, int splits, int mt,
                                 hipStream_t stream) {
  const int S = linear_mxfp4_plan(M, N, K, splits);
  if (S < 1 || (S > 1 && ws == nullptr) || mt < 0 || mt > 2) return 1;
  if (mt == 0) mt = M > MX_BM ? 2 : 1;
  const int rc =
      mt == 2 ? mx_gemm_launch<2>((const mx_u8*)xq, xscale,
                                  (const mx_u8*)qweight, (const mx_u8*)wscale,
                                  ws, (short*)y, M, N, K, S, stream)
              : mx_gemm_launch<1>((const mx_u8*)xq, xscale,
                                  (const mx_u8*)qweight, (const mx_u8*)wscale,
                                  ws, (short*)y, M, N, K, S, stream);
  if (rc) return rc;
  if (S > 1) {
    const long long n4 = M * (N / 4);
    int grid = (int)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256);
    hipLaunchKernelGGL(mxfp4_reduce_kernel, dim3(grid), dim3(256), 0, stream,
                       (const float*)ws, xscale, (short*)y, n4, N / 4, S);
  }
  return 0;
}
