// Fused MoE FFN over MXFP4 experts (W4A8, OCP MX block scales), gfx950:
// moe.hip's schedule, slot map, epilogues and plane combine around grouped
// GEMMs that feed the experts' fp4 bytes and E8M0 scale bytes to
// v_mfma_scale_f32_32x32x64_f8f6f4 exactly as loaded (mxfp4_mma.h, the chunk
// recipe of linear_mxfp4.hip).
//
// Format (ops.quantize_mxfp4_experts; linear_mxfp4.hip's with a leading
// expert dimension): gate_up_q u8 [E,2F,d/2] + gate_up_s u8 [E,2F,d/32],
// down_q u8 [E,d,F/2] + down_s u8 [E,d,F/32]; element 2j of a row in the low
// nibble of byte j, one scale byte per 32 consecutive k.  Scale byte 255 is
// undefined, as in the dense lane.
//
// Semantics (ops.reference.moe_ffn_mxfp4_ref states them):
//   xq, xs = quantize_rows_fp8(x)                 once per token
//   g, u   = xs[t] * (xq[t] . w_hat_gate_up[e]^T) fp32
//   h      = bf16(silu(g) * u)
//   hq, hs = quantize_rows_fp8(h)                 per (token, expert) row
//   y      = hs * (hq . w_hat_down[e]^T)          fp32
//   out[t] = bf16(sum_j weights[t,j] * y[t,j])    in j order
// which is what a dense Mxfp4Linear SwiGLU FFN computes per expert.
//
// Launches, in order:
//   1 fp8_quant_rows_kernel over x [N,d] (linear_fp8.hip, unchanged)
//   2 moe_align_kernel (moe.hip, unchanged)
//   3 moe_gemm_mxfp4_kernel<true>: one wave per block owns one 32-slot M-tile
//     and two 32-column N-tiles, gate columns n0.. and up columns F+n0.. of
//     expert tile_expert[mtile].  A rows are xq rows gathered through the
//     slot map (a pad slot reads row 0 and its h is written as zero), one
//     byte per element, at the A operand's two runs of 16 k.  B is the
//     expert's fp4 rows and two scale bytes per lane half per chunk.  Epilogue:
//     acc * xs[token] on both fragments, SwiGLU in fp32, h bf16 [slots,F].
//   4 fp8_quant_rows_tiles_kernel over h: hq e4m3 [slots,F], hs f32 [slots]
//   5 moe_gemm_mxfp4_kernel<false>: 64 adjacent columns, A rows hq in slot
//     order, K cut into S contiguous slices of one wave each (S = 1 by the
//     rule, moe_ffn_mxfp4_plan); epilogue acc * hs[slot] into plane z of y
//     f32 [S][N*k][d]
//   6 moe_combine_kernel / moe_combine_planes_kernel (moe.hip, unchanged)
//
// Against the dense kernel the grouped one differs in three things: the
// gather and the per-tile expert base on the A / B addresses, MT fixed at 1
// (a tile belongs to one expert, so a second M-tile would need a second set
// of B fragments), and its two epilogues.  The inner loop is mx_chunks<1>,
// the same code: chunks of 128 k through two register sets, the loads of
// chunk i+1 issued before the MFMAs of chunk i, no LDS, and no VALU
// instruction on a weight or activation byte.
//
// Why h gets a pass of its own.  The down GEMM's A operand is e4m3 with one
// scale per row, and a row's absmax spans the F/32 waves of the up GEMM that
// produce it, so no up-GEMM wave can quantize what it holds.  The pass reads
// 2 B and writes 1 B per h element: slots*F*3 bytes against the E*3*F*d*0.53
// bytes of weights that a decode-sized call streams — at d = F = 4096, E = 8,
// N = 64 that is 4.7 MB (at most 384 slots) against 213 MB, 2 %.  The
// alternative, converting bf16 h to e4m3 inside the down GEMM, still needs
// the row maximum from somewhere, repeats the conversion in each of the d/64
// column blocks that read the row, and puts a divide and a convert per
// element back on an operand path whose point is that bytes go from memory
// to the matrix unit untouched.  The pass reuses the row quantizer's
// arithmetic (fp8_quant_row, linear_fp8.hip) under a grid sized from
// max_tiles whose blocks past the device-side tile count exit.
//
// Registers of one set: 16 (x: four 16 B loads) + 16 (weights: two rows of
// two 16 B loads) + 2 (scales) = 34; two sets and the 32 accumulators are
// 100, and with the addresses both kernels build to 111, under the 128
// registers of four waves per SIMD, which is what amdgpu_waves_per_eu asks
// for (no spills and no scratch: scripts/check_kernel_resources.py).
//
// Contract, as the bf16 and int4 lanes: every grid and workspace size is a
// function of (N, top_k, E, dim, ffn_dim) only; nothing allocates or
// synchronises; no float atomics; each GEMM sums K in one fixed order, so a
// token's row is bitwise reproducible and independent of the rest of the
// batch and of the tile it lands in; the call captures into a hipGraph.
#include "mxfp4_mma.h"
#include "moe_sched.h"

// linear_fp8.hip
extern "C" int fp8_quant_rows_bf16(const void*, void*, float*, long long, int,
                                   hipStream_t);
extern "C" int fp8_quant_rows_tiles_bf16(const void*, void*, float*,
                                         long long, int, const int*, int,
                                         hipStream_t);

// One wave per block: M-tile mtile (32 slots of one expert) x two 32-column
// N-tiles over the chunks of K slice z.  UP (one slice): A = xq [N,K] rows
// gathered through the slot map, AS = xs [N]; the N-tiles are gate columns
// n0.. and up columns Nout+n0..; silu(gate)*up to H.  !UP: A = hq [slots,K]
// in slot order, AS = hs [slots]; 64 adjacent columns; the slice's scaled
// fp32 partial of each row to its pair's row of plane z of Y [S][P][Nout].
// cps = chunks per slice.
template <bool UP>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
void moe_gemm_mxfp4_kernel(
    const mx_u8* __restrict__ A, const float* __restrict__ AS,
    const mx_u8* __restrict__ QW, const mx_u8* __restrict__ SC,
    const int* __restrict__ slot_map, const int* __restrict__ tile_expert,
    const int* __restrict__ num_tiles, short* __restrict__ H,
    float* __restrict__ Y, int K, int Nout, int top_k, int max_tiles, int cps,
    long long plane) {
  const int mtile = blockIdx.x % max_tiles;
  if (mtile >= *num_tiles) return;  // tiles past the device-side count
  const int rest = blockIdx.x / max_tiles;
  const int nblocks = Nout / (UP ? 32 : 64);
  const int nb = rest % nblocks, z = rest / nblocks;
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int e = tile_expert[mtile];
  const int slot = mtile * MOE_BM + l31;
  const int nch = K / MX_CH;
  const int ch0 = z * cps;
  const int ch1 = ch0 + cps < nch ? ch0 + cps : nch;

  int n[2];  // first column of each N-tile, as rows of the expert's matrix
#pragma unroll
  for (int t = 0; t < 2; ++t)
    n[t] = UP ? t * Nout + nb * 32 : (nb * 2 + t) * 32;
  size_t a_row = (size_t)slot;
  if (UP) {
    // a pad slot reads token 0: its sums land in C rows stored as zero
    const int pair = slot_map[slot];
    a_row = pair < 0 ? 0 : (size_t)(pair / top_k);
  }
  const size_t w_row0 = (size_t)e * (UP ? 2 * (size_t)Nout : (size_t)Nout);
  const mx_u8* const pa[1] = {A + a_row * K + hi5 * 16};
  const size_t r0 = w_row0 + n[0] + l31, r1 = w_row0 + n[1] + l31;
  const mx_u8* const pb[2] = {QW + r0 * (K / 2) + hi5 * 32,
                              QW + r1 * (K / 2) + hi5 * 32};
  const mx_u8* const ps[2] = {SC + r0 * (K / 32) + hi5 * 2,
                              SC + r1 * (K / 32) + hi5 * 2};

  f32x16 acc[1][2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][0][r] = acc[0][1][r] = 0.f;
  mx_chunks<1>(acc, pa, pb, ps, ch0, ch1);

  // C fragment: register r of this lane is row c_row(r, hi5), column l31
  if constexpr (UP) {
    short* hrow = H + (size_t)mtile * MOE_BM * Nout + n[0] + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = c_row(r, hi5);
      const int pr = slot_map[mtile * MOE_BM + row];
      float h = 0.f;
      if (pr >= 0) {
        const float xs = AS[pr / top_k];
        const float g = acc[0][0][r] * xs, u = acc[0][1][r] * xs;
        h = g / (1.f + __expf(-g)) * u;
      }
      hrow[(size_t)row * Nout] = f2bf(h);
    }
  } else {
    float* yz = Y + (size_t)z * plane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = mtile * MOE_BM + c_row(r, hi5);
      const int pr = slot_map[s];
      if (pr >= 0) {
        const float hs = AS[s];
        float* yrow = yz + (size_t)pr * Nout + l31;
        yrow[n[0]] = acc[0][0][r] * hs;
        yrow[n[1]] = acc[0][1][r] * hs;
      }
    }
  }
}

// ---------------------------------------------------------------- launchers

// The K slices of the down GEMM for ffn_dim F (= planes of y), 0 for an
// unsupported F.  splits <= 0 asks for the rule, MOE_MX_DOWN_SLICES capped at
// one slice per chunk: a function of F only.  splits > 0 (tests and the
// benchmark's sweep) is taken as given.  Either way the count is normalised
// so that no slice is empty.  Measured at dim = ffn_dim = 4096, E = 8, k = 2
// (profiles/moe_ffn_mxfp4.txt, "mxfp4_only[sS]" lines): one slice is the
// fastest at every N from 64 to 4096, by 0.3 to 4 % over two (77.9 / 78.7 us
// at N = 64, 211.8 / 220.6 at 256, with window spreads of 0.1 to 0.3 us);
// four and eight lose 3 to 21 %.  Unlike the int4 lane, whose waves carry 48
// partial sums at two waves per SIMD, this kernel runs four waves per SIMD,
// which already hide a chunk's load latency.
#define MOE_MX_DOWN_SLICES 1

extern "C" int moe_ffn_mxfp4_plan(int F, int splits) {
  if (F < MX_CH || F % MX_CH) return 0;
  const int nch = F / MX_CH;
  int S = splits > 0 ? splits : MOE_MX_DOWN_SLICES;
  if (S > nch) {
    if (splits > 0) return 0;
    S = nch;
  }
  const int cps = (nch + S - 1) / S;
  return (nch + cps - 1) / cps;
}

// x bf16 [N,d]; gate_up_q u8 [E,2F,d/2], gate_up_s u8 [E,2F,d/32], down_q u8
// [E,d,F/2], down_s u8 [E,d,F/32]; weights f32 / idx i32 [N,top_k].
// Workspaces: xq u8 [N,d], xs f32 [N], sched i32 [max_tiles*32 + max_tiles +
// 1], h bf16 / hq u8 [max_tiles*32, F], hs f32 [max_tiles*32], y f32
// [S, N*top_k, d] with S = moe_ffn_mxfp4_plan(F, splits); out bf16 [N,d].
// Returns 0 once launched, non-zero (nothing launched) otherwise.
extern "C" int moe_ffn_mxfp4_bf16(
    const void* x, const void* gate_up_q, const void* gate_up_s,
    const void* down_q, const void* down_s, const float* weights,
    const int* idx, void* xq, float* xs, int* sched, void* h, void* hq,
    float* hs, float* y, void* out, long long N, int d, int F, int E,
    int top_k, int splits, hipStream_t stream) {
  if (!moe_shape_ok(N, E, top_k) || d < MX_CH || d % MX_CH) return 1;
  const int S = moe_ffn_mxfp4_plan(F, splits);
  if (S < 1) return 1;
  const int cps = (F / MX_CH + S - 1) / S;
  const int max_tiles = moe_max_tiles(N, top_k, E);
  const long long up_blocks = (long long)max_tiles * (F / 32);
  const long long down_blocks = (long long)max_tiles * (d / 64) * S;
  if (up_blocks >= (1ll << 31) || down_blocks >= (1ll << 31)) return 1;
  const int* slot_map = sched;
  const int* tile_expert = sched + (size_t)max_tiles * MOE_BM;
  const int* num_tiles = tile_expert + max_tiles;
  const int P = (int)(N * top_k);
  const long long plane = (long long)P * d;

  if (fp8_quant_rows_bf16(x, xq, xs, N, d, stream)) return 1;
  moe_align_launch(idx, P, E, max_tiles, sched, stream);
  hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<true>), dim3((unsigned)up_blocks),
                     dim3(WAVE), 0, stream, (const mx_u8*)xq,
                     (const float*)xs, (const mx_u8*)gate_up_q,
                     (const mx_u8*)gate_up_s, slot_map, tile_expert,
                     num_tiles, (short*)h, (float*)nullptr, d, F, top_k,
                     max_tiles, d / MX_CH, 0ll);
  if (fp8_quant_rows_tiles_bf16(h, hq, hs, (long long)max_tiles * MOE_BM, F,
                                num_tiles, MOE_BM, stream))
    return 1;
  hipLaunchKernelGGL((moe_gemm_mxfp4_kernel<false>),
                     dim3((unsigned)down_blocks), dim3(WAVE), 0, stream,
                     (const mx_u8*)hq, (const float*)hs, (const mx_u8*)down_q,
                     (const mx_u8*)down_s, slot_map, tile_expert, num_tiles,
                     (short*)nullptr, y, F, d, top_k, max_tiles, cps, plane);
  moe_combine_launch(y, weights, out, N, d, top_k, S, stream);
  return 0;
}
