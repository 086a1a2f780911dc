// The block-scaled fp4 MFMA recipe shared by linear_mxfp4.hip (dense) and
// moe_mxfp4.hip (grouped, per-expert): one 128-k chunk of an e4m3 A operand
// against OCP MXFP4 weights and their E8M0 block scales, as loaded, through
// v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz = 0, blgp = 4).  The operand layout,
// the k bookkeeping of a chunk and the probe lines that establish them are in
// linear_mxfp4.hip's header; nothing here knows where a row's bytes come
// from — the callers build the per-lane row pointers.
#pragma once
#include "attention_mfma32.h"  // f32x16, c_row

#define MX_CH 128  // k per chunk: four MX blocks, two per lane half
#define MX_BM 32   // rows per M-tile
#define MX_UNIT_SCALE 0x7F7F7F7F  // E8M0 127 = 2^0 in every byte

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef unsigned char mx_u8;

// one chunk's operands of a lane: 4 x 16 B of each of its MT x rows, 32 B
// and two scale bytes of each of its two weight rows, as loaded
template <int MT>
struct MxFrags {
  i32x4 a[MT][4];
  i32x4 b[2][2];
  int s[2];
};

// pa[t]: this lane's x row of M-tile t, + hi5*16; pb[f] / ps[f]: its weight
// row of N-fragment f, + hi5*32 bytes / + hi5*2 scale bytes
template <int MT>
DEV_INLINE void mx_load(MxFrags<MT>& f, const mx_u8* const* pa,
                        const mx_u8* const* pb, const mx_u8* const* ps,
                        int ch) {
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const i32x4* w = (const i32x4*)(pb[n] + (size_t)ch * (MX_CH / 2));
    f.b[n][0] = w[0];
    f.b[n][1] = w[1];
    f.s[n] = *(const unsigned short*)(ps[n] + (size_t)ch * (MX_CH / 32));
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const i32x4* a = (const i32x4*)(pa[t] + (size_t)ch * MX_CH);
#pragma unroll
    for (int q = 0; q < 4; ++q) f.a[t][q] = a[2 * q];  // bytes 16h + 32q
  }
}

DEV_INLINE i32x8 mx_operand8(i32x4 lo, i32x4 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the fp4 operand: four registers, the upper four of the builtin's type are
// not read (probe: "upper four B registers ignored")
DEV_INLINE i32x8 mx_operand4(i32x4 lo) {
  return __builtin_shufflevector(lo, lo, 0, 1, 2, 3, -1, -1, -1, -1);
}

// one chunk: two K=64 MFMAs per fragment.  MFMA j takes weight bytes j*16 ..
// j*16+15 and scale byte j of every lane's share, against x loads j and
// 2 + j (linear_mxfp4.hip's header has the k bookkeeping).
template <int MT>
DEV_INLINE void mx_mma(const MxFrags<MT>& f, f32x16 (&acc)[MT][2]) {
#pragma unroll
  for (int n = 0; n < 2; ++n) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
      acc[t][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          mx_operand8(f.a[t][0], f.a[t][2]), mx_operand4(f.b[n][0]),
          acc[t][n], 0 /* A: e4m3 */, 4 /* B: e2m1 */, 0, MX_UNIT_SCALE,
          0 /* scale byte 0 */, f.s[n]);
  }
#pragma unroll
  for (int n = 0; n < 2; ++n) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
      acc[t][n] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          mx_operand8(f.a[t][1], f.a[t][3]), mx_operand4(f.b[n][1]),
          acc[t][n], 0, 4, 0, MX_UNIT_SCALE, 1 /* scale byte 1 */, f.s[n]);
  }
}

// all chunks [ch0, ch1) ascending through two register sets in turn, the
// loads of chunk i+1 issued before the MFMAs of chunk i; ch0 < ch1
template <int MT>
DEV_INLINE void mx_chunks(f32x16 (&acc)[MT][2], const mx_u8* const* pa,
                          const mx_u8* const* pb, const mx_u8* const* ps,
                          int ch0, int ch1) {
  MxFrags<MT> f0, f1;
  mx_load<MT>(f0, pa, pb, ps, ch0);
  int c = ch0;
  for (; c + 2 < ch1; c += 2) {
    mx_load<MT>(f1, pa, pb, ps, c + 1);
    mx_mma<MT>(f0, acc);
    mx_load<MT>(f0, pa, pb, ps, c + 2);
    mx_mma<MT>(f1, acc);
  }
  if (c + 1 < ch1) {
    mx_load<MT>(f1, pa, pb, ps, c + 1);
    mx_mma<MT>(f0, acc);
    mx_mma<MT>(f1, acc);
  } else {
    mx_mma<MT>(f0, acc);
  }
}
