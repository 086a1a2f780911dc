// The int4 weight recipe shared by the dense int4 linear (linear_w4.hip) and
// the int4 grouped GEMMs of the MoE FFN (moe.hip): one group of 128 k for a
// 32-row M-tile against NT 32-column N-tiles, from packed words to the fp32
// accumulators.  Format and the exponent-bias derivation: top of
// linear_w4.hip.  The kernels keep the addressing, the work split and the
// epilogues.  No torch dependency.
#pragma once

#include "attention_mfma32.h"

#define W4_G 128           // quantization group = K-chunk
#define W4_BIAS 136.f      // 128 from the exponent trick + 8 from u = q + 8

// New kernels are built without the packed fp32 VALU forms (v_pk_fma_f32 and
// its kin): the per-group scale step is sixteen independent fmas per tile and
// gains nothing from them.
#ifdef __HIP_DEVICE_COMPILE__
#define W4_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define W4_NO_PK_F32  // the host pass does not know the feature
#endif

// one group's operands of a lane: lane half hi5 owns k = hi5*64 .. +63 of the
// group — eight x fragments, and per N-tile eight packed words and a scale
template <int NT>
struct W4Frags {
  bf16x8 a[8];
  i32x4 b[NT][2];
  unsigned short s[NT];
};

// pa: this lane's x row + hi5*64; p[t]: its row of N-tile t's packed words
// + hi5*8; ps[t]: that row's scales.  ch = group index along K.
template <int NT>
DEV_INLINE void w4_load(W4Frags<NT>& f, const short* pa,
                        const int* const (&p)[NT],
                        const unsigned short* const (&ps)[NT], int ch,
                        short keep) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int* w = p[t] + ch * (W4_G / 8);
    f.b[t][0] = *(const i32x4*)w;
    f.b[t][1] = *(const i32x4*)(w + 4);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) f.s[t] = ps[t][ch];
  const short* a = pa + ch * W4_G;
  // keep is all ones, or zero on a row that does not exist: a mask, not a
  // select, so the load itself stays unconditional
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

// one group: biased products P per N-tile and the row sums X (shared by the
// tiles) by MFMA, then acc[t] += scale[t] * (P[t] - 136 X) in fp32
template <int NT>
DEV_INLINE void w4_mma(const W4Frags<NT>& f, f32x16 (&acc)[NT]) {
  const short one = 0x3F80;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};
  f32x16 p[NT], xs;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    xs[r] = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) p[t][r] = 0.f;
  }
#pragma unroll
  for (int s = 0; s < 8; ++s) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      p[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          f.a[s], w4_unpack(f.b[t][s >> 2][s & 3]), p[t], 0, 0, 0);
    xs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[s], ones, xs, 0, 0, 0);
  }
  float sc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) sc[t] = bf2f((short)f.s[t]);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t][r] = __builtin_fmaf(
          sc[t], __builtin_fmaf(-W4_BIAS, xs[r], p[t][r]), acc[t][r]);
  }
}

// All groups [ch0, ch1) of a slice, ascending, through two register sets in
// turn: the loads of group c + 1 are issued before the MFMAs of group c.
template <int NT>
DEV_INLINE void w4_groups(f32x16 (&acc)[NT], const short* pa,
                          const int* const (&p)[NT],
                          const unsigned short* const (&ps)[NT], int ch0,
                          int ch1, short keep) {
  W4Frags<NT> f0, f1;
  w4_load<NT>(f0, pa, p, ps, ch0, keep);
  int c = ch0;
  for (; c + 2 < ch1; c += 2) {
    w4_load<NT>(f1, pa, p, ps, c + 1, keep);
    w4_mma<NT>(f0, acc);
    w4_load<NT>(f0, pa, p, ps, c + 2, keep);
    w4_mma<NT>(f1, acc);
  }
  if (c + 1 < ch1) {
    w4_load<NT>(f1, pa, p, ps, c + 1, keep);
    w4_mma<NT>(f0, acc);
    w4_mma<NT>(f1, acc);
  } else {
    w4_mma<NT>(f0, acc);
  }
}
