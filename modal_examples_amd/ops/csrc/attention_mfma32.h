// The 32x32x16 bf16 MFMA operand recipe shared by the attention forward
// (attention_fwd32.hip) and backward (attention_bwd.hip): how a [rows][D+8]
// LDS tile is written, read row-wise and read transposed, and how a C
// fragment becomes the next product's B operand without leaving registers.
// Helpers here only address, load, pack and shuffle — the arithmetic (scale,
// exp, masks, softmax, every MFMA) stays in the kernels.  No torch dependency.
//
// Fragment layouts (verified on-device, scripts/probe_mfma32.cpp), with
// l31 = lane & 31 and hi5 = lane >> 5:
//   A[m][k]: lane holds A[l31][hi5*8 + j];   B[k][n]: B[hi5*8 + j][l31]
//   C[m][n]: lane holds C[c_row(reg, hi5)][l31], reg 0..15.
// Computing a product TRANSPOSED (S^T = K.Q^T) therefore puts 16 rows of one
// column — one query's scores — on a lane; its partner lane^32 holds the rest.
#pragma once

#include "common.h"

#include <cstring>

#define FA_PPAD 8  // bf16 of padding per LDS tile row: pitch D + 8

typedef __attribute__((ext_vector_type(16))) float f32x16;  // 32x32 C fragment
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((address_space(3))) bf16x4* lds_tr_ptr;

DEV_INLINE bf16x8 bf16x8_zero() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// XOR row swizzle of a tile's byte offset within a row: 16 B chunks move by
// (row>>3)&3, which keeps both the row reads and the transposed reads below
// off each other's banks.  Stores and reads go through the same function.
DEV_INLINE int tile_swz(int row, int byte_off) {
  return byte_off ^ (((row >> 3) & 3) << 4);
}

// two f32 -> one word of two bf16 (lo in the low half); no builtin on gfx950
DEV_INLINE unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// row of a 32x32 C fragment held in register r by lane half hi5
DEV_INLINE int c_row(int r, int hi5) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi5;
}

// Row read of a swizzled tile (row pitch KROW bf16) as the A operand:
// lane holds T[row][c*16 + hi5*8 + j], row = this lane's l31 (+ 32*fragment).
template <int KROW>
DEV_INLINE bf16x8 row_frag(const short* tile, int row, int hi5, int c) {
  return *(const bf16x8*)((const char*)tile + row * (KROW * 2) +
                          tile_swz(row, (c * 16 + hi5 * 8) * 2));
}

// Transposed read of the same tile as the A operand T^T: lane holds
// T[c*16 + hi5*8 + j][dt*32 + l31].  ds_read_b64_tr_b16 semantics, measured
// (scripts/probe_tr16.cpp; the documented behaviour is wrong on this part):
// a 4x4 lane-grid exchange per 16-lane group — lane 4a+b issues the source
// read of row (l&15)>>2 at columns 4b..4b+3 and receives halfword b of lane
// 4j+a's read.  So lane l reads
//   T[c*16 + hi5*8 + ((l&15)>>2) (+4)][dt*32 + ((l>>4)&1)*16 + (l&3)*4 ..]
// and the two reads 4 rows apart make the 8 k-values of the fragment.
template <int KROW>
DEV_INLINE bf16x8 tr_frag(const short* tile, int l, int hi5, int c, int dt) {
  int row0 = c * 16 + hi5 * 8 + ((l & 15) >> 2);
  int dbase = dt * 32 + ((l >> 4) & 1) * 16 + ((l & 3) * 4);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(
      (char*)tile + row0 * (KROW * 2) + tile_swz(row0, dbase * 2)));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(
      (char*)tile + (row0 + 4) * (KROW * 2) + tile_swz(row0 + 4, dbase * 2)));
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = lo[j];
    f[j + 4] = hi[j];
  }
  return f;
}

// Half a C fragment (8 registers sv[0..7] = 16 rows across the lane pair)
// -> the natural-k-order bf16 B fragment of that 16-row chunk, in registers.
// Own registers pack row pairs; permlane32_swap (semantics measured: the
// result pair is (A_lo||B_lo, A_hi||B_hi)) exchanges halves with lane^32:
//   words = [A'(pk01,pk45), A'(pk23,pk67), B'(same), B'(same)]
// Takes a pointer, not the fragment: indexing a const f32x16& here cost the
// D=64 non-causal forward 8 VGPRs and one wave per SIMD.
DEV_INLINE bf16x8 c8_to_bfrag(const float* sv) {
  int pk01 = (int)cvt_pk_bf16(sv[0], sv[1]);
  int pk23 = (int)cvt_pk_bf16(sv[2], sv[3]);
  int pk45 = (int)cvt_pk_bf16(sv[4], sv[5]);
  int pk67 = (int)cvt_pk_bf16(sv[6], sv[7]);
  i32x2 x = __builtin_amdgcn_permlane32_swap(pk01, pk45, false, false);
  i32x2 y = __builtin_amdgcn_permlane32_swap(pk23, pk67, false, false);
  union {
    int w[4];
    bf16x8 v;
  } u;
  u.w[0] = x[0];
  u.w[1] = y[0];
  u.w[2] = x[1];
  u.w[3] = y[1];
  return u.v;
}

// Both values of a lane pair (lane, lane^32), in registers: lo is the value
// of the pair's lane below 32, hi the one above, the same on both lanes.
// One permlane32_swap of x with itself (semantics above) instead of a
// ds_bpermute round trip and its full LDS wait.  The results go through
// plain ints: __builtin_bit_cast applied to r[1] itself reads r[0].
DEV_INLINE void lane_pair(float x, float& lo, float& hi) {
  int xi = __builtin_bit_cast(int, x);
  i32x2 r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
  int r0 = r[0], r1 = r[1];
  lo = __builtin_bit_cast(float, r0);
  hi = __builtin_bit_cast(float, r1);
}

// Two-tile staging, global -> registers -> swizzled LDS, split so the loads
// of the next block issue before this block computes.  a/b point at row 0 of
// the (batch, head) plane, *_rs are their row strides in elements; tile rows
// row0..row0+ROWS-1, zero past nrows.  NT threads move ROWS*D/8 16 B chunks.
template <int D, int ROWS, int NT>
DEV_INLINE void stage_load(const short* a, long long a_rs, const short* b,
                           long long b_rs, int row0, int nrows, int tid,
                           bf16x8 (&ra)[ROWS * (D / 8) / NT],
                           bf16x8 (&rb)[ROWS * (D / 8) / NT]) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int i = 0; i < ROWS * CPR / NT; ++i) {
    int ci = i * NT + tid;
    int row = ci / CPR, c8 = ci % CPR;
    int gr = row0 + row;
    if (gr < nrows) {
      ra[i] = *(const bf16x8*)&a[gr * a_rs + c8 * 8];
      rb[i] = *(const bf16x8*)&b[gr * b_rs + c8 * 8];
    } else {
      ra[i] = bf16x8_zero();
      rb[i] = bf16x8_zero();
    }
  }
}

template <int D, int ROWS, int NT>
DEV_INLINE void stage_write(short* ta, short* tb, int tid,
                            const bf16x8 (&ra)[ROWS * (D / 8) / NT],
                            const bf16x8 (&rb)[ROWS * (D / 8) / NT]) {
  constexpr int CPR = D / 8;
#pragma unroll
  for (int i = 0; i < ROWS * CPR / NT; ++i) {
    int ci = i * NT + tid;
    int row = ci / CPR, c8 = ci % CPR;
    int off = row * ((D + FA_PPAD) * 2) + tile_swz(row, c8 * 16);
    *(bf16x8*)((char*)ta + off) = ra[i];
    *(bf16x8*)((char*)tb + off) = rb[i];
  }
}

// Element strides (batch, head, sequence) of a [B,H,S,D]-logical tensor with
// d contiguous.  The launchers take the flat image of these structs: three
// long long per tensor, in member order.
struct AttnStride {
  long long b, h, s;
};
struct AttnFwdStrides {
  AttnStride q, k, v, o;
};
struct AttnBwdStrides {
  AttnStride q, k, v, o, g, dq, dk, dv;  // g = dO
};

template <typename S>
inline S attn_strides_from(const long long* flat) {
  static_assert(sizeof(S) % sizeof(AttnStride) == 0, "triples only");
  S st;
  memcpy(&st, flat, sizeof(S));
  return st;
}

// what both launchers support: head dim 64 or 128, Hq a multiple of Hkv
inline bool attn_mfma32_supported(int D, int Hq, int Hkv) {
  return (D == 64 || D == 128) && Hkv > 0 && Hq % Hkv == 0;
}
