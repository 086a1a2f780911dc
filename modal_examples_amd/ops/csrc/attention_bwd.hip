// Flash-attention backward for gfx950 — recompute-from-LSE, no atomics.
//
// The forward (attention_fwd32.hip) saves one fp32 log-sum-exp per query row.
// Three kernels turn (q, k, v, o, lse, dO) into (dq, dk, dv) with O(S) extra
// memory and bitwise-reproducible results (every sum has one owner and a
// fixed order; no float atomics, no workgroup waits on another):
//
//   fa_bwd_delta_kernel  delta[b,h,q] = sum_d dO*O (fp32), summed like dP
//   fa_bwd_dkdv_kernel   one workgroup per (batch, kv head, 128 keys); each
//                        wave keeps dK^T and dV^T of its 32 keys in
//                        accumulators while the workgroup sweeps the G query
//                        heads of the group and all 32-row query slices, so
//                        GQA's sum over the group happens in registers.
//   fa_bwd_dq_kernel     the forward's shape: one workgroup per 128 query
//                        rows, the query on the lane, sweeping key blocks.
//
// Both MFMA kernels recompute P = exp(s*scale - lse) directly (no running
// max, no rescale) and dS = P o (dP - delta); P and dS are rounded to bf16
// before their products, outputs to bf16 — reference.attention_bwd_ref with
// emulate_bf16=True rounds at the same places.
//
// Operand recipe (all of it the forward's, see the top of attention_fwd32.hip
// for the measured lane semantics):
//   dkdv: S = Q.K^T and dP = dO.V^T with the KEY on the lane (A = a row read
//     of the Q / dO LDS image, B = this lane's K / V row held in registers).
//     The C fragments (rows = query in registers, column = key on the lane)
//     become natural-k-order B operands by cvt_pk_bf16 + permlane32_swap,
//     exactly as the forward turns P into the B operand of P.V, and feed
//       dV^T += dO^T . P      dK^T += Q^T . dS
//     whose A operands dO^T / Q^T come from the SAME LDS image by
//     ds_read_b64_tr_b16 (the forward's V^T read).
//   dq: S^T = K.Q^T and dP^T = V.dO^T with the QUERY on the lane (Q and dO
//     rows in registers), dS^T = P^T o (dP^T - delta) lane-local, and
//       dQ^T += K^T . dS^T
//     with K^T read transposed from the K tile where the forward reads V^T.
#include "common.h"

#define FAB_NWAVES 4
#define FAB_PPAD 8
#define FAB_BLK 32  // rows per LDS tile: kv rows (dq) / query rows (dkdv)

typedef __attribute__((ext_vector_type(16))) float fab_f32x16;
typedef __attribute__((ext_vector_type(4))) short fab_bf16x4;
typedef __attribute__((address_space(3))) fab_bf16x4* fab_lds_tr_ptr;
typedef __attribute__((ext_vector_type(2))) int fab_i32x2;

DEV_INLINE int fab_swz(int row, int byte_off) {
  return byte_off ^ (((row >> 3) & 3) << 4);
}

DEV_INLINE unsigned fab_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// element strides of the [B,H,S,D]-logical, d-contiguous tensors
struct FABwdStrides {
  long long qb, qh, qs, kb, kh, ks, vb, vh, vs, ob, oh, os;
  long long gb, gh, gs;  // dO
  long long dqb, dqh, dqs, dkb, dkh, dks, dvb, dvh, dvs;
};

// row of a 32x32 C fragment held in register r by lane half hi5
DEV_INLINE int fab_crow(int r, int hi5) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi5;
}

// Row read of a [FAB_BLK][D+PPAD] swizzled tile as the A operand of a
// 32x32x16 MFMA: lane holds T[l31][c*16 + hi5*8 + j].
template <int KROW>
DEV_INLINE bf16x8 fab_row_frag(const short* tile, int l31, int hi5, int c) {
  return *(const bf16x8*)((const char*)tile + l31 * (KROW * 2) +
                          fab_swz(l31, (c * 16 + hi5 * 8) * 2));
}

// Transposed read of the same tile as the A operand T^T: lane holds
// T[c*16 + hi5*8 + j][dt*32 + l31] (the forward's V^T read).
template <int KROW>
DEV_INLINE bf16x8 fab_tr_frag(const short* tile, int l, int hi5, int c,
                              int dt) {
  int row0 = c * 16 + hi5 * 8 + ((l & 15) >> 2);
  int dbase = dt * 32 + ((l >> 4) & 1) * 16 + ((l & 3) * 4);
  fab_bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((fab_lds_tr_ptr)(
      (char*)tile + row0 * (KROW * 2) + fab_swz(row0, dbase * 2)));
  fab_bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((fab_lds_tr_ptr)(
      (char*)tile + (row0 + 4) * (KROW * 2) + fab_swz(row0 + 4, dbase * 2)));
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[j] = lo[j];
    f[j + 4] = hi[j];
  }
  return f;
}

// C fragment (rows in registers) -> the two natural-k-order bf16 B fragments
// of the 16-row chunks 0 and 1 (the forward's P recipe).
DEV_INLINE void fab_acc_to_bfrag(const fab_f32x16& x, bf16x8 out[2]) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    int pk01 = (int)fab_cvt_pk_bf16(x[c * 8 + 0], x[c * 8 + 1]);
    int pk23 = (int)fab_cvt_pk_bf16(x[c * 8 + 2], x[c * 8 + 3]);
    int pk45 = (int)fab_cvt_pk_bf16(x[c * 8 + 4], x[c * 8 + 5]);
    int pk67 = (int)fab_cvt_pk_bf16(x[c * 8 + 6], x[c * 8 + 7]);
    fab_i32x2 a = __builtin_amdgcn_permlane32_swap(pk01, pk45, false, false);
    fab_i32x2 b = __builtin_amdgcn_permlane32_swap(pk23, pk67, false, false);
    union {
      int w[4];
      bf16x8 v;
    } u;
    u.w[0] = a[0];
    u.w[1] = b[0];
    u.w[2] = a[1];
    u.w[3] = b[1];
    out[c] = u.v;
  }
}

// ------------------------------------------------------------------ delta
// delta[b,h,q] = sum_d dO[b,h,q,d] * O[b,h,q,d], one wave per 32 rows, as
// the diagonal of the 32x32 MFMA product dO.O^T.  It is summed by the same
// instruction chain (operand order, k chunks) as dP = dO.V^T in the kernels
// below, so the cancellation in dP - delta sees two sums rounded alike — a
// row that attends to a single key (o == v) gets dS == 0 exactly.
template <int D>
__global__ __launch_bounds__(FAB_NWAVES * WAVE) void fa_bwd_delta_kernel(
    const short* __restrict__ O, const short* __restrict__ dO,
    float* __restrict__ delta, int Hq, int Sq, FABwdStrides st) {
  constexpr int DCH = D / 16;
  const int w = threadIdx.x / WAVE;
  const int l = threadIdx.x % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int my_q = blockIdx.x * (32 * FAB_NWAVES) + w * 32 + l31;
  const bool q_ok = my_q < Sq;
  const long long oro = b * st.ob + h * st.oh + (long long)my_q * st.os;
  const long long gro = b * st.gb + h * st.gh + (long long)my_q * st.gs;
  fab_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int c = 0; c < DCH; ++c) {
    bf16x8 of = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    bf16x8 gf = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (q_ok) {
      of = *(const bf16x8*)&O[oro + c * 16 + hi5 * 8];
      gf = *(const bf16x8*)&dO[gro + c * 16 + hi5 * 8];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf, of, acc, 0, 0, 0);
  }
  // C[row = fab_crow(r, hi5)][col = l31]: the diagonal element of column l31
  // sits in the lane half hi5 == bit 2 of l31, register (l31&3) + 4*(l31>>3)
  const int rsel = (l31 & 3) + 4 * (l31 >> 3);
  float dsum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) dsum = (r == rsel) ? acc[r] : dsum;
  if (q_ok && ((l31 >> 2) & 1) == hi5)
    delta[((long long)b * Hq + h) * Sq + my_q] = dsum;
}

// ------------------------------------------------------------------ dK, dV
template <int D, bool CAUSAL>
__global__ __launch_bounds__(FAB_NWAVES * WAVE) void fa_bwd_dkdv_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    short* __restrict__ dK, short* __restrict__ dV, int B, int Hq, int Hkv,
    int Sq, int Sk, float scale, FABwdStrides st) {
  constexpr int KROW = D + FAB_PPAD;
  constexpr int DCH = D / 16;
  constexpr int DT = D / 32;
  constexpr int KBLK = 32 * FAB_NWAVES;  // keys per workgroup

  __shared__ alignas(16) short Qs[FAB_BLK][KROW];
  __shared__ alignas(16) short Gs[FAB_BLK][KROW];  // dO
  __shared__ alignas(16) float lse_s[FAB_BLK];
  __shared__ alignas(16) float delta_s[FAB_BLK];

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;

  const int hkv = blockIdx.y;
  const int b = blockIdx.z;
  const int G = Hq / Hkv;
  const int k0 = blockIdx.x * KBLK;
  const int my_k = k0 + w * 32 + l31;  // this lane's key
  const bool k_ok = my_k < Sk;
  const int causal_off = Sk - Sq;

  // this lane's K and V rows: the B operands of S = Q.K^T and dP = dO.V^T
  bf16x8 kreg[DCH], vreg[DCH];
  {
    const long long kro = b * st.kb + hkv * st.kh + (long long)my_k * st.ks;
    const long long vro = b * st.vb + hkv * st.vh + (long long)my_k * st.vs;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      if (k_ok) {
        kreg[c] = *(const bf16x8*)&K[kro + c * 16 + hi5 * 8];
        vreg[c] = *(const bf16x8*)&V[vro + c * 16 + hi5 * 8];
      } else {
        kreg[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        vreg[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  }

  fab_f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk[dt][r] = 0.f;
      dv[dt][r] = 0.f;
    }

  // query slices of 32 rows; under the causal mask slices wholly above the
  // diagonal of this key block (last row + causal_off < k0) are skipped
  const int nqb = (Sq + FAB_BLK - 1) / FAB_BLK;
  int qb_start = 0;
  if (CAUSAL && k0 - causal_off > 0) qb_start = (k0 - causal_off) / FAB_BLK;
  const int nsl = nqb > qb_start ? nqb - qb_start : 0;
  const int total = G * nsl;  // (head of the group, slice), heads outermost

  constexpr int CPR = D / 8;
  constexpr int CPT = (FAB_BLK * CPR) / (FAB_NWAVES * WAVE);
  bf16x8 qst[CPT], gst[CPT];
  float lse_st = 0.f, delta_st = 0.f;
  auto load_slice = [&](int it) {
    const int g = it / nsl;
    const int q0 = (qb_start + it % nsl) * FAB_BLK;
    const int h = hkv * G + g;
    const long long qoff = b * st.qb + h * st.qh;
    const long long goff = b * st.gb + h * st.gh;
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int ci = i * FAB_NWAVES * WAVE + tid;
      int row = ci / CPR, c8 = ci % CPR;
      int qp = q0 + row;
      if (qp < Sq) {
        qst[i] = *(const bf16x8*)&Q[qoff + (long long)qp * st.qs + c8 * 8];
        gst[i] = *(const bf16x8*)&dO[goff + (long long)qp * st.gs + c8 * 8];
      } else {
        qst[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        gst[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    if (tid < FAB_BLK) {
      int qp = q0 + tid;
      bool ok = qp < Sq;
      long long ro = ((long long)b * Hq + h) * Sq + qp;
      lse_st = ok ? LSE[ro] : 0.f;
      delta_st = ok ? DELTA[ro] : 0.f;
    }
  };
  auto write_slice = [&]() {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int ci = i * FAB_NWAVES * WAVE + tid;
      int row = ci / CPR, c8 = ci % CPR;
      int boff = fab_swz(row, c8 * 16);
      *(bf16x8*)((char*)&Qs[row][0] + boff) = qst[i];
      *(bf16x8*)((char*)&Gs[row][0] + boff) = gst[i];
    }
    if (tid < FAB_BLK) {
      lse_s[tid] = lse_st;
      delta_s[tid] = delta_st;
    }
  };

  if (total > 0) load_slice(0);
  for (int it = 0; it < total; ++it) {
    const int q0 = (qb_start + it % nsl) * FAB_BLK;
    __syncthreads();
    write_slice();
    __syncthreads();
    if (it + 1 < total) load_slice(it + 1);

    // ---- S = Q.K^T, dP = dO.V^T: rows = query (registers), col = key ----
    fab_f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = 0.f;
      dp[r] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      bf16x8 qf = fab_row_frag<KROW>(&Qs[0][0], l31, hi5, c);
      bf16x8 gf = fab_row_frag<KROW>(&Gs[0][0], l31, hi5, c);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kreg[c], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf, vreg[c], dp, 0, 0, 0);
    }

    // ---- P = exp(s*scale - lse), dS = P o (dP - delta); masked -> 0 ----
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      f32x4 lse4 = *(const f32x4*)&lse_s[8 * g4 + 4 * hi5];
      f32x4 del4 = *(const f32x4*)&delta_s[8 * g4 + 4 * hi5];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int r = 4 * g4 + j;
        int qp = q0 + 8 * g4 + 4 * hi5 + j;  // == q0 + fab_crow(r, hi5)
        bool dead = !k_ok || qp >= Sq || (CAUSAL && my_k > qp + causal_off);
        float p = dead ? 0.f : __expf(s[r] * scale - lse4[j]);
        s[r] = p;
        dp[r] = p * (dp[r] - del4[j]);
      }
    }
    bf16x8 pfrag[2], dsfrag[2];
    fab_acc_to_bfrag(s, pfrag);
    fab_acc_to_bfrag(dp, dsfrag);

    // ---- dV^T += dO^T . P ; dK^T += Q^T . dS ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        bf16x8 gt = fab_tr_frag<KROW>(&Gs[0][0], l, hi5, c, dt);
        bf16x8 qt = fab_tr_frag<KROW>(&Qs[0][0], l, hi5, c, dt);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gt, pfrag[c], dv[dt],
                                                         0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qt, dsfrag[c], dk[dt],
                                                         0, 0, 0);
      }
    }
  }

  // ---- epilogue: dK[key][d] = scale * dK^T[d][key], dV[key][d] ----
  if (k_ok) {
    const long long dko =
        b * st.dkb + hkv * st.dkh + (long long)my_k * st.dks;
    const long long dvo =
        b * st.dvb + hkv * st.dvh + (long long)my_k * st.dvs;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = dt * 32 + fab_crow(r, hi5);
        dK[dko + d] = f2bf(dk[dt][r] * scale);
        dV[dvo + d] = f2bf(dv[dt][r]);
      }
  }
}

// ------------------------------------------------------------------ dQ
template <int D, bool CAUSAL>
__global__ __launch_bounds__(FAB_NWAVES * WAVE) void fa_bwd_dq_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    short* __restrict__ dQ, int B, int Hq, int Hkv, int Sq, int Sk,
    float scale, FABwdStrides st) {
  constexpr int KROW = D + FAB_PPAD;
  constexpr int DCH = D / 16;
  constexpr int DT = D / 32;
  constexpr int QBLK = 32 * FAB_NWAVES;
  constexpr int KVB = FAB_BLK;

  __shared__ alignas(16) short Ks[KVB][KROW];
  __shared__ alignas(16) short Vs[KVB][KROW];

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;

  const int qblk = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);

  const long long koff = b * st.kb + hkv * st.kh;
  const long long voff = b * st.vb + hkv * st.vh;
  const int my_q = qblk * QBLK + w * 32 + l31;  // this lane's query row
  const bool q_ok = my_q < Sq;
  const int causal_off = Sk - Sq;

  // this lane's Q and dO rows (B operands) and its row constants
  bf16x8 qreg[DCH], greg[DCH];
  float lse_q = 0.f, delta_q = 0.f;
  {
    const long long qro = b * st.qb + h * st.qh + (long long)my_q * st.qs;
    const long long gro = b * st.gb + h * st.gh + (long long)my_q * st.gs;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      if (q_ok) {
        qreg[c] = *(const bf16x8*)&Q[qro + c * 16 + hi5 * 8];
        greg[c] = *(const bf16x8*)&dO[gro + c * 16 + hi5 * 8];
      } else {
        qreg[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        greg[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    if (q_ok) {
      long long ro = ((long long)b * Hq + h) * Sq + my_q;
      lse_q = LSE[ro];
      delta_q = DELTA[ro];
    }
  }

  fab_f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;

  int nkb = (Sk + KVB - 1) / KVB;
  if (CAUSAL) {
    int max_kv = qblk * QBLK + QBLK - 1 + causal_off;
    int lim = (max_kv + KVB) / KVB;
    if (lim < nkb) nkb = lim;
  }

  constexpr int CPR = D / 8;
  constexpr int CPT = (KVB * CPR) / (FAB_NWAVES * WAVE);
  bf16x8 kst[CPT], vst[CPT];
  auto load_chunks = [&](int kb) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int ci = i * FAB_NWAVES * WAVE + tid;
      int row = ci / CPR, c8 = ci % CPR;
      int kvp = kb * KVB + row;
      if (kvp < Sk) {
        kst[i] = *(const bf16x8*)&K[koff + (long long)kvp * st.ks + c8 * 8];
        vst[i] = *(const bf16x8*)&V[voff + (long long)kvp * st.vs + c8 * 8];
      } else {
        kst[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        vst[i] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };
  auto write_chunks = [&]() {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      int ci = i * FAB_NWAVES * WAVE + tid;
      int row = ci / CPR, c8 = ci % CPR;
      int boff = fab_swz(row, c8 * 16);
      *(bf16x8*)((char*)&Ks[row][0] + boff) = kst[i];
      *(bf16x8*)((char*)&Vs[row][0] + boff) = vst[i];
    }
  };

  if (nkb > 0) load_chunks(0);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    write_chunks();
    __syncthreads();
    if (kb + 1 < nkb) load_chunks(kb + 1);

    // ---- S^T = K.Q^T, dP^T = V.dO^T: rows = key (registers), col = query
    fab_f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = 0.f;
      dp[r] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      bf16x8 kf = fab_row_frag<KROW>(&Ks[0][0], l31, hi5, c);
      bf16x8 vf = fab_row_frag<KROW>(&Vs[0][0], l31, hi5, c);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qreg[c], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, greg[c], dp, 0, 0, 0);
    }

    // ---- dS^T = P^T o (dP^T - delta); masked -> 0 ----
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int kvp = kb * KVB + fab_crow(r, hi5);
      bool dead = !q_ok || kvp >= Sk || (CAUSAL && kvp > my_q + causal_off);
      float p = dead ? 0.f : __expf(s[r] * scale - lse_q);
      dp[r] = p * (dp[r] - delta_q);
    }
    bf16x8 dsfrag[2];
    fab_acc_to_bfrag(dp, dsfrag);

    // ---- dQ^T += K^T . dS^T (K^T via transposed reads of the K tile) ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        bf16x8 kt = fab_tr_frag<KROW>(&Ks[0][0], l, hi5, c, dt);
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, dsfrag[c],
                                                          acc[dt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: dQ[q][d] = scale * dQ^T[d][q] ----
  if (q_ok) {
    const long long dqo = b * st.dqb + h * st.dqh + (long long)my_q * st.dqs;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = dt * 32 + fab_crow(r, hi5);
        dQ[dqo + d] = f2bf(acc[dt][r] * scale);
      }
  }
}

// q/k/v/o/dout and dq/dk/dv are logically [B,H,S,D] with d contiguous;
// strides[24] holds the element strides (batch, head, sequence) of
// q k v o dout dq dk dv in that order.  lse and delta are fp32 [B,Hq,Sq]
// contiguous; delta is scratch that the preprocess kernel fills.  Returns 0
// once the three kernels are launched, non-zero (nothing launched) for an
// unsupported configuration: D must be 64 or 128, Hq a multiple of Hkv,
// Sq and Sk at least 1, and causal needs Sk >= Sq.
extern "C" int fa_bwd_strided_bf16(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, float* delta, void* dq, void* dk,
    void* dv, int B, int Hq, int Hkv, int Sq, int Sk, int D, float scale,
    int causal, const long long* strides, hipStream_t stream) {
  if ((D != 64 && D != 128) || Hkv <= 0 || Hq % Hkv != 0) return 1;
  if (B < 1 || Sq < 1 || Sk < 1 || (causal && Sk < Sq)) return 1;
  FABwdStrides st;
  st.qb = strides[0]; st.qh = strides[1]; st.qs = strides[2];
  st.kb = strides[3]; st.kh = strides[4]; st.ks = strides[5];
  st.vb = strides[6]; st.vh = strides[7]; st.vs = strides[8];
  st.ob = strides[9]; st.oh = strides[10]; st.os = strides[11];
  st.gb = strides[12]; st.gh = strides[13]; st.gs = strides[14];
  st.dqb = strides[15]; st.dqh = strides[16]; st.dqs = strides[17];
  st.dkb = strides[18]; st.dkh = strides[19]; st.dks = strides[20];
  st.dvb = strides[21]; st.dvh = strides[22]; st.dvs = strides[23];
  const short* Qp = (const short*)q;
  const short* Kp = (const short*)k;
  const short* Vp = (const short*)v;
  const short* Op = (const short*)o;
  const short* Gp = (const short*)dout;
  short* dQp = (short*)dq;
  short* dKp = (short*)dk;
  short* dVp = (short*)dv;

  dim3 block(FAB_NWAVES * WAVE);
  dim3 grid_kv((Sk + 127) / 128, Hkv, B);
  dim3 grid_q((Sq + 127) / 128, Hq, B);
#define FAB_LAUNCH(DD, CC)                                                    \
  do {                                                                        \
    hipLaunchKernelGGL((fa_bwd_delta_kernel<DD>), grid_q, block, 0, stream,   \
                       Op, Gp, delta, Hq, Sq, st);                            \
    hipLaunchKernelGGL((fa_bwd_dkdv_kernel<DD, CC>), grid_kv, block, 0,       \
                       stream, Qp, Kp, Vp, Gp, lse, delta, dKp, dVp, B, Hq,   \
                       Hkv, Sq, Sk, scale, st);                               \
    hipLaunchKernelGGL((fa_bwd_dq_kernel<DD, CC>), grid_q, block, 0, stream,  \
                       Qp, Kp, Vp, Gp, lse, delta, dQp, B, Hq, Hkv, Sq, Sk,   \
                       scale, st);                                            \
  } while (0)
  if (D == 64) {
    if (causal) FAB_LAUNCH(64, true); else FAB_LAUNCH(64, false);
  } else {
    if (causal) FAB_LAUNCH(128, true); else FAB_LAUNCH(128, false);
  }
#undef FAB_LAUNCH
  return 0;
}
