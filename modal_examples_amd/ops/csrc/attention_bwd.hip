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
// Operand recipe: all of it is the forward's, and both files take it from
// attention_mfma32.h (tile image, row_frag / tr_frag reads, c8_to_bfrag):
//   dkdv: S = Q.K^T and dP = dO.V^T with the KEY on the lane (A = a row read
//     of the Q / dO LDS image, B = this lane's K / V row held in registers).
//     The C fragments (rows = query in registers, column = key on the lane)
//     become natural-k-order B operands exactly as the forward turns P into
//     the B operand of P.V, and feed
//       dV^T += dO^T . P      dK^T += Q^T . dS
//     whose A operands dO^T / Q^T are transposed reads of the SAME LDS image.
//   dq: S^T = K.Q^T and dP^T = V.dO^T with the QUERY on the lane (Q and dO
//     rows in registers), dS^T = P^T o (dP^T - delta) lane-local, and
//       dQ^T += K^T . dS^T
//     with K^T read transposed from the K tile where the forward reads V^T.
#include "attention_mfma32.h"

#define FA_BWD_NWAVES 4
#define FA_BWD_BLK 32  // rows per LDS tile: kv rows (dq) / query rows (dkdv)
#define FA_BWD_NT (FA_BWD_NWAVES * WAVE)

// ------------------------------------------------------------------ delta
// delta[b,h,q] = sum_d dO[b,h,q,d] * O[b,h,q,d], one wave per 32 rows, as
// the diagonal of the 32x32 MFMA product dO.O^T.  It is summed by the same
// instruction chain (operand order, k chunks) as dP = dO.V^T in the kernels
// below, so the cancellation in dP - delta sees two sums rounded alike — a
// row that attends to a single key (o == v) gets dS == 0 exactly.
template <int D>
__global__ __launch_bounds__(FA_BWD_NT) void fa_bwd_delta_kernel(
    const short* __restrict__ O, const short* __restrict__ dO,
    float* __restrict__ delta, int Hq, int Sq, AttnBwdStrides st) {
  constexpr int DCH = D / 16;
  const int w = threadIdx.x / WAVE;
  const int l = threadIdx.x % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int my_q = blockIdx.x * (32 * FA_BWD_NWAVES) + w * 32 + l31;
  const bool q_ok = my_q < Sq;
  const long long oro = b * st.o.b + h * st.o.h + (long long)my_q * st.o.s;
  const long long gro = b * st.g.b + h * st.g.h + (long long)my_q * st.g.s;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int c = 0; c < DCH; ++c) {
    bf16x8 of = bf16x8_zero();
    bf16x8 gf = bf16x8_zero();
    if (q_ok) {
      of = *(const bf16x8*)&O[oro + c * 16 + hi5 * 8];
      gf = *(const bf16x8*)&dO[gro + c * 16 + hi5 * 8];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gf, of, acc, 0, 0, 0);
  }
  // C[row = c_row(r, hi5)][col = l31]: the diagonal element of column l31
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
__global__ __launch_bounds__(FA_BWD_NT) void fa_bwd_dkdv_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    short* __restrict__ dK, short* __restrict__ dV, int B, int Hq, int Hkv,
    int Sq, int Sk, float scale, AttnBwdStrides st) {
  constexpr int KROW = D + FA_PPAD;
  constexpr int DCH = D / 16;
  constexpr int DT = D / 32;
  constexpr int KBLK = 32 * FA_BWD_NWAVES;  // keys per workgroup

  __shared__ alignas(16) short Qs[FA_BWD_BLK][KROW];
  __shared__ alignas(16) short Gs[FA_BWD_BLK][KROW];  // dO
  __shared__ alignas(16) float lse_s[FA_BWD_BLK];
  __shared__ alignas(16) float delta_s[FA_BWD_BLK];

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
    const long long kro = b * st.k.b + hkv * st.k.h + (long long)my_k * st.k.s;
    const long long vro = b * st.v.b + hkv * st.v.h + (long long)my_k * st.v.s;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      if (k_ok) {
        kreg[c] = *(const bf16x8*)&K[kro + c * 16 + hi5 * 8];
        vreg[c] = *(const bf16x8*)&V[vro + c * 16 + hi5 * 8];
      } else {
        kreg[c] = bf16x8_zero();
        vreg[c] = bf16x8_zero();
      }
    }
  }

  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dk[dt][r] = 0.f;
      dv[dt][r] = 0.f;
    }

  // query slices of 32 rows; under the causal mask slices wholly above the
  // diagonal of this key block (last row + causal_off < k0) are skipped
  const int nqb = (Sq + FA_BWD_BLK - 1) / FA_BWD_BLK;
  int qb_start = 0;
  if (CAUSAL && k0 - causal_off > 0) qb_start = (k0 - causal_off) / FA_BWD_BLK;
  const int nsl = nqb > qb_start ? nqb - qb_start : 0;
  const int total = G * nsl;  // (head of the group, slice), heads outermost

  bf16x8 qst[FA_BWD_BLK * (D / 8) / FA_BWD_NT];
  bf16x8 gst[FA_BWD_BLK * (D / 8) / FA_BWD_NT];
  float lse_st = 0.f, delta_st = 0.f;
  auto load_slice = [&](int it) {
    const int g = it / nsl;
    const int q0 = (qb_start + it % nsl) * FA_BWD_BLK;
    const int h = hkv * G + g;
    stage_load<D, FA_BWD_BLK, FA_BWD_NT>(
        Q + (b * st.q.b + h * st.q.h), st.q.s, dO + (b * st.g.b + h * st.g.h),
        st.g.s, q0, Sq, tid, qst, gst);
    if (tid < FA_BWD_BLK) {
      int qp = q0 + tid;
      bool ok = qp < Sq;
      long long ro = ((long long)b * Hq + h) * Sq + qp;
      lse_st = ok ? LSE[ro] : 0.f;
      delta_st = ok ? DELTA[ro] : 0.f;
    }
  };
  auto write_slice = [&]() {
    stage_write<D, FA_BWD_BLK, FA_BWD_NT>(&Qs[0][0], &Gs[0][0], tid, qst,
                                          gst);
    if (tid < FA_BWD_BLK) {
      lse_s[tid] = lse_st;
      delta_s[tid] = delta_st;
    }
  };

  if (total > 0) load_slice(0);
  for (int it = 0; it < total; ++it) {
    const int q0 = (qb_start + it % nsl) * FA_BWD_BLK;
    __syncthreads();
    write_slice();
    __syncthreads();
    if (it + 1 < total) load_slice(it + 1);

    // ---- S = Q.K^T, dP = dO.V^T: rows = query (registers), col = key ----
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = 0.f;
      dp[r] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      bf16x8 qf = row_frag<KROW>(&Qs[0][0], l31, hi5, c);
      bf16x8 gf = row_frag<KROW>(&Gs[0][0], l31, hi5, c);
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
        int qp = q0 + 8 * g4 + 4 * hi5 + j;  // == q0 + c_row(r, hi5)
        bool dead = !k_ok || qp >= Sq || (CAUSAL && my_k > qp + causal_off);
        float p = dead ? 0.f : __expf(s[r] * scale - lse4[j]);
        s[r] = p;
        dp[r] = p * (dp[r] - del4[j]);
      }
    }
    bf16x8 pfrag[2], dsfrag[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      pfrag[c] = c8_to_bfrag((const float*)&s + c * 8);
      dsfrag[c] = c8_to_bfrag((const float*)&dp + c * 8);
    }

    // ---- dV^T += dO^T . P ; dK^T += Q^T . dS ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        bf16x8 gt = tr_frag<KROW>(&Gs[0][0], l, hi5, c, dt);
        bf16x8 qt = tr_frag<KROW>(&Qs[0][0], l, hi5, c, dt);
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
        b * st.dk.b + hkv * st.dk.h + (long long)my_k * st.dk.s;
    const long long dvo =
        b * st.dv.b + hkv * st.dv.h + (long long)my_k * st.dv.s;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = dt * 32 + c_row(r, hi5);
        dK[dko + d] = f2bf(dk[dt][r] * scale);
        dV[dvo + d] = f2bf(dv[dt][r]);
      }
  }
}

// ------------------------------------------------------------------ dQ
template <int D, bool CAUSAL>
__global__ __launch_bounds__(FA_BWD_NT) void fa_bwd_dq_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, const short* __restrict__ dO,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    short* __restrict__ dQ, int B, int Hq, int Hkv, int Sq, int Sk,
    float scale, AttnBwdStrides st) {
  constexpr int KROW = D + FA_PPAD;
  constexpr int DCH = D / 16;
  constexpr int DT = D / 32;
  constexpr int QBLK = 32 * FA_BWD_NWAVES;
  constexpr int KVB = FA_BWD_BLK;

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

  const long long koff = b * st.k.b + hkv * st.k.h;
  const long long voff = b * st.v.b + hkv * st.v.h;
  const int my_q = qblk * QBLK + w * 32 + l31;  // this lane's query row
  const bool q_ok = my_q < Sq;
  const int causal_off = Sk - Sq;

  // this lane's Q and dO rows (B operands) and its row constants
  bf16x8 qreg[DCH], greg[DCH];
  float lse_q = 0.f, delta_q = 0.f;
  {
    const long long qro = b * st.q.b + h * st.q.h + (long long)my_q * st.q.s;
    const long long gro = b * st.g.b + h * st.g.h + (long long)my_q * st.g.s;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      if (q_ok) {
        qreg[c] = *(const bf16x8*)&Q[qro + c * 16 + hi5 * 8];
        greg[c] = *(const bf16x8*)&dO[gro + c * 16 + hi5 * 8];
      } else {
        qreg[c] = bf16x8_zero();
        greg[c] = bf16x8_zero();
      }
    }
    if (q_ok) {
      long long ro = ((long long)b * Hq + h) * Sq + my_q;
      lse_q = LSE[ro];
      delta_q = DELTA[ro];
    }
  }

  f32x16 acc[DT];
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

  bf16x8 kst[KVB * (D / 8) / FA_BWD_NT], vst[KVB * (D / 8) / FA_BWD_NT];
  auto load_chunks = [&](int kb) {
    stage_load<D, KVB, FA_BWD_NT>(K + koff, st.k.s, V + voff, st.v.s,
                                  kb * KVB, Sk, tid, kst, vst);
  };
  auto write_chunks = [&]() {
    stage_write<D, KVB, FA_BWD_NT>(&Ks[0][0], &Vs[0][0], tid, kst, vst);
  };

  if (nkb > 0) load_chunks(0);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    write_chunks();
    __syncthreads();
    if (kb + 1 < nkb) load_chunks(kb + 1);

    // ---- S^T = K.Q^T, dP^T = V.dO^T: rows = key (registers), col = query
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = 0.f;
      dp[r] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      bf16x8 kf = row_frag<KROW>(&Ks[0][0], l31, hi5, c);
      bf16x8 vf = row_frag<KROW>(&Vs[0][0], l31, hi5, c);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qreg[c], s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, greg[c], dp, 0, 0, 0);
    }

    // ---- dS^T = P^T o (dP^T - delta); masked -> 0 ----
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int kvp = kb * KVB + c_row(r, hi5);
      bool dead = !q_ok || kvp >= Sk || (CAUSAL && kvp > my_q + causal_off);
      float p = dead ? 0.f : __expf(s[r] * scale - lse_q);
      dp[r] = p * (dp[r] - delta_q);
    }
    bf16x8 dsfrag[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
      dsfrag[c] = c8_to_bfrag((const float*)&dp + c * 8);

    // ---- dQ^T += K^T . dS^T (K^T via transposed reads of the K tile) ----
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        bf16x8 kt = tr_frag<KROW>(&Ks[0][0], l, hi5, c, dt);
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kt, dsfrag[c],
                                                          acc[dt], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: dQ[q][d] = scale * dQ^T[d][q] ----
  if (q_ok) {
    const long long dqo = b * st.dq.b + h * st.dq.h + (long long)my_q * st.dq.s;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = dt * 32 + c_row(r, hi5);
        dQ[dqo + d] = f2bf(acc[dt][r] * scale);
      }
  }
}

// q/k/v/o/dout and dq/dk/dv are logically [B,H,S,D] with d contiguous;
// strides[24] is the flat image of AttnBwdStrides (q k v o dout dq dk dv).
// lse and delta are fp32 [B,Hq,Sq] contiguous; delta is scratch that the preprocess kernel fills.  Returns 0
// once the three kernels are launched, non-zero (nothing launched) for an
// unsupported configuration: D must be 64 or 128, Hq a multiple of Hkv,
// Sq and Sk at least 1, and causal needs Sk >= Sq.
extern "C" int fa_bwd_strided_bf16(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, float* delta, void* dq, void* dk,
    void* dv, int B, int Hq, int Hkv, int Sq, int Sk, int D, float scale,
    int causal, const long long* strides, hipStream_t stream) {
  if (!attn_mfma32_supported(D, Hq, Hkv)) return 1;
  if (B < 1 || Sq < 1 || Sk < 1 || (causal && Sk < Sq)) return 1;
  const AttnBwdStrides st = attn_strides_from<AttnBwdStrides>(strides);
  const short* Qp = (const short*)q;
  const short* Kp = (const short*)k;
  const short* Vp = (const short*)v;
  const short* Op = (const short*)o;
  const short* Gp = (const short*)dout;
  short* dQp = (short*)dq;
  short* dKp = (short*)dk;
  short* dVp = (short*)dv;

  dim3 block(FA_BWD_NT);
  dim3 grid_kv((Sk + 127) / 128, Hkv, B);
  dim3 grid_q((Sq + 127) / 128, Hq, B);
#define FA_BWD_LAUNCH(DD, CC)                                                 \
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
    if (causal) FA_BWD_LAUNCH(64, true); else FA_BWD_LAUNCH(64, false);
  } else {
    if (causal) FA_BWD_LAUNCH(128, true); else FA_BWD_LAUNCH(128, false);
  }
#undef FA_BWD_LAUNCH
  return 0;
}
