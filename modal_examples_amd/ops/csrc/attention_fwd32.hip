// Flash-attention forward v8 — 32x32x16 MFMA with LANE-LOCAL online softmax,
// per-head-dim KV block size and defer-max rescale skipping.  The single
// forward attention kernel: every model reaches it through bindings.cpp.
//
// The retired 16x16 kernels (v3-v6) were softmax-LATENCY-bound: ablation
// measured the 16-lane-group shuffle/exp chains at ~56% of kernel time.  This
// structure eliminates cross-lane reductions almost entirely (the m214-style
// swapped-operand recipe, re-derived for gfx950):
//
//   QK^T is computed TRANSPOSED with mfma_f32_32x32x16_bf16:
//     S^T = K · Q^T  →  each lane holds 16 of the 32 kv-scores for ONE query
//     (C layout col = q = lane&31); row-softmax becomes 15 in-register ops +
//     ONE exchange with the partner lane (lane_pair, no LDS).  Rescale
//     factors are lane-local (no broadcast).
//   P converts to bf16 B-fragments IN REGISTERS (c8_to_bfrag) — P never
//     touches LDS.
//   PV: O^T = V^T · P^T, V^T fragments by hardware transpose reads (tr_frag)
//     of the same LDS image the K row reads (row_frag) use.
//
// Fragment layouts, the LDS tile image and the measured lane semantics of
// those helpers: attention_mfma32.h, shared with attention_bwd.hip.
#include "attention_mfma32.h"

#include <cstdlib>

#define FA32_NWAVES 4

// KVB: kv rows per block iteration.  64 halves the barrier/softmax rounds
// per token vs the r1 kernel's 32 (the m214-ladder "KVBLK=64" lever).
// DEFER: defer-max rescale skipping (HK THR=8) — keep the old running max
// while per-block growth <= 8, so P = exp(s - m_old) <= e^8 (f32 acc safe)
// and the O-wide rescale is skipped entirely.
// Every instance asks for its occupancy floor (3 waves/SIMD at D=64, 2 at
// D=128).  Without the request the compiler budgets 512 registers, parks the
// accumulators in AGPRs and copies O out and back on every tile (64
// v_accvgpr moves per tile at D=64); with it every MFMA takes its VGPR form.
template <int D, bool CAUSAL, int KVB, bool DEFER>
__global__ __launch_bounds__(FA32_NWAVES * WAVE)
__attribute__((amdgpu_waves_per_eu(D == 64 ? 3 : 2)))
void fa32_kernel(
    const short* __restrict__ Q, const short* __restrict__ K,
    const short* __restrict__ V, short* __restrict__ O,
    float* __restrict__ LSE, int B, int Hq, int Hkv, int Sq, int Sk,
    float scale, AttnFwdStrides st) {
  constexpr int KROW = D + FA_PPAD;
  constexpr int DCH = D / 16;  // QK^T k-chunks (K-dim 16)
  constexpr int DT = D / 32;   // PV d-tiles (M-dim 32)
  constexpr int QBLK = 32 * FA32_NWAVES;
  constexpr int KF = KVB / 32;  // 32-kv score fragments per iteration

  __shared__ alignas(16) short Ks[KVB][KROW];
  __shared__ alignas(16) short Vs[KVB][KROW];

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;  // 0 for lanes 0-31, 1 for 32-63

  const int qblk = blockIdx.x;
  const int h = blockIdx.y;
  const int b = blockIdx.z;
  const int hkv = h / (Hq / Hkv);

  const long long qoff = b * st.q.b + h * st.q.h;
  const long long koff = b * st.k.b + hkv * st.k.h;
  const long long voff = b * st.v.b + hkv * st.v.h;
  const long long ooff = b * st.o.b + h * st.o.h;
  const int q0 = qblk * QBLK + w * 32;
  const int my_q = q0 + l31;  // this lane's query row
  const int q0w = __builtin_amdgcn_readfirstlane(q0);  // q0, known uniform
  const int causal_off = Sk - Sq;

  // Q^T B-fragments: qreg[c][j] = Q[my_q][c*16 + hi5*8 + j], held in
  // registers for all D — measured: reloading Q from L2 per KV block instead
  // regressed D=128 by 22-30% (occupancy stayed at 2 waves/SIMD).
  bf16x8 qreg[DCH];
  const long long qrow_off = qoff + (long long)my_q * st.q.s;
  const bool q_ok = my_q < Sq;
#pragma unroll
  for (int c = 0; c < DCH; ++c) {
    qreg[c] = q_ok
        ? *(const bf16x8*)&Q[qrow_off + c * 16 + hi5 * 8]
        : bf16x8_zero();
  }

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  int nkb = (Sk + KVB - 1) / KVB;
  if (CAUSAL) {
    int max_kv = qblk * QBLK + QBLK - 1 + causal_off;
    int lim = (max_kv + KVB) / KVB;
    if (lim < nkb) nkb = lim;
  }

  // async register staging: next block loads issue before this block computes
  constexpr int NT = FA32_NWAVES * WAVE;
  bf16x8 kreg[KVB * (D / 8) / NT], vreg[KVB * (D / 8) / NT];
  auto load_chunks = [&](int kb) {
    stage_load<D, KVB, NT>(K + koff, st.k.s, V + voff, st.v.s, kb * KVB, Sk,
                           tid, kreg, vreg);
  };
  auto write_chunks = [&]() {
    stage_write<D, KVB, NT>(&Ks[0][0], &Vs[0][0], tid, kreg, vreg);
  };

  load_chunks(0);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    write_chunks();
    __syncthreads();
    if (kb + 1 < nkb) load_chunks(kb + 1);

    // ---- S^T = K · Q^T (KF fragments of 32 kv each) ----
    f32x16 s[KF];
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[f][r] = 0.f;
    // Reads run ahead of the MFMAs: all DCH row reads of a 32-key fragment
    // go out together into registers of their own, and while its MFMAs run
    // the next fragment's reads (after the last one, the first V^T reads,
    // whose tile has been in LDS since the barrier) are already in flight.
    // LDS returns in order, so each MFMA waits on a counted lgkmcnt.  The
    // scheduling fences keep that issue order; one priority pair per cluster.
    // A = K[kv][d]: lane holds K[f*32 + l31][c*16 + hi5*8 + j]
    bf16x8 kf[KF][DCH];
    bf16x8 vf[2][DT];
#pragma unroll
    for (int c = 0; c < DCH; ++c)
      kf[0][c] = row_frag<KROW>(&Ks[0][0], l31, hi5, c);
#pragma unroll
    for (int f = 0; f < KF; ++f) {
      if (f + 1 < KF) {
#pragma unroll
        for (int c = 0; c < DCH; ++c)
          kf[f + 1][c] = row_frag<KROW>(&Ks[0][0], (f + 1) * 32 + l31, hi5, c);
      } else {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          vf[0][dt] = tr_frag<KROW>(&Vs[0][0], l, hi5, 0, dt);
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int c = 0; c < DCH; ++c)
        s[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[f][c], qreg[c], s[f],
                                                       0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- mask + lane-local online softmax (this lane owns query my_q) ----
    // A tile is interior when every key of it exists and, under the causal
    // mask, is visible to the wave's FIRST row (so to all 32).  The test is
    // wave-uniform: interior tiles branch past the per-score compares and
    // selects.  An edge tile masks per element; a lane whose own row sees the
    // whole tile gets the same s * scale there.
    const bool full = (kb * KVB + KVB <= Sk) &&
                      (!CAUSAL || kb * KVB + KVB - 1 <= q0w + causal_off);
    if (full) {
#pragma unroll
      for (int f = 0; f < KF; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[f][r] *= scale;
    } else {
#pragma unroll
      for (int f = 0; f < KF; ++f)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int kvp = kb * KVB + f * 32 + c_row(r, hi5);
          bool dead = (kvp >= Sk) || (CAUSAL && kvp > my_q + causal_off);
          s[f][r] = dead ? -1e30f : s[f][r] * scale;
        }
    }
    float smax = s[0][0];
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) smax = fmaxf(smax, s[f][r]);
    float pa, pb;
    lane_pair(smax, pa, pb);  // partner combine, in registers
    smax = fmaxf(pa, pb);
    if (!DEFER || kb == 0 ||
        __ballot(smax > m_run + 8.f) != 0ull) {
      float m_new = fmaxf(m_run, smax);
      float rs = __expf(m_run - m_new);
      if (kb > 0 && __ballot(rs < 0.999999f) != 0ull) {
        l_run *= rs;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[dt][r] *= rs;
      }
      m_run = m_new;
    }
    float psum = 0.f;
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[f][r] = __expf(s[f][r] - m_run);
        psum += s[f][r];
      }
    lane_pair(psum, pa, pb);
    psum = pa + pb;
    l_run = (kb == 0) ? psum : l_run + psum;

    // ---- P → bf16 B-fragments in registers, one per 16-kv chunk ----
    bf16x8 pfrag[2 * KF];
#pragma unroll
    for (int c = 0; c < 2 * KF; ++c)
      pfrag[c] = c8_to_bfrag((const float*)&s[c >> 1] + (c & 1) * 8);

    // ---- O^T += V^T · P^T (V^T via hardware transpose reads) ----
    // chunk c + 1 is read while chunk c multiplies; chunk 0 came in above
#pragma unroll
    for (int c = 0; c < 2 * KF; ++c) {
      if (c + 1 < 2 * KF) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
          vf[(c + 1) & 1][dt] = tr_frag<KROW>(&Vs[0][0], l, hi5, c + 1, dt);
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            vf[c & 1][dt], pfrag[c], acc[dt], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l ----
  if (my_q < Sq) {
    // A causal row before the first key (Sq > Sk) sees nothing: o = 0 and
    // lse = -inf.  In a q block that still has live rows the loop ran with
    // every score of such a row at -1e30, which leaves the mean of a KV
    // block in acc, so the row is overridden here, not in the loop.
    const bool hidden = CAUSAL && my_q + causal_off < 0;
    // log-sum-exp of the scaled scores for the backward: l_run is always
    // sum exp(s - m_run), with defer-max on or off.  Both lane halves hold
    // the same pair; the low half writes.
    if (LSE != nullptr && hi5 == 0)
      LSE[((long long)b * Hq + h) * Sq + my_q] =
          hidden ? -INFINITY : m_run + logf(l_run);
    float inv = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = dt * 32 + c_row(r, hi5);
        O[ooff + (long long)my_q * st.o.s + d] =
            f2bf(hidden ? 0.f : acc[dt][r] * inv);
      }
  }
}

// q/k/v/o are logically [B,H,S,D] with d contiguous; strides[12] is the flat
// image of AttnFwdStrides (q k v o).  Returns 0 once the
// kernel is launched, non-zero (nothing launched) for an unsupported
// configuration: D must be 64 or 128 and Hq a multiple of Hkv.  lse, when
// not null, receives the fp32 log-sum-exp per query row, [B,Hq,Sq] contiguous.
extern "C" int fa32_fwd_strided_bf16(
    const void* q, const void* k, const void* v, void* o, float* lse, int B,
    int Hq, int Hkv, int Sq, int Sk, int D, float scale, int causal,
    const long long* strides, hipStream_t stream) {
  if (!attn_mfma32_supported(D, Hq, Hkv)) return 1;
  const short* Qp = (const short*)q;
  const short* Kp = (const short*)k;
  const short* Vp = (const short*)v;
  short* Op = (short*)o;
  const AttnFwdStrides st = attn_strides_from<AttnFwdStrides>(strides);
  dim3 grid((Sq + 127) / 128, Hq, B);
  dim3 block(FA32_NWAVES * WAVE);
  // KVB is chosen per head-dim (A/B-measured, profiles/attn_ab_r2.txt):
  //   D=64:  KVB=64 wins (447 vs 407 TF — fewer barrier/softmax rounds)
  //   D=128: KVB=64 LOST 40% (causal instantiation lands at 1 wave/SIMD —
  //          the r1 double-buffer failure mode); only KVB=32 is built.
  // MODAL_AMD_FA_NODEFER disables defer-max rescale skipping (+5-10% A/B).
  static const bool defer_env = getenv("MODAL_AMD_FA_NODEFER") == nullptr;
#define L32K(DD, CC, KK)                                                      \
  do {                                                                        \
    if (defer_env)                                                            \
      hipLaunchKernelGGL((fa32_kernel<DD, CC, KK, true>), grid, block, 0,     \
                         stream, Qp, Kp, Vp, Op, lse, B, Hq, Hkv, Sq, Sk,     \
                         scale, st);                                          \
    else                                                                      \
      hipLaunchKernelGGL((fa32_kernel<DD, CC, KK, false>), grid, block, 0,    \
                         stream, Qp, Kp, Vp, Op, lse, B, Hq, Hkv, Sq, Sk,     \
                         scale, st);                                          \
  } while (0)
  if (D == 64) {
    if (causal) L32K(64, true, 64); else L32K(64, false, 64);
  } else {
    if (causal) L32K(128, true, 32); else L32K(128, false, 32);
  }
#undef L32K
  return 0;
}
