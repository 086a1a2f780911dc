// Paged prefill attention: causal flash attention of a ragged batch of NEW
// query tokens against a paged KV cache that already holds those tokens' own
// K/V — the chunked-prefill and prefix-cache-suffix lanes of the Llama engine.
//
// The compute path is attention_fwd32.hip's: S^T = K · Q^T on the 32x32x16
// bf16 MFMA, lane-local online softmax with defer-max, P to B-fragments in
// registers (c8_to_bfrag), V^T by hardware transpose reads (tr_frag) of the
// same LDS image — all through the helpers of attention_mfma32.h.  What
// differs is where the operands come from:
//
//   q/o  [T, Hq, D] bf16, token-major; sequence b owns rows cu_q[b] ..
//        cu_q[b+1] (n_b of them).  seq_lens[b] = S_b is the cached length
//        INCLUDING the new tokens, so query i sits at position S_b - n_b + i
//        and sees kv <= that: the forward kernel's causal_off, per sequence.
//   K/V  cache [num_blocks, Hkv, block_size, D] (attention_decode.hip's
//        layout), bf16 or OCP e4m3; kv row r of sequence b lives in block
//        block_table[b][r / block_size].  e4m3 rows become bf16 while they
//        are staged (exact: every e4m3 value is a bf16 value), so the LDS
//        image and everything after it is the forward kernel's.
//
//   grid = (ceil(max_q_len / 128), Hq, B), block = 256 (4 waves x 32 queries)
#include "attention_mfma32.h"

#include <type_traits>

#define PP_NWAVES 4

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2p;

// 8 OCP e4m3 (two dwords) -> 8 bf16: the HW converter widens to f32, whose
// high half is the bf16 of the same value (3 mantissa bits, nothing dropped).
DEV_INLINE bf16x8 fp8x8_to_bf16x8(u32x2p w) {
  union {
    unsigned u[4];
    bf16x8 v;
  } r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], false);  // bytes 0,1
    f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[h], true);   // bytes 2,3
    r.u[2 * h] = (__float_as_uint(lo[0]) >> 16) |
                 (__float_as_uint(lo[1]) & 0xffff0000u);
    r.u[2 * h + 1] = (__float_as_uint(hi[0]) >> 16) |
                     (__float_as_uint(hi[1]) & 0xffff0000u);
  }
  return r.v;
}

// The waves-per-SIMD requests are the forward kernel's occupancies (3 at
// D=64, 2 at D=128).  Without the 2, the D=128 fp8 instance is allocated 258
// registers — two past the 2-wave edge — and runs at 1 wave/SIMD; with it
// every instance fits with no scratch.
template <int D, int KVB, bool FP8>
__global__ __launch_bounds__(PP_NWAVES * WAVE)
__attribute__((amdgpu_waves_per_eu(D == 64 ? 3 : 2)))
void paged_prefill_kernel(
    const short* __restrict__ Q,          // [T, Hq, D]
    const void* __restrict__ Kc,          // cache, layout above
    const void* __restrict__ Vc,
    const int* __restrict__ block_table,  // [B, max_blocks]
    const int* __restrict__ cu_q,         // [B + 1]
    const int* __restrict__ seq_lens,     // [B]
    short* __restrict__ O,                // [T, Hq, D]
    int Hq, int Hkv, int block_size, int max_blocks, float scale) {
  constexpr int KROW = D + FA_PPAD;
  constexpr int DCH = D / 16;  // QK^T k-chunks (K-dim 16)
  constexpr int DT = D / 32;   // PV d-tiles (M-dim 32)
  constexpr int QBLK = 32 * PP_NWAVES;
  constexpr int KF = KVB / 32;  // 32-kv score fragments per iteration
  constexpr int NT = PP_NWAVES * WAVE;
  constexpr int CPR = D / 8;               // 8-element chunks per kv row
  constexpr int NCH = KVB * CPR / NT;      // chunks per thread and tile

  const int b = blockIdx.z;
  const int q_lo = cu_q[b];
  const int n_q = cu_q[b + 1] - q_lo;
  const int tile0 = blockIdx.x * QBLK;
  // workgroup-uniform, before the first barrier: tiles past this sequence's
  // queries (every tile when n_q == 0) have nothing to do
  if (tile0 >= n_q) return;

  __shared__ alignas(16) short Ks[KVB][KROW];
  __shared__ alignas(16) short Vs[KVB][KROW];

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;  // 0 for lanes 0-31, 1 for 32-63

  const int h = blockIdx.y;
  const int hkv = h / (Hq / Hkv);
  const int S = seq_lens[b];
  const int causal_off = S - n_q;
  const int my_q = tile0 + w * 32 + l31;  // this lane's query of sequence b
  const int my_kv = my_q + causal_off;    // the last kv position it sees
  const bool q_ok = my_q < n_q;

  // Q^T B-fragments: qreg[c][j] = Q[my_q][c*16 + hi5*8 + j], in registers for
  // the whole kv sweep (as in the forward kernel)
  bf16x8 qreg[DCH];
  const long long qrow_off = ((long long)(q_lo + my_q) * Hq + h) * D;
#pragma unroll
  for (int c = 0; c < DCH; ++c) {
    qreg[c] = q_ok ? *(const bf16x8*)&Q[qrow_off + c * 16 + hi5 * 8]
                   : bf16x8_zero();
  }

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  // the sweep ends at the last kv position any live query of this tile sees
  const int last_kv = min(tile0 + QBLK, n_q) - 1 + causal_off;
  const int nkb = last_kv >= 0 ? last_kv / KVB + 1 : 0;

  // ---- paged staging: stage_load's sibling, rows found through the table.
  // Chunk i of this thread is kv row (i*NT + tid) / CPR of the tile; its
  // table slot and row-in-block advance by one tile per call, so the sweep
  // divides by block_size once, here.  Rows at kv >= S are zero and neither
  // the table nor the cache is read for them.  Offsets are 64-bit: a pool
  // of a few hundred GB passes 2^31 elements.
  typedef typename std::conditional<FP8, u32x2p, bf16x8>::type kv_t;
  const int* bt = block_table + (long long)b * max_blocks;
  int tb_slot[NCH], tb_row[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    int row = (i * NT + tid) / CPR;
    tb_slot[i] = row / block_size;
    tb_row[i] = row % block_size;
  }
  const int adv_slot = KVB / block_size, adv_row = KVB % block_size;
  int kv_base = 0;
  kv_t kraw[NCH], vraw[NCH];
  auto load_chunks = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      int ci = i * NT + tid;
      int row = ci / CPR, c8 = ci % CPR;
      kv_t kz = {}, vz = {};
      if (kv_base + row < S) {
        long long off =
            (((long long)bt[tb_slot[i]] * Hkv + hkv) * block_size +
             tb_row[i]) * D + c8 * 8;
        kz = *(const kv_t*)((const char*)Kc + off * (FP8 ? 1 : 2));
        vz = *(const kv_t*)((const char*)Vc + off * (FP8 ? 1 : 2));
      }
      kraw[i] = kz;
      vraw[i] = vz;
      tb_slot[i] += adv_slot;
      tb_row[i] += adv_row;
      if (tb_row[i] >= block_size) {
        tb_row[i] -= block_size;
        ++tb_slot[i];
      }
    }
    kv_base += KVB;
  };
  auto write_chunks = [&]() {
    if constexpr (FP8) {
      bf16x8 kreg[NCH], vreg[NCH];
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        kreg[i] = fp8x8_to_bf16x8(kraw[i]);
        vreg[i] = fp8x8_to_bf16x8(vraw[i]);
      }
      stage_write<D, KVB, NT>(&Ks[0][0], &Vs[0][0], tid, kreg, vreg);
    } else {
      stage_write<D, KVB, NT>(&Ks[0][0], &Vs[0][0], tid, kraw, vraw);
    }
  };

  if (nkb > 0) load_chunks();
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();
    write_chunks();
    __syncthreads();
    if (kb + 1 < nkb) load_chunks();

    // ---- S^T = K · Q^T (KF fragments of 32 kv each) ----
    f32x16 s[KF];
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[f][r] = 0.f;
#pragma unroll
    for (int f = 0; f < KF; ++f) {
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
        bf16x8 kfrag = row_frag<KROW>(&Ks[0][0], f * 32 + l31, hi5, c);
        __builtin_amdgcn_s_setprio(1);
        s[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag, qreg[c], s[f], 0,
                                                       0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }

    // ---- causal mask + lane-local online softmax (lane owns query my_q).
    // kv >= S is past every live query's my_kv, so the one test covers it.
    bool full = kb * KVB + KVB - 1 <= my_kv;
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int kvp = kb * KVB + f * 32 + c_row(r, hi5);
        bool dead = !full && kvp > my_kv;
        s[f][r] = dead ? -1e30f : s[f][r] * scale;
      }
    float smax = s[0][0];
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int r = 0; r < 16; ++r) smax = fmaxf(smax, s[f][r]);
    smax = fmaxf(smax, __shfl_xor(smax, 32, WAVE));  // partner combine
    // defer-max: keep the old running max while the block's growth <= 8
    if (kb == 0 || __ballot(smax > m_run + 8.f) != 0ull) {
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
    psum += __shfl_xor(psum, 32, WAVE);
    l_run = (kb == 0) ? psum : l_run + psum;

    // ---- P -> bf16 B-fragments in registers, one per 16-kv chunk ----
    bf16x8 pfrag[2 * KF];
#pragma unroll
    for (int c = 0; c < 2 * KF; ++c)
      pfrag[c] = c8_to_bfrag((const float*)&s[c >> 1] + (c & 1) * 8);

    // ---- O^T += V^T · P^T (V^T via hardware transpose reads) ----
#pragma unroll
    for (int c = 0; c < 2 * KF; ++c) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        bf16x8 vfrag = tr_frag<KROW>(&Vs[0][0], l, hi5, c, dt);
        __builtin_amdgcn_s_setprio(1);
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag, pfrag[c],
                                                          acc[dt], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
  }

  // ---- epilogue: O[q][d] = O^T[d][q] / l; a query at a negative position
  // (S < n_q, outside the contract) saw nothing and gets zeros ----
  if (q_ok) {
    float inv = (my_kv >= 0 && l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int d = dt * 32 + c_row(r, hi5);
        O[qrow_off + d] = f2bf(acc[dt][r] * inv);
      }
  }
}

// q/o [T,Hq,D] bf16 contiguous; kc/vc [num_blocks,Hkv,block_size,D] contiguous,
// bf16 or (kv_fp8) OCP e4m3; block_table int32 [B,max_blocks]; cu_q int32
// [B+1]; seq_lens int32 [B] — all device pointers, nothing is read back.
// Returns 0 once the kernel is launched, non-zero (nothing launched) for an
// unsupported configuration: D must be 64 or 128, Hq a multiple of Hkv,
// block_size and max_q_len at least 1, Hq and B within the grid limits.
//
// Preconditions the host cannot check without a device read-back:
//   seq_lens[b] >= cu_q[b+1] - cu_q[b]   (the new tokens are in the cache)
//   block_table[b][i] is a valid block for every i <= (seq_lens[b]-1)/block_size
//   max_q_len >= max_b (cu_q[b+1] - cu_q[b])   (larger only launches idle tiles)
// Neither the table nor the cache is read for kv >= seq_lens[b].
extern "C" int paged_prefill_bf16(const void* q, const void* kc, const void* vc,
                                  const int* block_table, const int* cu_q,
                                  const int* seq_lens, void* o, int B, int Hq,
                                  int Hkv, int D, int block_size,
                                  int max_blocks, int max_q_len, float scale,
                                  int kv_fp8, hipStream_t stream) {
  if (!attn_mfma32_supported(D, Hq, Hkv)) return 1;
  if (block_size < 1 || max_q_len < 1 || B < 1 || B > 65535 || Hq > 65535)
    return 1;
  dim3 grid((max_q_len + 127) / 128, Hq, B);
  dim3 block(PP_NWAVES * WAVE);
  // KVB per head dim as the forward kernel chose it (64 at D=64, 32 at D=128)
#define PPLAUNCH(DD, KK, F8)                                                  \
  hipLaunchKernelGGL((paged_prefill_kernel<DD, KK, F8>), grid, block, 0,      \
                     stream, (const short*)q, kc, vc, block_table, cu_q,      \
                     seq_lens, (short*)o, Hq, Hkv, block_size, max_blocks,    \
                     scale)
  if (D == 64) {
    if (kv_fp8) PPLAUNCH(64, 64, true); else PPLAUNCH(64, 64, false);
  } else {
    if (kv_fp8) PPLAUNCH(128, 32, true); else PPLAUNCH(128, 32, false);
  }
#undef PPLAUNCH
  return 0;
}
