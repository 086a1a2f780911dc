// Packed multi-token paged decode: the verify step of speculative decoding.
//
// A sequence brings T new tokens (its last sampled token and T-1 drafts), a
// kv-head group has G = Hq/Hkv query heads, and T*G <= 32: all of them fit
// the N dimension of ONE 32x32x16 MFMA tile ("pack GQA").  One sweep of the
// sequence's KV cache per (sequence, kv head) therefore serves every draft
// position and every head of the group on the matrix pipe, where T rows of
// paged_decode stream the cache T times through the vector ALU.
//
// Semantics are paged_prefill's (attention_prefill_paged.hip), for short runs:
//   q/o  [R, Hq, D] bf16, token-major; sequence b owns rows cu_q[b] ..
//        cu_q[b+1] (n_b <= 32/G of them).  seq_lens[b] = S_b INCLUDES the new
//        tokens: query t sits at position S_b - n_b + t and sees kv <= that;
//        a query at a negative position gets zeros.
//   K/V  cache [num_blocks, Hkv, block_size, D], bf16 or OCP e4m3, kv row r of
//        sequence b in block block_table[b][r / block_size].
//
//   grid = (Hkv, B, splits), block = 256 (4 waves)
//
// Tile.  Packed column t*G + g is query t of the sequence, head hkv*G + g.
// Columns at t >= n_b are dead: they load zeros, are never merged and never
// stored.  The math is the swapped-operand recipe of attention_mfma32.h:
// S^T = K · Q^T puts the 32 kv rows of a tile on M and the packed queries on
// N, so a lane (with its partner lane^32) owns one query column and the
// online softmax is lane-local; P becomes B-fragments in registers
// (c8_to_bfrag) and O^T += V^T · P reads V^T with the hardware transpose
// (tr_frag).
//
// Sweep.  The split's 32-row kv tiles go round-robin to the four waves (wave
// w takes tiles w, w+4, ...); each wave keeps its own (m, l, acc) and stages
// its K/V tile in a wave-private LDS region, so the sweep has no workgroup
// barrier — only wave-scope fences around the LDS image.  Global loads are
// whole rows (D/8 lanes x 16 B), issued for the wave's next tile before the
// math of the current one, into fully unrolled (named) registers.  fp8 rows
// widen to bf16 on the way into LDS (exact).  Block-table slots are found per
// kv row and advanced by one round (128 rows) per load, so block_size may be
// anything >= 1; rows at kv >= S_b are zero and neither table nor cache is
// read for them.
//
// Rows never see each other.  Every softmax decision is lane-local: masked
// scores take p = 0 exactly (not exp of a sentinel), the running max is
// updated on every tile, and the one wave-uniform shortcut — skip the
// accumulator rescale when every lane's factor is exactly 1.0f — multiplies
// by 1.0f when it does not skip, so a row's bits cannot depend on what else
// is in the tile.  Tiles that end at or before S_b - n_b skip the mask test.
//
// Epilogue.  After one barrier the staging LDS becomes the merge buffer: the
// four waves' partials are realigned to their common max, then either
// normalised and stored (splits == 1) or written unnormalised with (m, l) to
// the fp32 workspace [R, Hq, splits, D+2] — paged_decode's layout, finished
// by its merge kernel (decode_merge_bf16 in attention_decode.hip).  No
// atomics anywhere: results are bitwise reproducible.
#include "attention_mfma32.h"

#include <type_traits>

#define DP_NWAVES 4
#define DP_MAX_G 8
#define DP_MAX_SPLITS 64

extern "C" void decode_merge_bf16(const float* ws, void* o, long long rows,
                                  int Hq, int D, int splits,
                                  hipStream_t stream);

// Orders this wave's LDS writes against its own later reads (and reads
// against later writes) of the wave-private staging region.
DEV_INLINE void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Built without the packed fp32 VALU forms (v_pk_mul_f32 and its kin), as the
// project's newer kernels are (w4_mma.h).  Here that is a per-source compiler
// flag (_build.py, EXTRA_FLAGS) and not w4_mma.h's function attribute: the
// attribute makes the kernel's target differ from that of the shared
// attention_mfma32.h helpers, which then are not inlined and the register
// arrays go to scratch (336 to 528 bytes per lane, measured).  The only
// candidates are the accumulator rescale and the softmax sums, a few dozen
// multiplies per tile beside 16 MFMAs; registers, occupancy and LDS come out
// the same with and without the flag.
//
// Two waves per SIMD (two workgroups per CU) at both head dims: the second
// workgroup's loads cover the first one's MFMA phases, and 2 x 68 KB of
// staging fits the CU's LDS at D = 128.
template <int D, bool FP8>
__global__ __launch_bounds__(DP_NWAVES * WAVE)
__attribute__((amdgpu_waves_per_eu(2)))
void paged_decode_packed_kernel(
    const short* __restrict__ Q,          // [R, Hq, D]
    const void* __restrict__ Kc,          // cache, layout above
    const void* __restrict__ Vc,
    const int* __restrict__ block_table,  // [B, max_blocks]
    const int* __restrict__ cu_q,         // [B + 1]
    const int* __restrict__ seq_lens,     // [B]
    short* __restrict__ O,                // [R, Hq, D]
    float* __restrict__ WS,               // [R, Hq, splits, D+2] or nullptr
    int Hq, int Hkv, int block_size, int max_blocks, int splits, float scale) {
  constexpr int KROW = D + FA_PPAD;
  constexpr int DCH = D / 16;  // QK^T k-chunks (K-dim 16)
  constexpr int DT = D / 32;   // PV d-tiles (M-dim 32)
  constexpr int CPR = D / 8;              // 16 B chunks per kv row
  constexpr int RPI = WAVE / CPR;         // kv rows per load instruction
  constexpr int NCH = 32 / RPI;           // chunks per lane and tile
  constexpr int TILE_E = 32 * KROW;       // bf16 elements of one staged tile
  constexpr int STAGE_B = DP_NWAVES * 2 * TILE_E * 2;
  constexpr int MERGE_B = DP_NWAVES * (D + 2) * 32 * 4;
  static_assert(MERGE_B <= STAGE_B, "the merge buffer reuses the staging LDS");
  constexpr int ROUND = 32 * DP_NWAVES;   // kv rows between a wave's tiles

  const int hkv = blockIdx.x;
  const int b = blockIdx.y;
  const int split = blockIdx.z;
  const int G = Hq / Hkv;
  const int q_lo = cu_q[b];
  // a run longer than the tile holds is outside the contract; clamping keeps
  // every access inside this sequence's rows
  const int n_q = min(cu_q[b + 1] - q_lo, 32 / G);
  // workgroup-uniform, before the first barrier
  if (n_q <= 0) return;

  __shared__ alignas(16) char smem[STAGE_B];

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;
  short* Ks = (short*)smem + w * 2 * TILE_E;
  short* Vs = Ks + TILE_E;

  const int S = seq_lens[b];
  const int causal_off = S - n_q;
  // this lane's packed column: query my_t of the run, head hkv*G + my_g
  const int my_t = l31 / G, my_g = l31 - my_t * G;
  const bool q_ok = my_t < n_q;
  const int my_kv = q_ok ? my_t + causal_off : -1;  // last kv position seen

  bf16x8 qreg[DCH];
  {
    const long long qoff = ((long long)(q_lo + my_t) * Hq + hkv * G + my_g) * D;
#pragma unroll
    for (int c = 0; c < DCH; ++c)
      qreg[c] = q_ok ? *(const bf16x8*)&Q[qoff + c * 16 + hi5 * 8]
                     : bf16x8_zero();
  }

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  // this split's tiles: [t_lo, t_hi), boundaries on the 32-row tile
  const int ntile = S > 0 ? (S + 31) / 32 : 0;
  const int per = (ntile + splits - 1) / splits;
  const int t_lo = split * per;
  const int t_hi = min(ntile, t_lo + per);

  // ---- paged staging.  Chunk i of this lane is kv row i*RPI + l/CPR of the
  // tile, 16 B chunk l%CPR of that row.  The table slot and row-in-block of
  // chunk 0 are divided out once, here, and advance by one round per load;
  // the other chunks step RPI rows on from it (one wrap at most unless
  // block_size < RPI), which keeps the cursor in two registers.
  typedef typename std::conditional<FP8, u32x2p, bf16x8>::type kv_t;
  const int* bt = block_table + (long long)b * max_blocks;
  const int c8 = l % CPR, r0 = l / CPR;
  int kv_next = (t_lo + w) * 32 + r0;  // kv position of this lane's chunk 0
  int tb_slot = kv_next / block_size;
  int tb_row = kv_next - tb_slot * block_size;
  const int adv_slot = ROUND / block_size;
  const int adv_row = ROUND - adv_slot * block_size;
  kv_t kraw[NCH], vraw[NCH];
  auto load_chunks = [&]() {
    int slot = tb_slot, row = tb_row;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      kv_t kz = {}, vz = {};
      if (kv_next + i * RPI < S) {
        long long off =
            (((long long)bt[slot] * Hkv + hkv) * block_size + row) * D +
            c8 * 8;
        kz = *(const kv_t*)((const char*)Kc + off * (FP8 ? 1 : 2));
        vz = *(const kv_t*)((const char*)Vc + off * (FP8 ? 1 : 2));
      }
      kraw[i] = kz;
      vraw[i] = vz;
      row += RPI;
      while (row >= block_size) {
        row -= block_size;
        ++slot;
      }
    }
    tb_slot += adv_slot;
    tb_row += adv_row;
    if (tb_row >= block_size) {
      tb_row -= block_size;
      ++tb_slot;
    }
    kv_next += ROUND;
  };
  auto write_chunks = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if constexpr (FP8) {
        row_store<KROW>(Ks, i * RPI + r0, c8, fp8x8_to_bf16x8(kraw[i]));
        row_store<KROW>(Vs, i * RPI + r0, c8, fp8x8_to_bf16x8(vraw[i]));
      } else {
        row_store<KROW>(Ks, i * RPI + r0, c8, kraw[i]);
        row_store<KROW>(Vs, i * RPI + r0, c8, vraw[i]);
      }
    }
  };

  int tile = t_lo + w;
  if (tile < t_hi) load_chunks();
  for (; tile < t_hi; tile += DP_NWAVES) {
    wave_lds_sync();  // the previous tile's reads are done
    write_chunks();
    wave_lds_sync();
    if (tile + DP_NWAVES < t_hi) load_chunks();

    // ---- S^T = K · Q^T ----
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      bf16x8 kfrag = row_frag<KROW>(Ks, l31, hi5, c);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag, qreg[c], s, 0, 0, 0);
    }

    // ---- causal mask: only tiles that reach past the run's first query.
    // kv >= S is past every live query's my_kv, so the one test covers it.
    unsigned dead = 0;
    if (tile * 32 + 31 > causal_off) {  // wave-uniform
#pragma unroll
      for (int r = 0; r < 16; ++r)
        dead |= (tile * 32 + c_row(r, hi5) > my_kv ? 1u : 0u) << r;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
      s[r] = (dead >> r) & 1 ? -1e30f : s[r] * scale;

    // ---- lane-local online softmax (the lane pair owns one query) ----
    float smax = s[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) smax = fmaxf(smax, s[r]);
    smax = fmaxf(smax, __shfl_xor(smax, 32, WAVE));
    const float m_new = fmaxf(m_run, smax);
    const float rs = __expf(m_run - m_new);
    m_run = m_new;
    // x * 1.0f == x: skipping when no lane rescales changes no row's bits
    if (__ballot(rs != 1.f) != 0ull) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] *= rs;
    }
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = (dead >> r) & 1 ? 0.f : __expf(s[r] - m_new);
      psum += s[r];
    }
    psum += __shfl_xor(psum, 32, WAVE);
    l_run = l_run * rs + psum;

    // ---- P -> bf16 B-fragments, O^T += V^T · P ----
    bf16x8 pfrag[2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
      pfrag[c] = c8_to_bfrag((const float*)&s + c * 8);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        bf16x8 vfrag = tr_frag<KROW>(Vs, l, hi5, c, dt);
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag, pfrag[c],
                                                          acc[dt], 0, 0, 0);
      }
    }
  }

  // ---- merge the four waves through LDS (max realignment) ----
  float* sacc = (float*)smem;                // [wave][d][column]
  float* sml = sacc + DP_NWAVES * D * 32;    // [wave][m, l][column]
  __syncthreads();  // every wave is done with its staging region
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      sacc[(w * D + dt * 32 + c_row(r, hi5)) * 32 + l31] = acc[dt][r];
  if (hi5 == 0) {
    sml[(w * 2) * 32 + l31] = m_run;
    sml[(w * 2 + 1) * 32 + l31] = l_run;
  }
  __syncthreads();

  // thread = (column, group of D/8 consecutive d)
  constexpr int DPT = D / 8;
  const int col = tid & 31, dg = tid >> 5;
  const int t = col / G, g = col - t * G;
  if (t >= n_q) return;
  float m_star = -1e30f;
#pragma unroll
  for (int u = 0; u < DP_NWAVES; ++u)
    m_star = fmaxf(m_star, sml[(u * 2) * 32 + col]);
  float f[DP_NWAVES], den = 0.f;
#pragma unroll
  for (int u = 0; u < DP_NWAVES; ++u) {
    f[u] = __expf(sml[(u * 2) * 32 + col] - m_star);
    den += f[u] * sml[(u * 2 + 1) * 32 + col];
  }
  float num[DPT];
#pragma unroll
  for (int j = 0; j < DPT; ++j) {
    float a = 0.f;
#pragma unroll
    for (int u = 0; u < DP_NWAVES; ++u)
      a += f[u] * sacc[(u * D + dg * DPT + j) * 32 + col];
    num[j] = a;
  }
  const long long orow = (long long)(q_lo + t) * Hq + hkv * G + g;
  if (WS == nullptr) {
    // a query at a negative position saw nothing: den == 0, zeros
    const float inv = den > 0.f ? 1.f / den : 0.f;
#pragma unroll
    for (int j0 = 0; j0 < DPT; j0 += 8) {
      bf16x8 o8;
#pragma unroll
      for (int j = 0; j < 8; ++j) o8[j] = f2bf(num[j0 + j] * inv);
      *(bf16x8*)&O[orow * D + dg * DPT + j0] = o8;
    }
  } else {
    float* ws = WS + (orow * splits + split) * (D + 2);
#pragma unroll
    for (int j = 0; j < DPT; ++j) ws[dg * DPT + j] = num[j];
    if (dg == 0) {
      ws[D] = m_star;  // the partial is unnormalised, at this max
      ws[D + 1] = den;
    }
  }
}

// The flash-decoding split count, a function of shapes only (so the op
// captures into a graph): fill the chip when B*Hkv is small, keep every
// split at least two rounds (256 kv rows) of the longest representable
// sequence.  forced > 0 takes that count instead (tests and benchmarks).
// Returns 0 for a count the kernel does not take.
extern "C" int paged_decode_packed_splits(long long B, int Hkv,
                                          long long s_bound, int forced) {
  if (forced < 0 || forced > DP_MAX_SPLITS) return 0;
  if (forced > 0) return forced;
  int splits = 1;
  while (B * Hkv * splits < 512 && (long long)splits * 256 < s_bound &&
         splits < DP_MAX_SPLITS)
    splits *= 2;
  return splits;
}

// q/o [R,Hq,D] bf16 contiguous; kc/vc [num_blocks,Hkv,block_size,D]
// contiguous, bf16 or (kv_fp8) OCP e4m3; block_table int32 [B,max_blocks];
// cu_q int32 [B+1]; seq_lens int32 [B]; ws fp32 [R,Hq,splits,D+2] when
// splits > 1 — all device pointers, nothing is read back.  Returns 0 once
// the kernels are launched, non-zero (nothing launched) for an unsupported
// configuration: D must be 64 or 128, Hq a multiple of Hkv with Hq/Hkv <= 8,
// max_q_len * (Hq/Hkv) <= 32, block_size >= 1, splits in 1..64.
//
// Preconditions the host cannot check without a device read-back:
//   cu_q[b+1] - cu_q[b] <= max_q_len, and cu_q[B] == R when splits > 1
//   seq_lens[b] >= cu_q[b+1] - cu_q[b]   (the new tokens are in the cache)
//   block_table[b][i] is a valid block for every i <= (seq_lens[b]-1)/block_size
// Neither the table nor the cache is read for kv >= seq_lens[b].
extern "C" int paged_decode_packed_bf16(
    const void* q, const void* kc, const void* vc, const int* block_table,
    const int* cu_q, const int* seq_lens, void* o, float* ws, long long R,
    int B, int Hq, int Hkv, int D, int block_size, int max_blocks,
    int max_q_len, int splits, float scale, int kv_fp8, hipStream_t stream) {
  if (!attn_mfma32_supported(D, Hq, Hkv)) return 1;
  const int G = Hq / Hkv;
  if (G > DP_MAX_G || max_q_len < 1 || max_q_len * G > 32) return 1;
  if (block_size < 1 || max_blocks < 1 || R < 1 || B < 1 || B > 65535)
    return 1;
  if (splits < 1 || splits > DP_MAX_SPLITS || (splits > 1 && ws == nullptr))
    return 1;
  dim3 grid(Hkv, B, splits);
  dim3 block(DP_NWAVES * WAVE);
  float* ws_arg = splits > 1 ? ws : nullptr;
#define DPLAUNCH(DD, F8)                                                      \
  hipLaunchKernelGGL((paged_decode_packed_kernel<DD, F8>), grid, block, 0,    \
                     stream, (const short*)q, kc, vc, block_table, cu_q,      \
                     seq_lens, (short*)o, ws_arg, Hq, Hkv, block_size,        \
                     max_blocks, splits, scale)
  if (D == 64) {
    if (kv_fp8) DPLAUNCH(64, true); else DPLAUNCH(64, false);
  } else {
    if (kv_fp8) DPLAUNCH(128, true); else DPLAUNCH(128, false);
  }
#undef DPLAUNCH
  if (splits > 1) decode_merge_bf16(ws, o, R, Hq, D, splits, stream);
  return 0;
}
