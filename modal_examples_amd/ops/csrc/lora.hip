// Multi-LoRA delta for one projection, bf16, gfx950: every row of a batch may
// belong to a different adapter, chosen by an index only the device knows.
//
//   y[n, :] <- bf16( float(y[n, :]) + sum_r t[n, r] * B[s][:, r] )
//   t[n, r]  = sum_k x[n, k] * A[s][r, k],    s = idx[n]
//
// x [N,K], y [N,O] (in place), banks A [S,R,K] and B [S,O,R] with the
// adapter's alpha/r folded into B.  Rows with idx outside [0,S) are not
// touched, not even rewritten.  Nothing on the host depends on idx — every
// grid and workspace size is a function of (N, S, R, K, O) only — so the op is
// sync-free and captures into a hipGraph.
//
//   align    idx -> per-adapter segments of rows, each padded to the 32-row
//            M-tile so a tile belongs to one adapter: slot_map [tiles*32]
//            (row id, -1 = pad), tile_adapter, num_tiles <= N/32 + S.  The
//            schedule of moe.hip's align with top_k = 1; it is built once per
//            model forward and serves every projection of every layer.
//   shrink   t = x . A[s]^T, a skinny GEMM (R <= 64 columns, long K).  One
//            wave per (M-tile, K-slice): the parallelism comes from split-K.
//            Each slice writes its fp32 partial to its own plane of the
//            workspace T [slices, tiles*32, R]; no float atomics.
//   expand   y += t . B[s]^T, a fat GEMM with K = R.  One wave per (M-tile,
//            128 output columns).  It sums the slice planes of its tile of t
//            in ascending slice order in fp32 and feeds t to the MFMA as two
//            bf16 operands, hi = bf16(t) and lo = bf16(t - hi), so the
//            intermediate is never rounded to bf16; the kernel is bound by
//            reading B and the read-modify-write of y, so the second MFMA per
//            k-step hides behind them.
//
// Both GEMMs have both operands contiguous along their k, so the 32x32x16
// fragments (layouts: attention_mfma32.h) are plain 16 B loads straight to
// registers.  The slice count depends on K alone and each slice sums its k
// in one fixed order, so a row's result never depends on the batch around
// it: results are bitwise reproducible and a row computed alone equals its
// row in any batch.  (The integer atomics of align only decide which slot of
// its adapter's segment a row takes.)
//
// The expand product is computed TRANSPOSED (B[s] tile as the A operand, t
// as the B operand): a lane then holds ONE row of y and runs of four
// consecutive output columns, so the epilogue is 8 B vector loads and stores
// addressed by the lane's own slot_map entry.  The untransposed form (a lane
// holds one column of 16 rows: 2 B accesses, a slot_map read per register)
// is kept behind `swap = 0` for the benchmark; profiles/lora.txt has both.
#include "attention_mfma32.h"

#define LORA_BM 32          // rows per M-tile = one 32x32 MFMA tile
#define LORA_MAX_S 32
#define LORA_ALIGN_NT 256
#define LORA_NF 4           // 16-wide k-steps per chunk of the shrink loop
#define LORA_KC (LORA_NF * 16)
#define LORA_SLICE_K 512    // shortest K-slice the rule cuts
#define LORA_MAX_SLICES 16
#define LORA_CB 128         // output columns per expand wave (four N-tiles)

// ---------------------------------------------------------------- align
// One block.  max_tiles = N/32 + S bounds the tiles in use (sum of
// ceil(c_s/32) <= floor(N/32) + S), so every index written here stays inside
// slot_map [max_tiles*32] and tile_adapter [max_tiles].

__global__ __launch_bounds__(LORA_ALIGN_NT) void lora_align_kernel(
    const int* __restrict__ idx, int N, int S, int* __restrict__ slot_map,
    int* __restrict__ tile_adapter, int* __restrict__ num_tiles) {
  __shared__ int cnt[LORA_MAX_S], start[LORA_MAX_S], fill[LORA_MAX_S];
  const int tid = threadIdx.x;
  if (tid < LORA_MAX_S) {
    cnt[tid] = 0;
    fill[tid] = 0;
  }
  __syncthreads();
  for (int p = tid; p < N; p += LORA_ALIGN_NT) {
    int s = idx[p];
    if ((unsigned)s < (unsigned)S) atomicAdd(&cnt[s], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int tile = 0;
    for (int s = 0; s < S; ++s) {
      start[s] = tile * LORA_BM;
      int nt = (cnt[s] + LORA_BM - 1) / LORA_BM;
      for (int i = 0; i < nt; ++i) tile_adapter[tile + i] = s;
      tile += nt;
    }
    *num_tiles = tile;
  }
  __syncthreads();
  // the pad slots behind each adapter's rows (fewer than 32 per adapter)
  for (int s = tid >> 5; s < S; s += LORA_ALIGN_NT / 32) {
    int c = cnt[s];
    int end = start[s] + (c + LORA_BM - 1) / LORA_BM * LORA_BM;
    int slot = start[s] + c + (tid & 31);
    if (slot < end) slot_map[slot] = -1;
  }
  for (int p = tid; p < N; p += LORA_ALIGN_NT) {
    int s = idx[p];
    if ((unsigned)s < (unsigned)S)
      slot_map[start[s] + atomicAdd(&fill[s], 1)] = p;
  }
}

// ---------------------------------------------------------------- shrink
// One wave per block: M-tile mtile (32 slots of one adapter) x NT 32-column
// N-tiles of t (NT = 2 for R = 64, else 1; for R = 16 the upper half of the
// one tile re-reads row R-1 and is not stored), over the chunks of K-slice z.
// x rows are gathered through the slot map; pad rows are masked to zero, not
// branched, so their t rows are written as zeros and expand can read every
// slot of a tile in use.  The loads of chunk i+1 are issued before the MFMAs
// of chunk i, two register sets in turn.

template <int NT>
struct LoraFrags {
  bf16x8 x[LORA_NF], a[NT][LORA_NF];
};

template <int NT>
DEV_INLINE void lora_load(LoraFrags<NT>& f, const short* px,
                          const short* const (&pa)[NT], int k0, short keep) {
#pragma unroll
  for (int c = 0; c < LORA_NF; ++c) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      f.a[t][c] = *(const bf16x8*)(pa[t] + k0 + c * 16);
    // keep is all ones, or zero on a pad row: a mask, not a select, so the
    // load itself stays unconditional
    f.x[c] = *(const bf16x8*)(px + k0 + c * 16) & keep;
  }
}

template <int NT>
DEV_INLINE void lora_mma(const LoraFrags<NT>& f, f32x16 (&acc)[NT]) {
#pragma unroll
  for (int c = 0; c < LORA_NF; ++c)
#pragma unroll
    for (int t = 0; t < NT; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.x[c], f.a[t][c],
                                                       acc[t], 0, 0, 0);
}

template <int NT>
__global__ __launch_bounds__(WAVE) void lora_shrink_kernel(
    const short* __restrict__ X, const short* __restrict__ A,
    const int* __restrict__ slot_map, const int* __restrict__ tile_adapter,
    const int* __restrict__ num_tiles, float* __restrict__ T, int N, int K,
    int R, int max_tiles, int cps, long long plane) {
  const int mtile = blockIdx.x % max_tiles;
  const int z = blockIdx.x / max_tiles;
  if (mtile >= *num_tiles) return;  // tiles past the device-side count
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int s = tile_adapter[mtile];
  const int row = slot_map[mtile * LORA_BM + l31];
  const bool pad = (unsigned)row >= (unsigned)N;
  const short keep = pad ? 0 : -1;
  const short* px = X + (pad ? 0 : (size_t)row) * K + hi5 * 8;
  const short* pa[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int r = t * 32 + l31;
    if (r >= R) r = R - 1;
    pa[t] = A + ((size_t)s * R + r) * K + hi5 * 8;
  }

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // two register sets in turn, k ascending: f0 holds chunk k0, f1 k0 + KC
  constexpr int KC = LORA_KC;
  int k0 = z * cps * KC;
  const int kend = k0 + cps * KC < K ? k0 + cps * KC : K;
  LoraFrags<NT> f0, f1;
  lora_load<NT>(f0, px, pa, k0, keep);
  for (; k0 + 2 * KC < kend; k0 += 2 * KC) {
    lora_load<NT>(f1, px, pa, k0 + KC, keep);
    lora_mma<NT>(f0, acc);
    lora_load<NT>(f0, px, pa, k0 + 2 * KC, keep);
    lora_mma<NT>(f1, acc);
  }
  if (k0 + KC < kend) {
    lora_load<NT>(f1, px, pa, k0 + KC, keep);
    lora_mma<NT>(f0, acc);
    lora_mma<NT>(f1, acc);
  } else {
    lora_mma<NT>(f0, acc);
  }

  // C fragment: register r of this lane is slot c_row(r, hi5), column l31
  float* tz = T + (size_t)z * plane + (size_t)mtile * LORA_BM * R;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = t * 32 + l31;
    if (col < R) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        tz[(size_t)c_row(r, hi5) * R + col] = acc[t][r];
    }
  }
}

// ---------------------------------------------------------------- expand
// One wave per block: M-tile mtile x LORA_CB output columns n0.., K = R =
// KS*16.  The t fragment of k-step c is t[slot l31][c*16 + hi5*8 ..+7]: eight
// consecutive floats of the lane's own workspace row, summed over the slice
// planes in ascending order and split into hi + lo.  The B[s] fragment of
// N-tile j is B[s][n0 + j*32 + l31][c*16 + hi5*8 ..+7], one 16 B load.
// SWAP: acc = B-tile . t^T, so register r of a lane is output column
// n0 + j*32 + c_row(r, hi5) of the lane's own row: four consecutive columns
// per register quad.

template <int KS, bool SWAP>
__global__ __launch_bounds__(WAVE) void lora_expand_kernel(
    const float* __restrict__ T, const short* __restrict__ B,
    const int* __restrict__ slot_map, const int* __restrict__ tile_adapter,
    const int* __restrict__ num_tiles, short* __restrict__ Y, int N, int O,
    int max_tiles, int slices, long long plane) {
  constexpr int R = KS * 16;
  constexpr int NT = LORA_CB / 32;
  const int mtile = blockIdx.x % max_tiles;
  const int n0 = blockIdx.x / max_tiles * LORA_CB;
  if (mtile >= *num_tiles) return;  // tiles past the device-side count
  const int lane = threadIdx.x, l31 = lane & 31, hi5 = lane >> 5;
  const int s = tile_adapter[mtile];
  const int slot = mtile * LORA_BM + l31;

  bf16x8 thi[KS], tlo[KS];
  const float* pt = T + (size_t)slot * R + hi5 * 8;
#pragma unroll
  for (int c = 0; c < KS; ++c) {
    f32x4 s0 = *(const f32x4*)(pt + c * 16);
    f32x4 s1 = *(const f32x4*)(pt + c * 16 + 4);
    for (int z = 1; z < slices; ++z) {
      f32x4 p0 = *(const f32x4*)(pt + z * plane + c * 16);
      f32x4 p1 = *(const f32x4*)(pt + z * plane + c * 16 + 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        s0[q] += p0[q];
        s1[q] += p1[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      short h0 = f2bf(s0[q]), h1 = f2bf(s1[q]);
      thi[c][q] = h0;
      thi[c][q + 4] = h1;
      tlo[c][q] = f2bf(s0[q] - bf2f(h0));  // the difference is exact in fp32
      tlo[c][q + 4] = f2bf(s1[q] - bf2f(h1));
    }
  }

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  const short* pb = B + ((size_t)s * O + n0 + l31) * R + hi5 * 8;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int c = 0; c < KS; ++c) {
      bf16x8 w = *(const bf16x8*)(pb + (size_t)j * 32 * R + c * 16);
      if (SWAP) {
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, thi[c], acc[j], 0,
                                                         0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, tlo[c], acc[j], 0,
                                                         0, 0);
      } else {
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(thi[c], w, acc[j], 0,
                                                         0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tlo[c], w, acc[j], 0,
                                                         0, 0);
      }
    }

  if (SWAP) {
    const int row = slot_map[slot];
    if ((unsigned)row >= (unsigned)N) return;  // a pad slot stores nothing
    short* yr = Y + (size_t)row * O + n0 + 4 * hi5;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4* p = (bf16x4*)(yr + j * 32 + 8 * g);
        bf16x4 v = *p;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          v[q] = f2bf(bf2f(v[q]) + acc[j][g * 4 + q]);
        *p = v;
      }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = slot_map[mtile * LORA_BM + c_row(r, hi5)];
      if ((unsigned)row < (unsigned)N) {
        short* yr = Y + (size_t)row * O + n0 + l31;
#pragma unroll
        for (int j = 0; j < NT; ++j)
          yr[j * 32] = f2bf(bf2f(yr[j * 32]) + acc[j][r]);
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
// The launchers return 0 once launched, non-zero (nothing launched) for a
// configuration outside what the kernels support.

static bool lora_shape_ok(long long N, int S) {
  return N >= 1 && N < (1ll << 30) && S >= 1 && S <= LORA_MAX_S;
}

extern "C" int lora_max_tiles(long long N, int S) {
  return (int)(N / LORA_BM) + S;
}

// The K-slices of the shrink GEMM for inner width K (= planes of the
// workspace), 0 for an unsupported K.  slices <= 0 asks for the rule: slices
// of at least LORA_SLICE_K, at most LORA_MAX_SLICES of them — a function of K
// only.  slices > 0 (the benchmark's sweep) is taken as given.  Either way
// the count is normalised so that no slice is empty.  Measured at N = 64 with
// four adapters (profiles/lora.txt): K = 4096 is fastest in 8 slices (9.7 us;
// 24.8 in one, 10.5 in 16), K = 14336 in 16 (13.5 us; 15.7 in 8, 73.6 in one).
extern "C" int lora_plan(int K, int slices) {
  if (K < LORA_KC || K % LORA_KC) return 0;
  const int nch = K / LORA_KC;
  int Z = slices;
  if (Z <= 0) {
    Z = (K + LORA_SLICE_K - 1) / LORA_SLICE_K;
    if (Z > LORA_MAX_SLICES) Z = LORA_MAX_SLICES;
  }
  if (Z > nch) return 0;
  const int cps = (nch + Z - 1) / Z;
  return (nch + cps - 1) / cps;
}

// sched is int32 [max_tiles*32 + max_tiles + 1]: slot_map, tile_adapter,
// num_tiles, with max_tiles = lora_max_tiles(N, S).
extern "C" int lora_align_i32(const int* idx, int* sched, long long N, int S,
                              hipStream_t stream) {
  if (!lora_shape_ok(N, S)) return 1;
  const int max_tiles = lora_max_tiles(N, S);
  int* tile_adapter = sched + (size_t)max_tiles * LORA_BM;
  hipLaunchKernelGGL(lora_align_kernel, dim3(1), dim3(LORA_ALIGN_NT), 0,
                     stream, idx, (int)N, S, sched, tile_adapter,
                     tile_adapter + max_tiles);
  return 0;
}

template <int KS>
static void lora_launch_expand(int swap, unsigned grid, hipStream_t stream,
                               const float* ws, const short* b,
                               const int* slot_map, const int* tile_adapter,
                               const int* num_tiles, short* y, int N, int O,
                               int max_tiles, int Z, long long plane) {
  if (swap)
    hipLaunchKernelGGL((lora_expand_kernel<KS, true>), dim3(grid), dim3(WAVE),
                       0, stream, ws, b, slot_map, tile_adapter, num_tiles, y,
                       N, O, max_tiles, Z, plane);
  else
    hipLaunchKernelGGL((lora_expand_kernel<KS, false>), dim3(grid), dim3(WAVE),
                       0, stream, ws, b, slot_map, tile_adapter, num_tiles, y,
                       N, O, max_tiles, Z, plane);
}

// y bf16 [N,O] in place, x bf16 [N,K], a bf16 [S,R,K], b bf16 [S,O,R], sched
// from lora_align_i32 for the same (N, S), ws f32 [Z, max_tiles*32, R] with
// Z = lora_plan(K, slices).
extern "C" int lora_apply_bf16(void* y, const void* x, const void* a,
                               const void* b, const int* sched, float* ws,
                               long long N, int K, int O, int S, int R,
                               int slices, int swap, hipStream_t stream) {
  if (!lora_shape_ok(N, S) || (R != 16 && R != 32 && R != 64) ||
      O < LORA_CB || O % LORA_CB)
    return 1;
  const int Z = lora_plan(K, slices);
  if (Z < 1) return 1;
  const int cps = (K / LORA_KC + Z - 1) / Z;
  const int max_tiles = lora_max_tiles(N, S);
  const long long expand_blocks = (long long)max_tiles * (O / LORA_CB);
  if (expand_blocks >= (1ll << 31) || N * (long long)O >= (1ll << 40) ||
      N * (long long)K >= (1ll << 40))
    return 1;
  const int* slot_map = sched;
  const int* tile_adapter = sched + (size_t)max_tiles * LORA_BM;
  const int* num_tiles = tile_adapter + max_tiles;
  const long long plane = (long long)max_tiles * LORA_BM * R;
  const unsigned sgrid = (unsigned)(max_tiles * Z);

  if (R == 64)
    hipLaunchKernelGGL((lora_shrink_kernel<2>), dim3(sgrid), dim3(WAVE), 0,
                       stream, (const short*)x, (const short*)a, slot_map,
                       tile_adapter, num_tiles, ws, (int)N, K, R, max_tiles,
                       cps, plane);
  else
    hipLaunchKernelGGL((lora_shrink_kernel<1>), dim3(sgrid), dim3(WAVE), 0,
                       stream, (const short*)x, (const short*)a, slot_map,
                       tile_adapter, num_tiles, ws, (int)N, K, R, max_tiles,
                       cps, plane);
  const unsigned egrid = (unsigned)expand_blocks;
  if (R == 16)
    lora_launch_expand<1>(swap, egrid, stream, ws, (const short*)b, slot_map,
                          tile_adapter, num_tiles, (short*)y, (int)N, O,
                          max_tiles, Z, plane);
  else if (R == 32)
    lora_launch_expand<2>(swap, egrid, stream, ws, (const short*)b, slot_map,
                          tile_adapter, num_tiles, (short*)y, (int)N, O,
                          max_tiles, Z, plane);
  else
    lora_launch_expand<4>(swap, egrid, stream, ws, (const short*)b, slot_map,
                          tile_adapter, num_tiles, (short*)y, (int)N, O,
                          max_tiles, Z, plane);
  return 0;
}
