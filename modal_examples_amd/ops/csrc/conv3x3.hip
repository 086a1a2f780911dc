// K3: hand-written NCHW implicit-GEMM 3x3 conv (stride 1, pad 1) on MFMA.
//
// Replaces MIOpen/CK for the SDXL VAE/UNet conv pyramid (reference trigger:
// 06_gpu_and_ml/stable_diffusion/text_to_image.py:114 VAE decode path,
// flux.py:259-261).  MIOpen's fastest solvers insert NCHW<->NHWC transpose
// pairs (~19 ms of the 390 ms SDXL step); this kernel consumes NCHW directly
// and does its one unavoidable transpose (x-contiguous -> c-contiguous) in
// LDS during staging.
//
// Formulation: 9 shifted GEMMs.  out[k][p] = sum_tap sum_c W[tap][k][c] *
// in[c][p+tap].  M = 64 out-channels, N = 256 pixels (8 rows x 32 cols),
// K-dim = C in chunks of 16 (mfma_f32_32x32x16_bf16).
//
//  - Input patch staged per 16-channel chunk as LDS [10 rows][34 cols][16 c]
//    (c innermost): the MFMA B-fragment read (8 consecutive c at the lane's
//    pixel) is one ds_read_b128 at 32 B col-stride -> 64 lanes cover a
//    contiguous span, every bank hit evenly (conflict-free; guide §6 G4
//    applies to same-column strides, not contiguous spans).
//  - Weights repacked on host to [9][Kpad][C16] (c contiguous) so the MFMA
//    A-fragment is one bf16x8 global read; per-k-tile weight working set
//    (64 x C x 9 x 2B <= 590 KB) stays L2-resident across the XCD-chunked
//    run of pixel tiles (bijective chunk swizzle, guide §5 T1/m204).
//  - Wave w owns output rows {2w, 2w+1} and BOTH 32-k fragments: 36 MFMA per
//    18 ds_read_b128 per chunk (2:1, the m97 GEMM ratio).
//  - Staging is software-pipelined: chunk cc+1's input and weight loads
//    issue back to back right after chunk cc's second barrier and are first
//    waited for after chunk cc's last MFMA.  Every input load is
//    UNCONDITIONAL from a clamped, always-valid address (row/col clamped into
//    the image, channel clamped to C-1, slot clamped to the last one); the
//    zero fill for padding pixels, spare slots and channels past C is an AND
//    with a 0/-1 mask when the values are packed for the LDS write.  A
//    `cond ? load : 0` per element makes hipcc branch around each load and
//    wait vmcnt(0) per element (guide §5 trap 4(c)), which serialised the
//    whole chunk in front of its MFMAs.
//  - Epilogue fuses bias add and an optional residual add (VAEResnet skip).
//    The block's 64 bias values sit in LDS from the prologue; residual loads
//    are unconditional (clamped on edge tiles) and issue 16 at a time with
//    one wait per batch; interior tiles carry no per-element condition, edge
//    tiles mask only the stores.
//  - Optional per-(n, k) addend (the UNet resnets' time-embedding
//    projection, broadcast over the pixels): out = bf16(bf16(acc + bias) +
//    addend[n][k]) - two roundings, the arithmetic of the separate broadcast
//    add over the conv's bf16 output that it replaces.  The block's 64 values
//    sit in LDS beside the bias.  Not combined with a residual.
//  - Offsets inside one image are 32-bit: the host checks C16*Hs*Ws and
//    64*H*W below 2^31 elements (bindings.cpp check_conv).
//
// The kernel is stride-1/pad-1 only; stride-2 downsample convs (3 per UNet
// fwd) stay on the library path.
#include "common.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#define CV_NW 4      // waves per block
#define CV_COLS 32   // output cols per block
#define CV_BK 64     // output channels per block
#define CV_CC 16     // input-channel chunk (MFMA K)

typedef __attribute__((ext_vector_type(16))) float f32x16c;

// GN staging value: silu(x*scale+shift) of one bf16, back to bf16 bits.
DEV_INLINE unsigned gn_silu_bf16(unsigned raw, float sc, float sh) {
  float f = bf2f((short)raw) * sc + sh;
  f = f / (1.f + __expf(-f));
  return (unsigned)(unsigned short)f2bf(f);
}

// A wave-uniform value moved to an SGPR.  The builtin readfirstlane is folded
// away when the compiler can prove the value uniform - and then leaves it in
// a VGPR; the s_nop covers the VALU-write -> readfirstlane hazard.
DEV_INLINE int to_sgpr(int v) {
  int s;
  asm volatile("s_nop 0\n\tv_readfirstlane_b32 %0, %1" : "=s"(s) : "v"(v));
  return s;
}

// RPW = output rows per wave (block rows = CV_NW*RPW).  RPW=2 runs 3
// waves/SIMD (its register budget: __launch_bounds__ below); RPW=4 doubles
// MFMA per staged byte/A-read at 1 wave/SIMD (128 accumulator registers).
// LDS patch: [rows+2][CV_COLS+2][CV_CC] bf16, c innermost.
#define PATCH_C (CV_COLS + 2)

// weight tile in LDS: [9 taps][CV_BK k][CV_CC c], staged once per c-chunk and
// shared by all 4 waves (per-wave global A-reads were 4x-redundant L2
// traffic — the v1 bottleneck).
#define WLDS_ELEMS (9 * CV_BK * CV_CC)
#define WSLOTS (WLDS_ELEMS / 8)  // bf16x8 units
#define WSLOTS_PER_T ((WSLOTS + CV_NW * WAVE - 1) / (CV_NW * WAVE))

// UP: fused nearest-2x upsample — the conv reads the half-res source
// directly (out pixel (y,x) <- src[y/2][x/2]), eliminating the materialized
// F.interpolate pass before every Upsample conv.  H/W are OUTPUT dims;
// Hs/Ws the source's.
// GN: fuse GroupNorm+SiLU into the staging read — silu(x*scale[c]+shift[c])
// with per-(n,c) coefficients from gn_conv_coeffs_bf16 (norms.hip).  The
// gn_norm write+read pass over the full tensor disappears.
template <bool UP, bool GN, int RPW>
__global__ __launch_bounds__(CV_NW * WAVE, RPW == 2 ? 3 : 1)
void conv3x3_kernel(
    const short* __restrict__ in, const short* __restrict__ wr,
    const float* __restrict__ bias, const short* __restrict__ res,
    const short* __restrict__ addend, short* __restrict__ out, const float* __restrict__ gn_scale,
    const float* __restrict__ gn_shift, int C, int H, int W, int Hs, int Ws,
    int K, int C16, int Kpad, int npix_x, int npix, int nk) {
  constexpr int CV_ROWS = CV_NW * RPW;
  constexpr int PATCH_R = CV_ROWS + 2;
  constexpr int PATCH_ELEMS = PATCH_R * PATCH_C * CV_CC;
  constexpr int STAGE_SLOTS = PATCH_R * PATCH_C * 2;  // (row, col, c-oct)
  constexpr int SLOTS_PER_T =
      (STAGE_SLOTS + CV_NW * WAVE - 1) / (CV_NW * WAVE);
  __shared__ alignas(16) short patch[PATCH_ELEMS];
  __shared__ alignas(16) short wlds[WLDS_ELEMS];
  __shared__ alignas(16) float bias_s[CV_BK];
  __shared__ alignas(16) float addend_s[CV_BK];

  const int tid = threadIdx.x;
  const int w = tid / WAVE;
  const int l = tid % WAVE;
  const int l31 = l & 31;
  const int hi5 = l >> 5;
  const int n = blockIdx.y;

  // bijective XCD-chunk swizzle (m204): each XCD runs a contiguous range of
  // block ids = consecutive pixel tiles of ONE k-tile -> weights L2-hit.
  int bid = blockIdx.x;
  {
    int nwg = npix * nk;
    int q = nwg >> 3, r = nwg & 7;
    int xcd = bid & 7, pos = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  // the division runs on the VALU and its (block-uniform) result would stay
  // in VGPRs, with every tile coordinate and address base built on it
  const int ktile = to_sgpr(bid / npix);
  const int pix = bid - ktile * npix;
  const int pix_y = pix / npix_x;
  const int y0 = pix_y * CV_ROWS;
  const int x0 = (pix - pix_y * npix_x) * CV_COLS;
  const int k0 = ktile * CV_BK;

  const long long in_n = (long long)n * C * Hs * Ws;
  const int nc = C16 / CV_CC;

  // bias: the block's 64 values go to LDS once (index clamped to K-1; the
  // loop's first barrier orders this write before the epilogue's reads).
  if (tid < CV_BK) {
    const int kc = min(k0 + tid, K - 1);
    bias_s[tid] = bias[kc];
    if (addend != nullptr) addend_s[tid] = bf2f(addend[(long long)n * K + kc]);
  }

  // ---- staging: slot s = (row, col, c-oct); thread gathers 8 strided
  // channel values (coalesced across lanes: consecutive threads read
  // consecutive x) and writes ONE bf16x8 to the c-contiguous LDS slot.
  // Fixed per slot for the whole kernel: the byte offset inside image n of
  // (clamped pixel, next chunk's channel oct*8) - advanced by 16 channels per
  // stage_load -, the pixel's last valid offset (channel C-1), the LDS
  // element offset, and a 0/-1 mask that is 0 for padding pixels and for the
  // slots past STAGE_SLOTS.
  const char* in_img = (const char*)(in + in_n);
  const unsigned hwb = (unsigned)Hs * (unsigned)Ws * 2u;  // channel stride, B
  unsigned soff[SLOTS_PER_T], soff_max[SLOTS_PER_T];
  int slds[SLOTS_PER_T], smask[SLOTS_PER_T];
#pragma unroll
  for (int i = 0; i < SLOTS_PER_T; ++i) {
    const int s_raw = i * CV_NW * WAVE + tid;
    const int s = min(s_raw, STAGE_SLOTS - 1);
    const int col = s % PATCH_C;
    const int u = s / PATCH_C;
    const int oct = u & 1;
    const int row = u >> 1;
    const int y = y0 + row - 1;
    const int x = x0 + col - 1;
    const bool live =
        s_raw < STAGE_SLOTS && y >= 0 && y < H && x >= 0 && x < W;
    const int yc = min(max(y, 0), H - 1);
    const int xc = min(max(x, 0), W - 1);
    const unsigned sy = UP ? (yc >> 1) : yc;
    const unsigned sx = UP ? (xc >> 1) : xc;
    const unsigned pix = (sy * (unsigned)Ws + sx) * 2u;
    soff[i] = pix + (unsigned)(oct * 8) * hwb;
    soff_max[i] = pix + (unsigned)(C - 1) * hwb;
    slds[i] = (row * PATCH_C + col) * CV_CC + oct * 8;
    // opaque to the optimiser: as a visible `live ? v : 0` the zero fill
    // turns back into a branch around every load
    int m = live ? -1 : 0;
    asm volatile("" : "+v"(m));
    smask[i] = m;
  }

  // All of a chunk's loads are unconditional and independent, so they issue
  // back to back; nothing here consumes a loaded value.
  unsigned sraw[SLOTS_PER_T][8];
  float gsc[GN ? CV_CC : 1], gsh[GN ? CV_CC : 1];  // chunk's GN coeffs
  auto stage_load = [&](int cc) {
#pragma unroll
    for (int i = 0; i < SLOTS_PER_T; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned o = min(soff[i] + (unsigned)j * hwb, soff_max[i]);
        sraw[i][j] = *(const unsigned short*)(in_img + o);
      }
      soff[i] += CV_CC * hwb;
    }
    if constexpr (GN) {
      // tiny [N, C16] arrays at a block-uniform address
      const float* ps = gn_scale + (long long)n * C16 + cc * CV_CC;
      const float* ph = gn_shift + (long long)n * C16 + cc * CV_CC;
#pragma unroll
      for (int j = 0; j < CV_CC; ++j) {
        gsc[j] = ps[j];
        gsh[j] = ph[j];
      }
    }
  };
  // The first use of the loaded values: (GN: normalise + SiLU,) pack pairs,
  // AND with the slot mask and the channel-tail mask, one 16-byte LDS write.
  auto stage_write = [&](int cc) {
    const int nv = C - cc * CV_CC;  // channels of this chunk below C (uniform)
#pragma unroll
    for (int i = 0; i < SLOTS_PER_T; ++i) {
      const int o8 = slds[i] & 8;  // oct * 8
      i32x4 pk;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        unsigned lo = sraw[i][2 * d], hi = sraw[i][2 * d + 1];
        // pin the first use here: left alone, hipcc hoists the pair packing
        // (and with it the wait for these loads) above the MFMA block
        asm volatile("" : "+v"(lo), "+v"(hi));
        if constexpr (GN) {
          lo = gn_silu_bf16(lo, o8 ? gsc[8 + 2 * d] : gsc[2 * d],
                            o8 ? gsh[8 + 2 * d] : gsh[2 * d]);
          hi = gn_silu_bf16(hi, o8 ? gsc[9 + 2 * d] : gsc[1 + 2 * d],
                            o8 ? gsh[9 + 2 * d] : gsh[1 + 2 * d]);
        }
        pk[d] = (int)((lo | (hi << 16)) & (unsigned)smask[i]);
      }
      // channel tail, last chunk only: a block-uniform branch round pure
      // ALU work; the masks are sign-bit arithmetic, never a select
      if (nv < CV_CC) {
        const int nvl = nv - o8;  // this oct's channels below C
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const unsigned lo = (unsigned)((2 * d - nvl) >> 31);
          const unsigned hi = (unsigned)((2 * d + 1 - nvl) >> 31);
          pk[d] &= (int)((lo & 0xffffu) | (hi & 0xffff0000u));
        }
      }
      // only the last round has spare slots
      if ((i + 1) * CV_NW * WAVE <= STAGE_SLOTS ||
          i * CV_NW * WAVE + tid < STAGE_SLOTS)
        *(i32x4*)&patch[slds[i]] = pk;
    }
  };

  // weight staging: slot = (tap, k-row, c-oct); one bf16x8 each.  The spare
  // slots of the last round re-read the last slot (no branch round a load).
  // Per-thread 32-bit byte offsets from the k-tile's (block-uniform) base.
  bf16x8 wreg[WSLOTS_PER_T];
  unsigned woff[WSLOTS_PER_T];
#pragma unroll
  for (int i = 0; i < WSLOTS_PER_T; ++i) {
    const int s = min(i * CV_NW * WAVE + tid, WSLOTS - 1);
    const int oct = s & 1;
    const int kr = (s >> 1) & (CV_BK - 1);
    const int tap = (s >> 1) >> 6;  // 64 k-rows per tap
    woff[i] = ((unsigned)(tap * Kpad + kr) * (unsigned)C16 + oct * 8) * 2u;
  }
  const char* w_tile = (const char*)(wr + (long long)k0 * C16);
  auto wstage_load = [&](int cc) {
    const char* wb = w_tile + cc * (CV_CC * 2);
#pragma unroll
    for (int i = 0; i < WSLOTS_PER_T; ++i)
      wreg[i] = *(const bf16x8*)(wb + woff[i]);
  };
  auto wstage_write = [&]() {
#pragma unroll
    for (int i = 0; i < WSLOTS_PER_T; ++i) {
      const int s = i * CV_NW * WAVE + tid;
      if ((i + 1) * CV_NW * WAVE <= WSLOTS || s < WSLOTS)
        *(bf16x8*)&wlds[s * 8] = wreg[i];
    }
  };

  // accumulators: [wave-row rr][k-fragment mf]
  f32x16c acc[RPW][2];
#pragma unroll
  for (int a = 0; a < RPW; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  stage_load(0);
  wstage_load(0);
  for (int cc = 0; cc < nc; ++cc) {
    __syncthreads();  // previous compute done; LDS free
    stage_write(cc);
    wstage_write();
    __syncthreads();  // patch + weights ready
    if (cc + 1 < nc) {
      stage_load(cc + 1);
      wstage_load(cc + 1);
    }

    // one base per operand; every tap/row is a compile-time LDS offset
    const short* wl = &wlds[l31 * CV_CC + hi5 * 8];
    const short* pl = &patch[(w * RPW * PATCH_C + l31) * CV_CC + hi5 * 8];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - 3 * (tap / 3);
      bf16x8 a0 = *(const bf16x8*)&wl[tap * CV_BK * CV_CC];
      bf16x8 a1 = *(const bf16x8*)&wl[(tap * CV_BK + 32) * CV_CC];
#pragma unroll
      for (int rr = 0; rr < RPW; ++rr) {
        bf16x8 b =
            *(const bf16x8*)&pl[((rr + dy) * PATCH_C + dx) * CV_CC];
        __builtin_amdgcn_s_setprio(1);
        acc[rr][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b, acc[rr][0], 0, 0, 0);
        acc[rr][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b, acc[rr][1], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
  }

  // ---- epilogue: bias (+ residual) add, NCHW store.  RES / EDGE are
  // block-uniform and decided once, outside: no load sits behind a
  // per-element condition.  Edge tiles clamp (y, x, k) for the residual
  // loads and mask the stores; interior tiles have no condition at all.
  // Offsets inside the block's (n, k0) slab of 64 planes are 32-bit.
  auto epilogue = [&](auto res_c, auto add_c, auto edge_c) {
    constexpr bool RES = decltype(res_c)::value;
    constexpr bool ADD = decltype(add_c)::value;
    constexpr bool EDGE = decltype(edge_c)::value;
    // lane coordinates rebuilt from an opaque copy of tid: kept live across
    // the main loop they cost registers the loop has not got
    int t = tid;
    asm volatile("" : "+v"(t));
    const int w = t / WAVE, l31 = t & 31, hi5 = (t >> 5) & 1;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const long long slab = ((long long)n * K + k0) * hw;
    // block-uniform bases, 32-bit byte offsets
    const char* resb = RES ? (const char*)(res + slab) : nullptr;
    char* outb = (char*)(out + slab);
    const int x = x0 + l31;
    const int kmax = K - 1 - k0;  // last valid k of this tile (EDGE)
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int y = y0 + w * RPW + rr;
      const bool pix_ok = !EDGE || (y < H && x < W);
      const unsigned po = EDGE ? (unsigned)min(y, H - 1) * W + min(x, W - 1)
                               : (unsigned)y * W + x;
#pragma unroll
      for (int mf = 0; mf < 2; ++mf) {
        unsigned rv[16];
        if constexpr (RES) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kl = mf * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi5;
            const unsigned ke = EDGE ? min(kl, kmax) : kl;
            rv[r] = *(const unsigned short*)(resb + (po + ke * hw) * 2u);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 b4 = *(const f32x4*)&bias_s[mf * 32 + 8 * q + 4 * hi5];
          f32x4 a4;
          if constexpr (ADD)
            a4 = *(const f32x4*)&addend_s[mf * 32 + 8 * q + 4 * hi5];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int r = q * 4 + j;
            const int kl = mf * 32 + j + 8 * q + 4 * hi5;
            float v = acc[rr][mf][r] + b4[j];
            if constexpr (RES) v += bf2f((short)rv[r]);
            if constexpr (ADD) v = bf2f(f2bf(v)) + a4[j];
            if (!EDGE || (pix_ok && kl <= kmax))
              *(short*)(outb + (po + (unsigned)kl * hw) * 2u) = f2bf(v);
          }
        }
      }
    }
  };
  const bool edge =
      y0 + CV_ROWS > H || x0 + CV_COLS > W || k0 + CV_BK > K;
  const std::true_type yes{};
  const std::false_type no{};
  if (res != nullptr) {
    if (edge) epilogue(yes, no, yes);
    else epilogue(yes, no, no);
  } else if (addend != nullptr) {
    if (edge) epilogue(no, yes, yes);
    else epilogue(no, yes, no);
  } else {
    if (edge) epilogue(no, no, yes);
    else epilogue(no, no, no);
  }
}

extern "C" void conv3x3_bf16(const void* in, const void* wrepack,
                             const void* bias, const void* residual,
                             const void* addend, void* out,
                             const float* gn_scale, const float* gn_shift,
                             int N, int C, int H, int W, int K, int C16,
                             int Kpad, int upsample, hipStream_t stream) {
  // H/W are the OUTPUT dims; with upsample the source is H/2 x W/2.
  const int Hs = upsample ? H / 2 : H;
  const int Ws = upsample ? W / 2 : W;
  // rows-per-wave A/B (MODAL_AMD_CONV_RPW=4): doubles MFMA per staged
  // byte/A-read at 1 wave/SIMD occupancy.
  static const int rpw = [] {
    const char* e = getenv("MODAL_AMD_CONV_RPW");
    return (e && atoi(e) == 4) ? 4 : 2;
  }();
  const int rows = CV_NW * rpw;
  const int npix_x = (W + CV_COLS - 1) / CV_COLS;
  const int npix_y = (H + rows - 1) / rows;
  const int npix = npix_x * npix_y;
  const int nk = (K + CV_BK - 1) / CV_BK;
  dim3 grid(npix * nk, N);
  dim3 block(CV_NW * WAVE);
  const bool gn = gn_scale != nullptr;
#define CVL(UPV, GNV, RPWV) \
  hipLaunchKernelGGL((conv3x3_kernel<UPV, GNV, RPWV>), grid, block, 0, \
                     stream, (const short*)in, (const short*)wrepack, \
                     (const float*)bias, (const short*)residual, \
                     (const short*)addend, (short*)out, \
                     gn_scale, gn_shift, C, H, W, Hs, Ws, K, C16, Kpad, \
                     npix_x, npix, nk)
  if (rpw == 4) {
    if (upsample) {
      if (gn) CVL(true, true, 4); else CVL(true, false, 4);
    } else {
      if (gn) CVL(false, true, 4); else CVL(false, false, 4);
    }
  } else {
    if (upsample) {
      if (gn) CVL(true, true, 2); else CVL(true, false, 2);
    } else {
      if (gn) CVL(false, true, 2); else CVL(false, false, 2);
    }
  }
#undef CVL
}
