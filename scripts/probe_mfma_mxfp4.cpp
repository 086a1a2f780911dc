// Verify what csrc/linear_mxfp4.hip relies on from gfx950's block-scaled MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4 with an e4m3 A operand (cbsz = 0, 32 bytes
// per lane) against an e2m1 B operand (blgp = 4, 16 bytes per lane = 32
// nibbles) and one E8M0 scale byte per lane per operand, picked by op_sel
// from the lane's scale register.
// Claims under test (h = lane >> 5, row = lane & 31, k = 0..63):
//   1. pairing: nibble i of B's 16 bytes (low nibble of byte i / 2 first)
//      is k = 32 * h + i, a lane holds one block of 32 consecutive k; byte
//      j of A's 32 bytes is k = 16 * h + j for j < 16 and k = 32 + 16 * h +
//      (j - 16) above, a lane holds two runs of 16.  (The first guess, byte
//      j of A at k = 32 * h + j like B's nibbles, is what the device
//      refuses: with it this probe printed C[0][0] = -26 where the plain
//      dot product is -29.25, and -26 is the sum under the layout above.)
//   2. decode: the 16 e2m1 codes are 0, 0.5, 1, 1.5, 2, 3, 4, 6 and, with
//      bit 3 set, their negatives; code 0x8 contributes nothing (-0);
//   3. scale lane: byte op_sel (0..3) of lane l's B scale register applies
//      to that lane's 32 k of row l & 31 and to nothing else — every lane
//      carries its own exponent and the other three bytes of the register
//      carry different ones, A's scale byte stays 127;
//   4. scale decode: the byte means 2^(byte - 127), checked at 97 (2^-30)
//      and 157 (2^30) on B against 127 on A;
//   5. the upper four registers of the builtin's 8-register B operand are
//      ignored for fp4: filling them with ones changes nothing.
// A holds 0, +-0.5, +-1, +-1.5, 2; every product is a multiple of 1/4, the
// block exponents are within +-3 (or one common +-30), so all sums are exact
// in fp32 and the comparison is ==.
//   hipcc --offload-arch=gfx950 -O2 -w scripts/probe_mfma_mxfp4.cpp -o out && ./out
// Printed on an MI355X:
//   pairing + decode (hashed, unit scales): OK
//   decode, code by code: OK
//   scale lane, op_sel 0: OK
//   scale lane, op_sel 1: OK
//   scale lane, op_sel 2: OK
//   scale lane, op_sel 3: OK
//   scale decode, byte 97 (2^-30): OK
//   scale decode, byte 157 (2^30): OK
//   upper four B registers ignored: OK
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// A [32][64] e4m3 bytes, B [32][32] bytes (64 nibbles a row), SB [64] scale
// registers (one per lane), hi: what the upper four B registers hold
template <int SEL>
__global__ void probe(const unsigned char* A, const unsigned char* B,
                      const unsigned* SB, int hi, float* C) {
  const int l = threadIdx.x, l31 = l & 31, hi5 = l >> 5;
  union {
    unsigned char c[32];
    i32x8 v;
  } a, b;
  for (int j = 0; j < 32; ++j)
    a.c[j] = A[l31 * 64 + (j < 16 ? 16 * hi5 + j : 32 + 16 * hi5 + j - 16)];
  for (int j = 0; j < 16; ++j) b.c[j] = B[l31 * 32 + hi5 * 16 + j];
  for (int j = 4; j < 8; ++j) b.v[j] = hi;
  f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
      a.v, b.v, acc, 0 /* A: e4m3 */, 4 /* B: e2m1 */, 0, 0x7F7F7F7F, SEL,
      (int)SB[l]);
  for (int r = 0; r < 16; ++r)
    C[((r & 3) + 8 * (r >> 2) + 4 * hi5) * 32 + l31] = acc[r];
}

static const unsigned char kByte[8] = {0x00, 0x30, 0x38, 0x3C,
                                       0x40, 0xB0, 0xB8, 0xBC};
static const float kVal[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, -0.5f, -1.f, -1.5f};
static const float kFp4[16] = {0.f,  0.5f,  1.f,  1.5f,  2.f,  3.f,  4.f,  6.f,
                               -0.f, -0.5f, -1.f, -1.5f, -2.f, -3.f, -4.f, -6.f};

static unsigned char *dA, *dB;
static unsigned* dS;
static float* dC;

// fA [32][64] values of A, code [32][64] nibbles of B, ex [64] the exponent
// of each lane's block; sel / garbage as the kernel's
static void check(const char* name, const unsigned char* hA, const float* fA,
                  const unsigned char* code, const int* ex, int sel, int hi) {
  unsigned char hB[32 * 32];
  unsigned hS[64];
  float hC[32 * 32];
  for (int n = 0; n < 32; ++n)
    for (int j = 0; j < 32; ++j)
      hB[n * 32 + j] = code[n * 64 + 2 * j] | (code[n * 64 + 2 * j + 1] << 4);
  for (int l = 0; l < 64; ++l) {
    hS[l] = 0;
    for (int byte = 0; byte < 4; ++byte) {
      // the other bytes: exponents that differ from the lane's own
      int e = byte == sel ? ex[l] : ex[l] + 1 + (l + byte) % 3;
      hS[l] |= (unsigned)(127 + e) << (8 * byte);
    }
  }
  hipMemcpy(dA, hA, 32 * 64, hipMemcpyHostToDevice);
  hipMemcpy(dB, hB, sizeof(hB), hipMemcpyHostToDevice);
  hipMemcpy(dS, hS, sizeof(hS), hipMemcpyHostToDevice);
  switch (sel) {
    case 0: hipLaunchKernelGGL(probe<0>, dim3(1), dim3(64), 0, 0, dA, dB, dS, hi, dC); break;
    case 1: hipLaunchKernelGGL(probe<1>, dim3(1), dim3(64), 0, 0, dA, dB, dS, hi, dC); break;
    case 2: hipLaunchKernelGGL(probe<2>, dim3(1), dim3(64), 0, 0, dA, dB, dS, hi, dC); break;
    default: hipLaunchKernelGGL(probe<3>, dim3(1), dim3(64), 0, 0, dA, dB, dS, hi, dC);
  }
  hipError_t e = hipMemcpy(hC, dC, sizeof(hC), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    printf("%s: HIP error %s\n", name, hipGetErrorString(e));
    return;
  }
  int bad = 0;
  for (int m = 0; m < 32; ++m)
    for (int n = 0; n < 32; ++n) {
      double want = 0;
      for (int k = 0; k < 64; ++k)  // lane n + 32 * (k / 32) holds B's block
        want += (double)fA[m * 64 + k] * kFp4[code[n * 64 + k]] *
                ldexp(1.0, ex[n + 32 * (k / 32)]);
      if ((float)want != hC[m * 32 + n] && bad++ < 4)
        printf("%s: C[%d][%d]=%g want %g\n", name, m, n, hC[m * 32 + n], want);
    }
  if (bad)
    printf("%s: WRONG (%d mismatches)\n", name, bad);
  else
    printf("%s: OK\n", name);
}

int main() {
  unsigned char hA[32 * 64], code[32 * 64];
  float fA[32 * 64];
  int ex[64], zero[64] = {0};
  char name[64];
  hipMalloc(&dA, 32 * 64);
  hipMalloc(&dB, 32 * 32);
  hipMalloc(&dS, 64 * sizeof(unsigned));
  hipMalloc(&dC, 32 * 32 * sizeof(float));
  for (int i = 0; i < 32 * 64; ++i) {
    // multiplicative hashes: no period along k that a slot mix-up could hide in
    int ia = ((unsigned)i * 2654435761u >> 13) % 8;
    hA[i] = kByte[ia], fA[i] = kVal[ia];
    code[i] = ((unsigned)(i + 7919) * 2246822519u >> 11) % 16;
  }
  check("pairing + decode (hashed, unit scales)", hA, fA, code, zero, 0, 0);

  // row m of A is 1 at k = m and at k = 32 + m: C[m][n] is the sum of two
  // codes of row n; the codes step with k and with k / 16, so no two of a
  // row's 16-runs look alike
  unsigned char uA[32 * 64], ucode[32 * 64];
  float ufA[32 * 64];
  for (int m = 0; m < 32; ++m)
    for (int k = 0; k < 64; ++k) {
      uA[m * 64 + k] = k % 32 == m ? 0x38 : 0;
      ufA[m * 64 + k] = k % 32 == m ? 1.f : 0.f;
      ucode[m * 64 + k] = (m + k + k / 16) % 16;
    }
  check("decode, code by code", uA, ufA, ucode, zero, 0, 0);

  for (int l = 0; l < 64; ++l) ex[l] = (int)((unsigned)(l + 1) * 2654435761u >> 9) % 7 - 3;
  for (int sel = 0; sel < 4; ++sel) {
    snprintf(name, sizeof(name), "scale lane, op_sel %d", sel);
    check(name, hA, fA, code, ex, sel, 0);
  }
  for (int l = 0; l < 64; ++l) ex[l] = -30;
  check("scale decode, byte 97 (2^-30)", hA, fA, code, ex, 1, 0);
  for (int l = 0; l < 64; ++l) ex[l] = 30;
  check("scale decode, byte 157 (2^30)", hA, fA, code, ex, 2, 0);
  check("upper four B registers ignored", hA, fA, code, zero, 0, -1);
  hipFree(dA), hipFree(dB), hipFree(dS), hipFree(dC);
  return 0;
}
