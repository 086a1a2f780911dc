// Verify what csrc/linear_fp8.hip relies on from gfx950's two fp8 MFMA
// forms, with asymmetric e4m3 inputs:
//   K=64  v_mfma_scale_f32_32x32x64_f8f6f4, cbsz = blgp = 0, both scale
//         operands 0x7F7F7F7F: a lane's operand is 32 bytes
//   K=16  v_mfma_f32_32x32x16_fp8_fp8: a lane's operand is 8 bytes
// Claims under test, for both forms:
//   1. A and B map (lane half, byte of the operand) to the same k — "slot"
//      hi5 * BYTES + byte pairs with the same slot of the other operand;
//   2. the operands are read as OCP e4m3 (0x3C is 1.5; as e5m2 it would be 1)
//      and E8M0 127 is a unit scale: the sums come out unscaled and exact;
//   3. C[m][n] sits in register r of lane l with n = l & 31 and
//      m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)  (c_row()).
// Every product and sum below is a small multiple of 1/4, exact in fp32, so
// the comparison is ==.
//   hipcc --offload-arch=gfx950 -O2 -w scripts/probe_mfma_fp8.cpp -o out && ./out
// Printed on an MI355X:
//   K=64 f8f6f4 (e4m3, unit scales): same-slot pairing, e4m3, C layout OK
//   K=16 fp8_fp8: same-slot pairing, e4m3, C layout OK
#include <hip/hip_runtime.h>
#include <cstdio>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// A[m][slot] and B[n][slot] as e4m3 bytes, [32][2 * BYTES]
template <int BYTES>
__global__ void probe(const unsigned char* A, const unsigned char* B,
                      float* C) {
  const int l = threadIdx.x, l31 = l & 31, hi5 = l >> 5;
  union {
    unsigned char c[32];
    i32x8 v8;
    long v1;
  } a, b;
  for (int j = 0; j < BYTES; ++j) {
    a.c[j] = A[l31 * 2 * BYTES + hi5 * BYTES + j];
    b.c[j] = B[l31 * 2 * BYTES + hi5 * BYTES + j];
  }
  f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  if (BYTES == 32)
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
        a.v8, b.v8, acc, 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
  else
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a.v1, b.v1, acc, 0, 0, 0);
  for (int r = 0; r < 16; ++r)
    C[((r & 3) + 8 * (r >> 2) + 4 * hi5) * 32 + l31] = acc[r];
}

// e4m3 values used: 0, +-0.5, +-1, +-1.5, 2
static const unsigned char kByte[8] = {0x00, 0x30, 0x38, 0x3C,
                                       0x40, 0xB0, 0xB8, 0xBC};
static const float kVal[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, -0.5f, -1.f, -1.5f};

template <int BYTES>
static void run(const char* name) {
  const int KK = 2 * BYTES;
  unsigned char hA[32 * 64], hB[32 * 64], *A, *B;
  float fA[32 * 64], fB[32 * 64], hC[32 * 32], *C;
  for (int i = 0; i < 32 * KK; ++i) {
    // multiplicative hashes: no period along k that a slot mix-up could hide in
    int ia = ((unsigned)i * 2654435761u >> 13) % 8;
    int ib = ((unsigned)(i + 7919) * 2246822519u >> 11) % 8;
    hA[i] = kByte[ia], fA[i] = kVal[ia];
    hB[i] = kByte[ib], fB[i] = kVal[ib];
  }
  hipMalloc(&A, sizeof(hA));
  hipMalloc(&B, sizeof(hB));
  hipMalloc(&C, sizeof(hC));
  hipMemcpy(A, hA, sizeof(hA), hipMemcpyHostToDevice);
  hipMemcpy(B, hB, sizeof(hB), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(probe<BYTES>, dim3(1), dim3(64), 0, 0, A, B, C);
  hipError_t e = hipMemcpy(hC, C, sizeof(hC), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    printf("%s: HIP error %s\n", name, hipGetErrorString(e));
    return;
  }
  int bad = 0;
  for (int m = 0; m < 32; ++m)
    for (int n = 0; n < 32; ++n) {
      float want = 0;
      for (int k = 0; k < KK; ++k) want += fA[m * KK + k] * fB[n * KK + k];
      if (want != hC[m * 32 + n] && bad++ < 4)
        printf("%s: C[%d][%d]=%f want %f\n", name, m, n, hC[m * 32 + n], want);
    }
  if (bad)
    printf("%s: WRONG (%d mismatches)\n", name, bad);
  else
    printf("%s: same-slot pairing, e4m3, C layout OK\n", name);
  hipFree(A), hipFree(B), hipFree(C);
}

int main() {
  run<32>("K=64 f8f6f4 (e4m3, unit scales)");
  run<8>("K=16 fp8_fp8");
  return 0;
}
