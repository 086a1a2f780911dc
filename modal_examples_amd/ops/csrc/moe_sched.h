// What the MoE lanes share across translation units: the tile constants and
// the host launchers of the schedule (align) and the combine, both defined in
// moe.hip.  The grouped GEMMs between the two are each lane's own.
#pragma once
#include <hip/hip_runtime.h>

#define MOE_BM 32  // rows per M-tile = one 32x32 MFMA tile
#define MOE_MAX_E 128
#define MOE_MAX_K 8

extern "C" {
// N, E, top_k inside what route / align / combine support
int moe_shape_ok(long long N, int E, int top_k);
// tiles that bound any routing of N*top_k pairs over E experts
int moe_max_tiles(long long N, int top_k, int E);
// idx [P] -> sched int32 [max_tiles*32 + max_tiles + 1]: slot_map,
// tile_expert, num_tiles (moe_align_kernel)
void moe_align_launch(const int* idx, int P, int E, int max_tiles, int* sched,
                      hipStream_t stream);
// out bf16 [N,d] = sum_j weights[t,j] * (sum_z y[z][t*k+j]), y f32 [S][N*k][d]
void moe_combine_launch(const float* y, const float* weights, void* out,
                        long long N, int d, int top_k, int S,
                        hipStream_t stream);
}
