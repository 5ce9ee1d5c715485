// linear_shared.h — the argument block of the fp32-storage Linear kernels: the exact-fp32 one (csrc/linear_f32.hip) and the
// split-bf16 one (csrc/linear_f32x.hip).  Not part of the C ABI.
#pragma once
#include "common.h"

namespace sgf {

struct LinArgs {
  const float* a;
  int64_t lda;
  const float* w;          // trans_w = 1: B[k][j] = w[j * ldw + k] (y = x W^T);  0: B[k][j] = w[k * ldw + j] (dx = dy W)
  int64_t ldw;
  int32_t trans_w;
  const float* bias;       // [dj] or null
  const float* addend;     // [n, dj] or null
  int64_t ldadd;
  const float* shift;      // [dj] or null (statistics are of out - shift)
  float* out;
  int64_t ldo;
  int64_t n;
  int32_t dk, dj;
  float* spart;            // [gridDim.x][2 * dj] per-block column sums / sums of squares, or null
  // DUAL form (T7 for fp32 storage, large/ours.py:269-275): the A operand is ca * a + cb * a2, formed while the row tile is
  // staged (a2 != null), and / or the result leaves twice, co * v -> out and co2 * v -> out2 (out2 != null)
  const float* a2;
  int64_t lda2;
  float ca, cb;
  float* out2;
  int64_t ldo2;
  float co, co2;
};

// csrc/linear_f32x.hip: the same products as three bf16 matrix-core products (SGF_F32_BF16X3); DP in {64, 128, 256}
int linear_f32x_launch(const LinArgs& p, int DP, bool stats, bool dual, int blocks, hipStream_t st);

}  // namespace sgf
