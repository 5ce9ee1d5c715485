// gram_f32x.hip — the node reduction  C[m x k] = A^T B  over the rows of two fp32 operands ([n, m], [n, k], m, k <= 256),
// with the column sums of A, as THREE bf16 matrix-core products: SGF_F32_BF16X3, what sgf_gram runs for fp32 storage under
// torch.set_float32_matmul_precision('high' / 'medium') — every dW / db of a Linear and G = h^T h.
//
// Each element is split as a = hi + lo (common.h split_bf16x2) and A^T B ~ Ahi^T Bhi + Ahi^T Blo + Alo^T Bhi on
// v_mfma_f32_32x32x16_bf16, fp32 accumulation (error model: DESIGN.md §4).  The exact path (k_attn_reduce<float, 256, 2>,
// csrc/attn.hip) runs v_mfma_f32_32x32x2_f32 at 1/16 of that rate and is MFMA-bound at d = 256.
//
// Layout, after csrc/gramx.hip (8 waves, wave (wm, wd) owns the 64 x 128 block of C, 2 x 4 accumulator tiles):
//   * stage = 32 rows of A and of B.  Unlike gramx the tiles come in through REGISTERS, not LDS-DMA: every element has to
//     pass through the VALU anyway to be split, so the staging pass loads a 4 row x 4 column patch of each operand (rows
//     128 bytes contiguous per 8 lanes), adds A's column sums in fp32, splits, and writes each column's 4 rows as one 8-byte
//     word into a [column][row] bf16 image.  A fragment (8 consecutive rows of one column) is then one ds_read_b128, with
//     no transposing read; image columns are 40 bf16 (80 bytes) apart, so 16 consecutive columns cover the 64 banks once.
//   * Stage depth and count: one stage is four images (A hi, A lo, B hi, B lo) of 256 columns x 80 bytes = 80 KiB — an fp32
//     stage (64 KiB) plus its two bf16 images would not fit gramx's 4-stage ring, and the fp32 stage never has to be in
//     LDS at all.  TWO stages (160 KiB, the whole LDS of a CU) make one barrier per stage enough: stage t + 1 is split into
//     the other buffer while stage t is multiplied, and its loads (64 KiB per CU, issued a stage ahead) are in flight during
//     both — at about 7 B per clock per CU of HBM, a stage's bytes take ~9000 clocks against ~3000 of MFMA and ~1500 of
//     splitting, so a deeper ring would buy nothing.
//   * Results are per-block partials in the layout of reduce_shared.h (DP = 256, RG = 1), added in a fixed order by
//     attn.hip's k_gram_finalize: deterministic, no atomics, and sharded runs all-reduce exactly what they do today.
#include "reduce_shared.h"

namespace sgf {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kGfThreads = 512;                 // 8 waves = 2 per SIMD
constexpr int kGfRows = 32;                     // rows per stage (two MFMA k-steps)
constexpr int kGfPitch = 40;                    // bf16 per image column: 32 rows + 16 bytes of pad
constexpr int kGfImage = 256 * kGfPitch;        // bf16 per image
constexpr int kGfStage = 4 * kGfImage;          // A hi, A lo, B hi, B lo

struct GramF32xArgs {
  const float* a;
  const float* b;
  int64_t lda, ldb;   // elements
  int64_t n;
  int32_t m, k;       // valid columns of a / b (multiples of 4, <= 256)
  float* partial;     // [gridDim.x][kRedPartialStride]
};

__global__ __launch_bounds__(kGfThreads) void k_gram_f32x(GramF32xArgs p) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * kGfStage];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wd = wave & 1;        // this wave's 64 x 128 block of C
  const int i31 = lane & 31, hh = lane >> 5;

  // staging: rows 4 r4 .. 4 r4 + 3, columns 4 c4 .. 4 c4 + 3 of both operands
  const int r4 = tid & 7, c4 = tid >> 3;
  const int col = 4 * c4;
  const bool a_ok = col < p.m, b_ok = col < p.k;
  float va[4][4], vb[4][4];
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t total = (p.n + kGfRows - 1) / kGfRows;

  auto issue = [&](int64_t t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = t * kGfRows + 4 * r4 + i;
      const bool ok = row < p.n;
      const float4 x = (a_ok && ok) ? *reinterpret_cast<const float4*>(p.a + row * p.lda + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 y = (b_ok && ok) ? *reinterpret_cast<const float4*>(p.b + row * p.ldb + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      va[i][0] = x.x; va[i][1] = x.y; va[i][2] = x.z; va[i][3] = x.w;
      vb[i][0] = y.x; vb[i][1] = y.y; vb[i][2] = y.z; vb[i][3] = y.w;
    }
  };
  auto commit = [&](int buf) {
    uint16_t* base = smem + buf * kGfStage + col * kGfPitch + 4 * r4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cs[q] += va[0][q];
      cs[q] += va[1][q];
      cs[q] += va[2][q];
      cs[q] += va[3][q];
      uint2 h, l;
      split_bf16x2(va[0][q], va[1][q], h.x, l.x);
      split_bf16x2(va[2][q], va[3][q], h.y, l.y);
      *reinterpret_cast<uint2*>(base + q * kGfPitch) = h;
      *reinterpret_cast<uint2*>(base + kGfImage + q * kGfPitch) = l;
      split_bf16x2(vb[0][q], vb[1][q], h.x, l.x);
      split_bf16x2(vb[2][q], vb[3][q], h.y, l.y);
      *reinterpret_cast<uint2*>(base + 2 * kGfImage + q * kGfPitch) = h;
      *reinterpret_cast<uint2*>(base + 3 * kGfImage + q * kGfPitch) = l;
    }
  };

  // accumulator tiles that hold valid columns (wave-uniform): rows 64 wm + 32 mt < m, columns 128 wd + 32 kt < k
  const int rem_a = p.m - 64 * wm, rem_b = p.k - 128 * wd;
  const int nta = rem_a <= 0 ? 0 : (rem_a > 32 ? 2 : 1);
  const int ntb = rem_b <= 0 ? 0 : (rem_b >= 128 ? 4 : (rem_b + 31) / 32);

  f32x16 acc[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][kt][r] = 0.f;

  int64_t t = blockIdx.x;
  int buf = 0;
  if (t < total) {
    issue(t);
    commit(0);
  }
  __syncthreads();
  for (; t < total; t += gridDim.x) {
    const int64_t next = t + gridDim.x;
    const bool has_next = next < total;
    if (has_next) issue(next);
    // lane (i31, hh) of k-step s: column i31 of the tile, rows 16 s + 8 hh .. + 7
    const uint16_t* fa = smem + buf * kGfStage + (64 * wm + i31) * kGfPitch + 8 * hh;
    const uint16_t* fb = smem + buf * kGfStage + 2 * kGfImage + (128 * wd + i31) * kGfPitch + 8 * hh;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 ah[2], al[2], bh[4], bl[4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        ah[mt] = *reinterpret_cast<const bf16x8*>(fa + 32 * mt * kGfPitch + 16 * s);
        al[mt] = *reinterpret_cast<const bf16x8*>(fa + kGfImage + 32 * mt * kGfPitch + 16 * s);
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        bh[kt] = *reinterpret_cast<const bf16x8*>(fb + 32 * kt * kGfPitch + 16 * s);
        bl[kt] = *reinterpret_cast<const bf16x8*>(fb + kGfImage + 32 * kt * kGfPitch + 16 * s);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (mt < nta && kt < ntb) {
            acc[mt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[kt], acc[mt][kt], 0, 0, 0);
            acc[mt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[kt], acc[mt][kt], 0, 0, 0);
            acc[mt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[kt], acc[mt][kt], 0, 0, 0);
          }
    }
    if (has_next) commit(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }

  float* part = p.partial + static_cast<int64_t>(blockIdx.x) * kRedPartialStride;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = 64 * wm + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
        part[i * 256 + 128 * wd + 32 * kt + i31] = acc[mt][kt][r];
      }
  // column sums of A: the 8 threads of a column chunk add theirs in row-group order (deterministic)
  float* red = reinterpret_cast<float*>(smem);      // [8][256]; the last barrier of the loop ended every LDS read
  *reinterpret_cast<float4*>(&red[r4 * 256 + col]) = make_float4(cs[0], cs[1], cs[2], cs[3]);
  __syncthreads();
  if (tid < 64) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(&red[g * 256 + 4 * tid]);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(part + kRedTileElems + 4 * tid) = s;
  }
}

}  // namespace

bool gram_f32x_supported(const void* a, int64_t lda, int m, const void* b, int64_t ldb, int k) {
  return m >= 4 && m <= 256 && m % 4 == 0 && k >= 4 && k <= 256 && k % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 &&
         reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0;
}

int gram_f32x(const float* a, int64_t lda, int m, const float* b, int64_t ldb, int k, int64_t n, float* partial, int* nblk,
              hipStream_t st) {
  SGF_REQUIRE(gram_f32x_supported(a, lda, m, b, ldb, k) && n > 0, SGF_E_UNSUPPORTED,
              "gram_f32x: m, k multiples of 4 up to 256, rows 16-byte aligned (m=%d k=%d)", m, k);
  const int64_t total = (n + kGfRows - 1) / kGfRows;
  const int nb = static_cast<int>(total < kRedMaxBlocks ? total : kRedMaxBlocks);
  GramF32xArgs p{a, b, lda, ldb, n, m, k, partial};
  hipLaunchKernelGGL(k_gram_f32x, dim3(nb), dim3(kGfThreads), 0, st, p);
  SGF_LAUNCH_CHECK();
  *nblk = nb;
  return SGF_OK;
}

}  // namespace sgf
