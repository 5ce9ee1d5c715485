// linear_f32x.hip — the fp32-storage Linear layers of csrc/linear_f32.hip (y = [x_1 | x_2] W^T + b with and without the
// BatchNorm column sums, dX = dY W, the DUAL head forward and backward) with every product formed as THREE bf16 matrix-core
// products: SGF_F32_BF16X3, what torch.set_float32_matmul_precision('high' / 'medium') asks for.
//
// Each fp32 operand is split as a = hi + lo (hi = bf16_rne(a), lo = bf16_rne(a - hi), common.h split_bf16x2) and
//     a b  ~  hi_a hi_b + hi_a lo_b + lo_a hi_b
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: three MFMAs per k-step of 16 against eight k-steps of 2 on the exact
// v_mfma_f32_32x32x2_f32, whose 1/16 rate makes k_linear_f32 MFMA-bound at d = 256 (about 2x its bytes at the copy rate).
// The dropped terms (lo_a lo_b and the two rounding residuals) bound each product's error by 3 * 2^-16 |a b|
// (DESIGN.md §4).
//
// Same skeleton and epilogue contract as k_linear_f32: waves = column strips x row sub-blocks x K-halves, the weight piece
// of a wave resident in registers for the whole (persistent) kernel, row tiles double-buffered through LDS, the K-halves'
// accumulators added in the row-wise epilogue (+ bias, + addend, shifted column sums, DUAL outputs).  What differs:
//   * the A rows are split ONCE, in the staging pass that already moves every element through registers: the tile lands in
//     LDS as two bf16 planes (hi, lo) — the same bytes as the fp32 tile — so the column-strip waves that read a row read
//     ready fragments (one ds_read_b128 per plane and k-step) and none of them redoes the split;
//   * W is split when a wave loads its piece: hi + lo take as many VGPRs as the fp32 piece.  No split copy of W is cached
//     anywhere: Adam updates W in place between launches;
//   * at DP = 256 a wave holds its strip's whole K (see lin_kh).
// Plane rows are DP + 8 bf16 apart (16 bytes of pad: 8 consecutive fragment rows start 4 banks apart).
#include "linear_shared.h"

namespace sgf {
namespace {

// K-halves per column strip: 2 at DP <= 128 (1024 threads, as k_linear_f32); at DP = 256 the split piece of a half-K wave
// (64 VGPRs) plus its operands spills at 4 waves per SIMD, so there a wave keeps its strip's whole K (128 VGPRs) and the
// block is 512 threads = 2 waves per SIMD with 256 registers each
template <int DP>
constexpr int lin_kh() { return DP == 256 ? 1 : 2; }
template <int DP>
constexpr int lin_threads() { return 512 * lin_kh<DP>(); }

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 zero4f() { return make_float4(0.f, 0.f, 0.f, 0.f); }

template <int DP, bool STATS, bool DUAL>
__global__ __launch_bounds__(lin_threads<DP>()) void k_linear_f32x(LinArgs p) {
  constexpr int KH = lin_kh<DP>();    // K-halves
  constexpr int NT = lin_threads<DP>();
  constexpr int NS = DP / 32;         // 32-column strips
  constexpr int RS = 8 / NS;          // row sub-blocks
  constexpr int RT = 32 * RS;         // rows per tile (32 / 64 / 128)
  constexpr int F4 = DP / 4;
  constexpr int RPP = NT / F4;        // rows covered per staging pass
  constexpr int NP = RT / RPP;        // staging passes (2, or 4 at DP = 256)
  constexpr int LD = DP + 4;          // fp32 accumulator rows
  constexpr int LH = DP + 8;          // bf16 plane rows
  constexpr int KW = DP / KH;         // k range of a wave
  constexpr int KS = KW / 16;         // its k-steps of 16
  constexpr int PLANE = RT * LH;      // bf16 elements per plane
  // [buf][hi, lo][RT][LH] bf16 (= 2 PLANE floats), then [kh][RT][LD] fp32
  __shared__ __attribute__((aligned(16))) float smem[2 * PLANE + KH * RT * LD];
  uint16_t* const ldsA = reinterpret_cast<uint16_t*>(smem);
  float* const ldsC = smem + 2 * PLANE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i31 = lane & 31;
  const int hi = lane >> 5;
  const int kh = wave % KH;
  const int ws = (wave / KH) % NS;
  const int wr = (wave / KH) / NS;

  // resident piece of the matrix, split: element e of bh[s] / bl[s] = B[KW kh + 16 s + 8 hi + e][32 ws + i31]
  bf16x8 bh[KS], bl[KS];
  {
    const int j = 32 * ws + i31;
    auto wval = [&](int k) -> float {
      if (k >= p.dk || j >= p.dj) return 0.f;
      return p.trans_w ? p.w[static_cast<int64_t>(j) * p.ldw + k] : p.w[static_cast<int64_t>(k) * p.ldw + j];
    };
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      u32x4 h, l;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = KW * kh + 16 * s + 8 * hi + 2 * t;
        uint32_t hh, ll;
        split_bf16x2(wval(k), wval(k + 1), hh, ll);
        h[t] = hh;
        l[t] = ll;
      }
      bh[s] = __builtin_bit_cast(bf16x8, h);
      bl[s] = __builtin_bit_cast(bf16x8, l);
    }
  }
  const int scol = (tid % F4) * 4;
  const int srow0 = tid / F4;
  const bool in_ok = scol < p.dk, out_ok = scol < p.dj;
  float4 s1 = zero4f(), s2 = zero4f();
  const float* pa = p.a + scol;
  const float* pa2 = (DUAL && p.a2) ? p.a2 + scol : nullptr;
  float4 ra[NP];
  const int64_t ntiles = (p.n + RT - 1) / RT;
  auto issue = [&](int64_t tile) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t row = tile * RT + srow0 + i * RPP;
      ra[i] = (in_ok && row < p.n) ? *reinterpret_cast<const float4*>(pa + row * p.lda) : zero4f();
      if (DUAL && pa2 != nullptr) {                     // the combination a * x1 + b * x2, in fp32, then split
        const float4 r2 = (in_ok && row < p.n) ? *reinterpret_cast<const float4*>(pa2 + row * p.lda2) : zero4f();
        ra[i] = make_float4(p.ca * ra[i].x + p.cb * r2.x, p.ca * ra[i].y + p.cb * r2.y, p.ca * ra[i].z + p.cb * r2.z,
                            p.ca * ra[i].w + p.cb * r2.w);
      }
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      uint2 h, l;
      split_bf16x2(ra[i].x, ra[i].y, h.x, l.x);
      split_bf16x2(ra[i].z, ra[i].w, h.y, l.y);
      uint16_t* dst = ldsA + (2 * buf * RT + srow0 + i * RPP) * LH + scol;
      *reinterpret_cast<uint2*>(dst) = h;
      *reinterpret_cast<uint2*>(dst + PLANE) = l;
    }
  };
  int64_t tile = blockIdx.x;
  int buf = 0;
  if (tile < ntiles) {
    issue(tile);
    commit(0);
  }
  __syncthreads();
  for (; tile < ntiles; tile += gridDim.x) {
    const int64_t next = tile + gridDim.x;
    const bool has_next = next < ntiles;
    if (has_next) issue(next);
    {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      // lane (i31, hi) of k-step s: row 32 wr + i31, k = KW kh + 16 s + 8 hi .. + 7 of each plane
      const uint16_t* Ah = ldsA + (2 * buf * RT + 32 * wr + i31) * LH + KW * kh + 8 * hi;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Ah + 16 * s);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(Ah + PLANE + 16 * s);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[s], acc, 0, 0, 0);
      }
      float* C = ldsC + (kh * RT + 32 * wr + 4 * hi) * LD + 32 * ws + i31;
#pragma unroll
      for (int r = 0; r < 16; ++r) C[((r & 3) + 8 * (r >> 2)) * LD] = acc[r];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int lrow = srow0 + i * RPP;
      const int64_t row = tile * RT + lrow;
      if (out_ok && row < p.n) {
        const float4 c0 = *reinterpret_cast<const float4*>(&ldsC[lrow * LD + scol]);
        const float4 c1 = KH == 2 ? *reinterpret_cast<const float4*>(&ldsC[(RT + lrow) * LD + scol]) : zero4f();
        const float4 bz = p.bias ? *reinterpret_cast<const float4*>(p.bias + scol) : zero4f();
        float4 v = make_float4((c0.x + c1.x) + bz.x, (c0.y + c1.y) + bz.y, (c0.z + c1.z) + bz.z, (c0.w + c1.w) + bz.w);
        if (p.addend) {
          const float4 o = *reinterpret_cast<const float4*>(p.addend + row * p.ldadd + scol);
          v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
        }
        if (DUAL && p.out2 != nullptr) {                // dx1 = a (g W), dx2 = b (g W): one product, two scaled copies
          *reinterpret_cast<float4*>(p.out + row * p.ldo + scol) = make_float4(p.co * v.x, p.co * v.y, p.co * v.z, p.co * v.w);
          *reinterpret_cast<float4*>(p.out2 + row * p.ldo2 + scol) =
              make_float4(p.co2 * v.x, p.co2 * v.y, p.co2 * v.z, p.co2 * v.w);
        } else {
          *reinterpret_cast<float4*>(p.out + row * p.ldo + scol) = v;
        }
        if (STATS) {
          const float4 sh = p.shift ? *reinterpret_cast<const float4*>(p.shift + scol) : zero4f();
          const float4 u = make_float4(v.x - sh.x, v.y - sh.y, v.z - sh.z, v.w - sh.w);
          s1.x += u.x; s1.y += u.y; s1.z += u.z; s1.w += u.w;
          s2.x = fmaf(u.x, u.x, s2.x); s2.y = fmaf(u.y, u.y, s2.y); s2.z = fmaf(u.z, u.z, s2.z); s2.w = fmaf(u.w, u.w, s2.w);
        }
      }
    }
    if (has_next) commit(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  if (STATS) {
    // the RPP threads that share a column chunk add their sums in thread order (deterministic)
    float* red = smem;                                   // [RPP][2][DP]
    *reinterpret_cast<float4*>(&red[(srow0 * 2 + 0) * DP + scol]) = s1;
    *reinterpret_cast<float4*>(&red[(srow0 * 2 + 1) * DP + scol]) = s2;
    __syncthreads();
    if (srow0 < 2 && out_ok) {
      float4 t = zero4f();
#pragma unroll 4
      for (int r = 0; r < RPP; ++r) {
        const float4 q = *reinterpret_cast<const float4*>(&red[(r * 2 + srow0) * DP + scol]);
        t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
      }
      *reinterpret_cast<float4*>(p.spart + (static_cast<int64_t>(blockIdx.x) * 2 + srow0) * p.dj + scol) = t;
    }
  }
}

}  // namespace

// the launch half of linear_f32 / linear_f32_dual (csrc/linear_f32.hip) for x3 != 0: arguments checked there, same grid
int linear_f32x_launch(const LinArgs& p, int DP, bool stats, bool dual, int blocks, hipStream_t st) {
#define SGF_LINX(DP_)                                                                                                    \
  do {                                                                                                                   \
    const dim3 block(lin_threads<DP_>());                                                                                \
    if (dual) hipLaunchKernelGGL((k_linear_f32x<DP_, false, true>), dim3(blocks), block, 0, st, p);                      \
    else if (stats) hipLaunchKernelGGL((k_linear_f32x<DP_, true, false>), dim3(blocks), block, 0, st, p);                \
    else hipLaunchKernelGGL((k_linear_f32x<DP_, false, false>), dim3(blocks), block, 0, st, p);                          \
  } while (0)
  if (DP == 64) SGF_LINX(64);
  else if (DP == 128) SGF_LINX(128);
  else SGF_LINX(256);
#undef SGF_LINX
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}

}  // namespace sgf
