// head_rows.hip — T7 on the SEED rows of a neighbour-sampled batch (100M/nb-sample.py:29 and :41):
//     output = model(graph.x, graph.edge_index)[:batch_size];  loss = nn.CrossEntropyLoss()(output, graph.y[:batch_size])
// reads m of the n rows of the head's result (1 000 of 756 000 for a [15, 10, 5] batch).  The full head computes, stores
// and differentiates all n rows; these entries touch the m selected rows only:
//
//   sgf_head_rows_fwd : logits_j = round(a x1[r_j] + b x2[r_j]) W^T + bias, compact fp32 [m, C]; with labels also the
//                       log-sum-exp of every row, the summed cross-entropy and the {labelled, correct} counts
//   sgf_head_rows_bwd : g from the caller or formed as softmax - onehot; dx1 / dx2 = a / b (g W) on the selected rows and
//                       exact zeros on every other row; dW = g^T z and db = sum_j g_j reduced here, nothing of size n read
//
// gfx950 mapping.  m is a thousand rows: the work is a few MFLOP and the kernels are latency-bound, so the layout is the
// simplest one that keeps every access in bounds and every sum in a fixed order.  A workgroup owns 32 selected rows.
//   * bf16 storage: v_mfma_f32_32x32x16_bf16 with the fragment layout of csrc/head.hip — A: lane (i31, hi) holds 8
//     consecutive k of row i31 (16 bytes of x1 and of x2, combined in fp32 and rounded to bf16 once, where sgf_axpby rounds),
//     B: 8 consecutive k of W's class row, rounded to bf16 as csrc/head.hip rounds it.  Wave w takes class tiles w, w + 4.
//   * fp32 storage: fp32 operands as they are under every matmul-precision setting, FMAs with fp64 accumulators (a product
//     of two fp32 values is exact there: each result is rounded to fp32 once), z staged in LDS 128 columns at a time.
//   * the 32 x C logits tile is parked in LDS: stored from there as whole rows, and reduced per row (max / first argmax /
//     sum of exp) by one wave for the cross-entropy epilogue.  Ragged class counts are masked; W is never padded or copied.
//   * backward: the 32 x C gradient tile is formed in LDS (and left compact in the workspace for dW); dX = g W on the
//     bf16 matrix cores (g rounded to bf16 as csrc/head.hip does) or in fp32 FMAs; in the prefix form the workgroups behind
//     the row tiles stream zeros over rows m .. n-1 in the same launch.
//   * dW / db: row slices of 128 selected rows x 8 classes per workgroup, thread = feature, fixed-order partial sums, then
//     the slices are added in slice order.  Deterministic.
#include "common.h"

namespace sgf {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kHrThreads = 256;      // 4 waves
constexpr int kHrRows = 32;          // selected rows per workgroup
constexpr int kHrMaxC = 256;
constexpr int kHrMaxD = 256;
constexpr int kHrPitch = kHrMaxC + 1;    // floats per LDS row of the logits / gradient tile
constexpr int kHrChunk = 128;        // fp32 forward: columns of z staged per pass
constexpr int kHrZPitch = kHrChunk + 4;
constexpr int kHrZeroBlocks = 1024;  // prefix form: workgroups that stream zeros behind the row tiles
constexpr int kHrDwClasses = 8;      // classes per workgroup of the weight-gradient pass
constexpr int kHrDwRows = 128;       // selected rows per slice of the weight-gradient pass ...
constexpr int kHrDwMaxSlices = 64;   // ... stretched when m is large

__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return static_cast<uint32_t>(f32_to_bf16(lo)) | (static_cast<uint32_t>(f32_to_bf16(hi)) << 16);
}
__device__ __forceinline__ float lo16(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi16(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

union Frag {
  bf16x8 v;
  uint4 u;
};

// node row of selected row j (j is clamped to the selection, the row to [0, n): no address depends on unchecked data)
__device__ __forceinline__ int64_t sel_row(const int64_t* __restrict__ idx, int64_t j, int64_t m, int64_t n) {
  if (j >= m) j = m - 1;
  int64_t r = idx ? idx[j] : j;
  if (r < 0) r = 0;
  if (r >= n) r = n - 1;
  return r;
}

// z = a x1 + b x2 (x2 may be absent) for 8 consecutive bf16 elements, rounded to bf16 once
__device__ __forceinline__ uint4 combine8(const uint16_t* __restrict__ p1, float a, const uint16_t* __restrict__ p2, float b) {
  const uint4 v1 = *reinterpret_cast<const uint4*>(p1);
  uint4 o;
  if (p2) {
    const uint4 v2 = *reinterpret_cast<const uint4*>(p2);
    o.x = pack2(a * lo16(v1.x) + b * lo16(v2.x), a * hi16(v1.x) + b * hi16(v2.x));
    o.y = pack2(a * lo16(v1.y) + b * lo16(v2.y), a * hi16(v1.y) + b * hi16(v2.y));
    o.z = pack2(a * lo16(v1.z) + b * lo16(v2.z), a * hi16(v1.z) + b * hi16(v2.z));
    o.w = pack2(a * lo16(v1.w) + b * lo16(v2.w), a * hi16(v1.w) + b * hi16(v2.w));
  } else {
    o.x = pack2(a * lo16(v1.x), a * hi16(v1.x));
    o.y = pack2(a * lo16(v1.y), a * hi16(v1.y));
    o.z = pack2(a * lo16(v1.z), a * hi16(v1.z));
    o.w = pack2(a * lo16(v1.w), a * hi16(v1.w));
  }
  return o;
}

// one element of z in fp32 registers, rounded as it would be stored
template <typename T>
__device__ __forceinline__ float combine1(const T* __restrict__ p1, float a, const T* __restrict__ p2, float b) {
  const float v = p2 ? a * load1<T>(p1) + b * load1<T>(p2) : a * load1<T>(p1);
  if constexpr (std::is_same<T, uint16_t>::value) return bf16_to_f32(f32_to_bf16(v));
  return v;
}

struct HrFwd {
  const void* x1;
  int64_t ld1;
  float a;
  const void* x2;
  int64_t ld2;
  float b;
  const float* w;
  const float* bias;
  const int64_t* idx;
  int64_t n, m;
  int d, c;
  float* logits;
  int64_t ldl;
  const int64_t* labels;   // null: no cross-entropy epilogue
  float* lse;
  float* part_loss;        // [blocks]
  int* part_cnt;           // [blocks][2]
};

// torch.argmax's order on the CPU (sgf_argmax_count): the first maximal column, a NaN is the maximum, the first NaN wins
__device__ __forceinline__ bool arg_better(float v, int col, float bv, int bc) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || col < bc);
  return v > bv || (v == bv && col < bc);
}

template <typename T>
__global__ __launch_bounds__(kHrThreads) void k_hr_fwd(const HrFwd p) {
  constexpr bool kBf16 = std::is_same<T, uint16_t>::value;
  __shared__ float lg[kHrRows * kHrPitch];
  __shared__ float zt[kBf16 ? 1 : kHrRows * kHrZPitch];
  __shared__ float red_loss[kHrThreads / 64];
  __shared__ int red_cnt[kHrThreads / 64][2];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kHrRows;
  const int d = p.d, c = p.c;
  const T* x1 = static_cast<const T*>(p.x1);
  const T* x2 = static_cast<const T*>(p.x2);

  if constexpr (kBf16) {
    const int i31 = lane & 31, hi = lane >> 5;
    const int64_t r = sel_row(p.idx, j0 + i31, p.m, p.n);
    const uint16_t* p1 = x1 + r * p.ld1 + 8 * hi;
    const uint16_t* p2 = x2 ? x2 + r * p.ld2 + 8 * hi : nullptr;
    const int ntile = (c + 31) / 32;                 // class tiles; this wave: wid and wid + 4
    const int cls0 = 32 * wid + i31, cls1 = 32 * (wid + 4) + i31;
    const float* w0 = p.w + static_cast<int64_t>(cls0 < c ? cls0 : c - 1) * d + 8 * hi;
    const float* w1 = p.w + static_cast<int64_t>(cls1 < c ? cls1 : c - 1) * d + 8 * hi;
    const bool t0 = wid < ntile, t1 = wid + 4 < ntile;     // (wave-uniform)
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc0[q] = acc1[q] = 0.f;
    if (t0) {
      for (int s = 0; s < d / 16; ++s) {
        Frag fa;
        fa.u = combine8(p1 + 16 * s, p.a, p2 ? p2 + 16 * s : nullptr, p.b);
        {
          const float4 u0 = *reinterpret_cast<const float4*>(w0 + 16 * s);
          const float4 u1 = *reinterpret_cast<const float4*>(w0 + 16 * s + 4);
          Frag fb;
          fb.u.x = pack2(u0.x, u0.y), fb.u.y = pack2(u0.z, u0.w), fb.u.z = pack2(u1.x, u1.y), fb.u.w = pack2(u1.z, u1.w);
          if (cls0 >= c) fb.u = make_uint4(0, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v, fb.v, acc0, 0, 0, 0);
        }
        if (t1) {
          const float4 u0 = *reinterpret_cast<const float4*>(w1 + 16 * s);
          const float4 u1 = *reinterpret_cast<const float4*>(w1 + 16 * s + 4);
          Frag fb;
          fb.u.x = pack2(u0.x, u0.y), fb.u.y = pack2(u0.z, u0.w), fb.u.z = pack2(u1.x, u1.y), fb.u.w = pack2(u1.z, u1.w);
          if (cls1 >= c) fb.u = make_uint4(0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v, fb.v, acc1, 0, 0, 0);
        }
      }
      const float bias0 = cls0 < c ? p.bias[cls0] : 0.f;
      const float bias1 = cls1 < c ? p.bias[cls1] : 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rl = mfma32_row(q, lane);
        if (cls0 < c) lg[rl * kHrPitch + cls0] = acc0[q] + bias0;
        if (t1 && cls1 < c) lg[rl * kHrPitch + cls1] = acc1[q] + bias1;
      }
    }
  } else {
    // thread (wid, lane): rows 8 wid .. 8 wid + 7, classes lane + 64 q
    // fp64 accumulators: a product of two fp32 values is exact in fp64, so a logit is rounded once, whatever d is
    double acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[i][q] = 0.0;
    const float* wq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cls = lane + 64 * q;
      wq[q] = p.w + static_cast<int64_t>(cls < c ? cls : c - 1) * d;
    }
    for (int k0 = 0; k0 < d; k0 += kHrChunk) {
      const int kc = d - k0 < kHrChunk ? d - k0 : kHrChunk;     // (a multiple of 4)
      __syncthreads();
      for (int e = threadIdx.x; e < kHrRows * (kc / 4); e += kHrThreads) {
        const int row = e / (kc / 4), col = (e % (kc / 4)) * 4;
        const int64_t r = sel_row(p.idx, j0 + row, p.m, p.n);
        const float4 v1 = *reinterpret_cast<const float4*>(x1 + r * p.ld1 + k0 + col);
        float4 z;
        if (x2) {
          const float4 v2 = *reinterpret_cast<const float4*>(x2 + r * p.ld2 + k0 + col);
          z = make_float4(p.a * v1.x + p.b * v2.x, p.a * v1.y + p.b * v2.y, p.a * v1.z + p.b * v2.z, p.a * v1.w + p.b * v2.w);
        } else {
          z = make_float4(p.a * v1.x, p.a * v1.y, p.a * v1.z, p.a * v1.w);
        }
        *reinterpret_cast<float4*>(&zt[row * kHrZPitch + col]) = z;
      }
      __syncthreads();
      for (int k = 0; k < kc; k += 4) {
        float4 wv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wv[q] = *reinterpret_cast<const float4*>(wq[q] + k0 + k);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float4 z = *reinterpret_cast<const float4*>(&zt[(8 * wid + i) * kHrZPitch + k]);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[i][q] = fma(static_cast<double>(z.x), static_cast<double>(wv[q].x), acc[i][q]);
            acc[i][q] = fma(static_cast<double>(z.y), static_cast<double>(wv[q].y), acc[i][q]);
            acc[i][q] = fma(static_cast<double>(z.z), static_cast<double>(wv[q].z), acc[i][q]);
            acc[i][q] = fma(static_cast<double>(z.w), static_cast<double>(wv[q].w), acc[i][q]);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cls = lane + 64 * q;
      if (cls < c) {
        const float bq = p.bias[cls];
#pragma unroll
        for (int i = 0; i < 8; ++i) lg[(8 * wid + i) * kHrPitch + cls] = static_cast<float>(acc[i][q] + static_cast<double>(bq));
      }
    }
  }
  __syncthreads();

  // the tile leaves as whole rows
  for (int e = threadIdx.x; e < kHrRows * c; e += kHrThreads) {
    const int row = e / c, col = e - row * c;
    if (j0 + row < p.m) p.logits[(j0 + row) * p.ldl + col] = lg[row * kHrPitch + col];
  }
  if (!p.labels) return;

  // cross-entropy epilogue: wave w reduces rows 8 w .. 8 w + 7, lane 0 keeps the wave's sums in row order
  float wloss = 0.f;
  int wcnt = 0, whit = 0;
  for (int i = 0; i < 8; ++i) {
    const int row = 8 * wid + i;
    const int64_t j = j0 + row;
    if (j >= p.m) break;                              // (wave-uniform)
    const float* lr = lg + row * kHrPitch;
    float bv = -INFINITY;
    int bc = 0x7fffffff;
    for (int col = lane; col < c; col += 64) {
      const float v = lr[col];
      if (arg_better(v, col, bv, bc)) bv = v, bc = col;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oc = __shfl_xor(bc, off, 64);
      if (arg_better(ov, oc, bv, bc)) bv = ov, bc = oc;
    }
    float s = 0.f;
    for (int col = lane; col < c; col += 64) s += expf(lr[col] - bv);
    s = group_sum<64>(s);
    const float l = bv + logf(s);
    if (lane == 0) {
      p.lse[j] = l;
      const int64_t y = p.labels[j];
      if (y >= 0 && y < c) {
        wloss += logf(s) + (bv - lr[y]);      // lse - logit, the maximum taken off first: exact zero where the label wins
        ++wcnt;
        whit += bc == static_cast<int>(y) ? 1 : 0;
      }
    }
  }
  if (lane == 0) red_loss[wid] = wloss, red_cnt[wid][0] = wcnt, red_cnt[wid][1] = whit;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    int n0 = 0, n1 = 0;
    for (int w = 0; w < kHrThreads / 64; ++w) s += red_loss[w], n0 += red_cnt[w][0], n1 += red_cnt[w][1];
    p.part_loss[blockIdx.x] = s;
    p.part_cnt[2 * blockIdx.x] = n0;
    p.part_cnt[2 * blockIdx.x + 1] = n1;
  }
}

// one wave: lane l adds partials l, l + 64, ... in order, then a fixed shuffle tree
__global__ void k_hr_sum(const float* __restrict__ part_loss, const int* __restrict__ part_cnt, int nblk,
                         float* __restrict__ loss_sum, int64_t* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  float s = 0.f;
  long long n0 = 0, n1 = 0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part_loss[b], n0 += part_cnt[2 * b], n1 += part_cnt[2 * b + 1];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    s += __shfl_xor(s, off, 64);
    n0 += __shfl_xor(n0, off, 64);
    n1 += __shfl_xor(n1, off, 64);
  }
  if (threadIdx.x == 0) loss_sum[0] = s, counts[0] = n0, counts[1] = n1;
}

struct HrBwd {
  const float* w;
  const int64_t* idx;
  int64_t n, m;
  int d, c;
  float a, b;
  const float* dlogits;    // generic form ...
  int64_t lddl;
  const float* logits;     // ... or the cross-entropy form
  int64_t ldl;
  const float* lse;
  const int64_t* labels;
  const float* gout;
  float inv_denom;
  void* dx1;
  int64_t ldd1;
  void* dx2;               // null when x2 is absent
  int64_t ldd2;
  float* g;                // [m, c] compact, fp32: the operand of the weight gradient
  int ntiles;              // workgroups >= ntiles stream zeros over rows m .. n-1 (prefix form)
};

template <typename T>
__global__ __launch_bounds__(kHrThreads) void k_hr_bwd(const HrBwd p) {
  constexpr bool kBf16 = std::is_same<T, uint16_t>::value;
  const int d = p.d, c = p.c;
  T* dx1 = static_cast<T*>(p.dx1);
  T* dx2 = static_cast<T*>(p.dx2);
  if (static_cast<int>(blockIdx.x) >= p.ntiles) {
    // 16-byte zero stores over the d columns of rows m .. n-1 of both gradients
    const int upr = d * static_cast<int>(sizeof(T)) / 16;
    const int64_t units = (p.n - p.m) * upr;
    const int64_t step = static_cast<int64_t>(gridDim.x - p.ntiles) * kHrThreads;
    const bool small = units < (static_cast<int64_t>(1) << 31);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (int64_t u = static_cast<int64_t>(blockIdx.x - p.ntiles) * kHrThreads + threadIdx.x; u < units; u += step) {
      int64_t row;
      int q;
      if (small) {
        const uint32_t rr = static_cast<uint32_t>(u) / static_cast<uint32_t>(upr);
        row = rr;
        q = static_cast<int>(static_cast<uint32_t>(u) - rr * static_cast<uint32_t>(upr));
      } else {
        row = u / upr;
        q = static_cast<int>(u - row * upr);
      }
      row += p.m;
      *reinterpret_cast<uint4*>(reinterpret_cast<char*>(dx1 + row * p.ldd1) + 16 * q) = zero;
      if (dx2) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(dx2 + row * p.ldd2) + 16 * q) = zero;
    }
    return;
  }
  __shared__ float gl[kHrRows * kHrPitch];
  __shared__ int rsel[kHrRows];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kHrRows;
  if (threadIdx.x < kHrRows) rsel[threadIdx.x] = static_cast<int>(sel_row(p.idx, j0 + threadIdx.x, p.m, p.n));
  const float scale = p.dlogits ? 0.f : p.gout[0] * p.inv_denom;
  for (int e = threadIdx.x; e < kHrRows * c; e += kHrThreads) {
    const int row = e / c, col = e - row * c;
    const int64_t j = j0 + row;
    float g = 0.f;
    if (j < p.m) {
      if (p.dlogits) {
        g = p.dlogits[j * p.lddl + col];
      } else {
        // softmax off the label column; the label's own entry, p_y - 1, is formed below as minus the sum of the others
        // (the row sums to zero): no cancellation where p_y is close to 1
        const int64_t y = p.labels[j];
        if (y >= 0 && y < c && y != col) g = scale * expf(p.logits[j * p.ldl + col] - p.lse[j]);
      }
      p.g[j * c + col] = g;
    }
    gl[row * kHrPitch + col] = g;
  }
  __syncthreads();
  if (!p.dlogits) {
    if (threadIdx.x < kHrRows && j0 + threadIdx.x < p.m) {
      const int64_t j = j0 + threadIdx.x;
      const int64_t y = p.labels[j];
      if (y >= 0 && y < c) {
        float* gr = gl + threadIdx.x * kHrPitch;
        float s = 0.f;
        for (int col = 0; col < c; ++col) s += col == y ? 0.f : gr[col];      // columns in order: a fixed sum
        gr[y] = -s;
        p.g[j * c + y] = -s;
      }
    }
    __syncthreads();
  }

  if constexpr (kBf16) {
    // D[row][feature] = sum_class g[row][class] W[class][feature]: A = g (bf16), B = W (bf16), feature tiles wid, wid + 4
    const int i31 = lane & 31, hi = lane >> 5;
    const int ks = (c + 15) / 16;
    const int nft = d / 32;
    for (int ft = wid; ft < nft; ft += kHrThreads / 64) {
      const int f = 32 * ft + i31;
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = 0.f;
      for (int s = 0; s < ks; ++s) {
        const int k0 = 16 * s + 8 * hi;
        float ga[8], wb[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int cls = k0 + j;
          ga[j] = cls < c ? gl[i31 * kHrPitch + cls] : 0.f;
          const float wv = p.w[static_cast<int64_t>(cls < c ? cls : c - 1) * d + f];
          wb[j] = cls < c ? wv : 0.f;
        }
        Frag fa, fb;
        fa.u.x = pack2(ga[0], ga[1]), fa.u.y = pack2(ga[2], ga[3]), fa.u.z = pack2(ga[4], ga[5]), fa.u.w = pack2(ga[6], ga[7]);
        fb.u.x = pack2(wb[0], wb[1]), fb.u.y = pack2(wb[2], wb[3]), fb.u.z = pack2(wb[4], wb[5]), fb.u.w = pack2(wb[6], wb[7]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa.v, fb.v, acc, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rl = mfma32_row(q, lane);
        if (j0 + rl < p.m) {
          const int64_t r = rsel[rl];
          dx1[r * p.ldd1 + f] = f32_to_bf16(p.a * acc[q]);
          if (dx2) dx2[r * p.ldd2 + f] = f32_to_bf16(p.b * acc[q]);
        }
      }
    }
  } else {
    // thread: one feature, 8 rows (a row group is wave-uniform when d % 64 == 0: LDS broadcast reads)
    for (int o = threadIdx.x; o < (kHrRows / 8) * d; o += kHrThreads) {
      const int rg = o / d, f = o - rg * d;
      double acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.0;
      for (int cls = 0; cls < c; ++cls) {
        const double wv = p.w[static_cast<int64_t>(cls) * d + f];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fma(static_cast<double>(gl[(8 * rg + i) * kHrPitch + cls]), wv, acc[i]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rl = 8 * rg + i;
        if (j0 + rl < p.m) {
          const int64_t r = rsel[rl];
          dx1[r * p.ldd1 + f] = static_cast<float>(static_cast<double>(p.a) * acc[i]);
          if (dx2) dx2[r * p.ldd2 + f] = static_cast<float>(static_cast<double>(p.b) * acc[i]);
        }
      }
    }
  }
}

// part[slice][class][0 .. d-1] = sum over the slice's rows of g[j][class] z[j][.], part[slice][class][d] = sum of g[j][class]
// grid (class groups of 8, slices); thread = feature.  Rows in order: a fixed sum.
template <typename T>
__global__ __launch_bounds__(kHrMaxD) void k_hr_dw_part(const T* __restrict__ x1, int64_t ld1, float a, const T* __restrict__ x2,
                                                        int64_t ld2, float b, const int64_t* __restrict__ idx, int64_t n,
                                                        int64_t m, int d, int c, const float* __restrict__ g,
                                                        int64_t slice_rows, float* __restrict__ part) {
  const int f = threadIdx.x;
  const int c0 = blockIdx.x * kHrDwClasses;
  const int64_t lo = static_cast<int64_t>(blockIdx.y) * slice_rows;
  const int64_t hi = lo + slice_rows < m ? lo + slice_rows : m;
  double acc[kHrDwClasses], gs[kHrDwClasses];      // fp64 inside a slice: a slice's partial is rounded once
#pragma unroll
  for (int q = 0; q < kHrDwClasses; ++q) acc[q] = gs[q] = 0.0;
  for (int64_t j = lo; j < hi; ++j) {
    const int64_t r = sel_row(idx, j, m, n);
    const double z = f < d ? combine1<T>(x1 + r * ld1 + f, a, x2 ? x2 + r * ld2 + f : nullptr, b) : 0.f;
#pragma unroll
    for (int q = 0; q < kHrDwClasses; ++q) {
      const double gv = g[j * c + (c0 + q < c ? c0 + q : c - 1)];
      acc[q] = fma(gv, z, acc[q]);
      gs[q] += gv;
    }
  }
  float* out = part + static_cast<int64_t>(blockIdx.y) * c * (d + 1);
#pragma unroll
  for (int q = 0; q < kHrDwClasses; ++q) {
    if (c0 + q < c) {
      if (f < d) out[static_cast<int64_t>(c0 + q) * (d + 1) + f] = static_cast<float>(acc[q]);
      if (f == 0) out[static_cast<int64_t>(c0 + q) * (d + 1) + d] = static_cast<float>(gs[q]);
    }
  }
}

// dw[class][f] / db[class] = the slices' partials added in slice order
__global__ __launch_bounds__(kHrThreads) void k_hr_dw_sum(const float* __restrict__ part, int slices, int d, int c,
                                                          float* __restrict__ dw, float* __restrict__ db) {
  const int e = blockIdx.x * kHrThreads + threadIdx.x;
  if (e >= c * (d + 1)) return;
  float s = 0.f;
  for (int sl = 0; sl < slices; ++sl) s += part[static_cast<int64_t>(sl) * c * (d + 1) + e];
  const int cls = e / (d + 1), f = e - cls * (d + 1);
  if (f < d) dw[static_cast<int64_t>(cls) * d + f] = s;
  else db[cls] = s;
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

inline bool hr_shape_ok(int d, int c, int dtype) {
  if (d <= 0 || d > kHrMaxD || c < 1 || c > kHrMaxC) return false;
  if (dtype == SGF_BF16) return d % 32 == 0;
  if (dtype == SGF_F32) return d % 4 == 0;
  return false;
}

inline int64_t hr_tiles(int64_t m) { return (m + kHrRows - 1) / kHrRows; }

inline void hr_slices(int64_t m, int64_t& slice_rows, int& slices) {
  int64_t s = (m + kHrDwRows - 1) / kHrDwRows;
  if (s > kHrDwMaxSlices) s = kHrDwMaxSlices;
  if (s < 1) s = 1;
  slice_rows = (m + s - 1) / s;
  if (slice_rows < 1) slice_rows = 1;
  slices = static_cast<int>((m + slice_rows - 1) / slice_rows);
  if (slices < 1) slices = 1;
}

// the sizes and the operands both entries share; x pointers are checked by the callers (m == 0 needs none)
int check_hr(const char* fn, int64_t ld1, const void* x2, int64_t ld2, int64_t n, int d, int c, int dtype, int64_t m) {
  SGF_REQUIRE(dtype == SGF_F32 || dtype == SGF_BF16, SGF_E_INVALID, "%s: dtype %d (SGF_F32 or SGF_BF16)", fn, dtype);
  SGF_REQUIRE(n >= 0 && m >= 0 && m <= n && d >= 1 && c >= 1, SGF_E_INVALID, "%s: bad sizes n=%lld m=%lld d=%d classes=%d", fn,
              static_cast<long long>(n), static_cast<long long>(m), d, c);
  SGF_REQUIRE(n < (static_cast<int64_t>(1) << 31), SGF_E_UNSUPPORTED, "%s: more than 2^31 - 1 rows", fn);
  SGF_REQUIRE(hr_shape_ok(d, c, dtype), SGF_E_UNSUPPORTED,
              "%s: needs d <= %d with d %% 32 == 0 (bf16) or d %% 4 == 0 (fp32) and classes <= %d (d=%d, classes=%d)", fn,
              kHrMaxD, kHrMaxC, d, c);
  const int64_t q = dtype == SGF_BF16 ? 8 : 4;      // elements per 16 bytes
  SGF_REQUIRE(ld1 >= d && ld1 % q == 0 && (!x2 || (ld2 >= d && ld2 % q == 0)), SGF_E_INVALID,
              "%s: leading dimensions must cover d and keep rows 16-byte aligned (ld1=%lld ld2=%lld)", fn,
              static_cast<long long>(ld1), static_cast<long long>(ld2));
  return SGF_OK;
}

}  // namespace
}  // namespace sgf

using namespace sgf;

extern "C" int32_t sgf_head_rows_supported(int32_t d, int32_t classes, int32_t dtype) {
  return hr_shape_ok(d, classes, dtype) ? 1 : 0;
}

extern "C" size_t sgf_head_rows_fwd_workspace_bytes(int64_t m) {
  const int64_t t = hr_tiles(m < 1 ? 1 : m);
  return static_cast<size_t>(t) * (sizeof(float) + 2 * sizeof(int));
}

extern "C" size_t sgf_head_rows_bwd_workspace_bytes(int64_t m, int32_t d, int32_t classes) {
  if (m < 1 || d < 1 || classes < 1) return 256;
  int64_t slice_rows;
  int slices;
  hr_slices(m, slice_rows, slices);
  const size_t g = align_up(static_cast<size_t>(m) * classes * sizeof(float), 256);
  return g + static_cast<size_t>(slices) * classes * (d + 1) * sizeof(float);
}

extern "C" int sgf_head_rows_fwd(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b, const float* w,
                                 const float* bias, int64_t n, int32_t d, int32_t classes, int32_t dtype,
                                 const int64_t* idx, int64_t m, float* logits, int64_t ldl, const int64_t* labels,
                                 float* lse, float* loss_sum, int64_t* counts, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* fn = "sgf_head_rows_fwd";
  if (int rc = check_hr(fn, ld1, x2, ld2, n, d, classes, dtype, m)) return rc;
  SGF_REQUIRE(ldl >= classes, SGF_E_INVALID, "%s: ldl=%lld < classes=%d", fn, static_cast<long long>(ldl), classes);
  SGF_REQUIRE(!labels || (loss_sum && counts), SGF_E_INVALID, "%s: labels need loss_sum and counts", fn);
  SGF_REQUIRE(m == 0 || (x1 && w && bias && logits), SGF_E_INVALID, "%s: null pointer", fn);
  SGF_REQUIRE(m == 0 || !labels || lse, SGF_E_INVALID, "%s: labels need lse", fn);
  SGF_REQUIRE(m == 0 || (aligned16(x1) && aligned16(x2) && aligned16(w)), SGF_E_INVALID,
              "%s: x1 / x2 / w must be 16-byte aligned", fn);
  SGF_REQUIRE(m == 0 || !labels || (workspace && workspace_bytes >= sgf_head_rows_fwd_workspace_bytes(m)), SGF_E_WORKSPACE,
              "%s: workspace too small", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m == 0) {
    if (labels) {
      SGF_CHECK_HIP(hipMemsetAsync(loss_sum, 0, sizeof(float), st));
      SGF_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    }
    return SGF_OK;
  }
  const int nblk = static_cast<int>(hr_tiles(m));
  HrFwd p;
  p.x1 = x1, p.ld1 = ld1, p.a = a, p.x2 = x2, p.ld2 = ld2, p.b = b, p.w = w, p.bias = bias, p.idx = idx, p.n = n, p.m = m;
  p.d = d, p.c = classes, p.logits = logits, p.ldl = ldl, p.labels = labels, p.lse = lse;
  p.part_loss = static_cast<float*>(workspace);
  p.part_cnt = labels ? reinterpret_cast<int*>(p.part_loss + nblk) : nullptr;
  if (dtype == SGF_BF16)
    hipLaunchKernelGGL(k_hr_fwd<uint16_t>, dim3(nblk), dim3(kHrThreads), 0, st, p);
  else
    hipLaunchKernelGGL(k_hr_fwd<float>, dim3(nblk), dim3(kHrThreads), 0, st, p);
  SGF_LAUNCH_CHECK();
  if (labels) {
    hipLaunchKernelGGL(k_hr_sum, dim3(1), dim3(64), 0, st, p.part_loss, p.part_cnt, nblk, loss_sum, counts);
    SGF_LAUNCH_CHECK();
  }
  return SGF_OK;
}

extern "C" int sgf_head_rows_bwd(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b, const float* w,
                                 int64_t n, int32_t d, int32_t classes, int32_t dtype, const int64_t* idx, int64_t m,
                                 const float* dlogits, int64_t lddl, const float* logits, int64_t ldl, const float* lse,
                                 const int64_t* labels, const float* gout, float inv_denom, void* dx1, int64_t ldd1,
                                 void* dx2, int64_t ldd2, float* dw, float* db, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const char* fn = "sgf_head_rows_bwd";
  if (int rc = check_hr(fn, ld1, x2, ld2, n, d, classes, dtype, m)) return rc;
  const int64_t q = dtype == SGF_BF16 ? 8 : 4;
  const size_t esz = dtype == SGF_BF16 ? 2 : 4;
  SGF_REQUIRE(dw && db, SGF_E_INVALID, "%s: null dw / db", fn);
  SGF_REQUIRE(n == 0 || (dx1 && aligned16(dx1) && ldd1 >= d && ldd1 % q == 0), SGF_E_INVALID,
              "%s: dx1 must be non-null and 16-byte aligned with ldd1 >= d keeping rows aligned", fn);
  SGF_REQUIRE((x2 == nullptr) == (dx2 == nullptr) || n == 0, SGF_E_INVALID, "%s: dx2 goes with x2", fn);
  SGF_REQUIRE(!dx2 || (aligned16(dx2) && ldd2 >= d && ldd2 % q == 0), SGF_E_INVALID,
              "%s: dx2 must be 16-byte aligned with ldd2 >= d keeping rows aligned", fn);
  SGF_REQUIRE(m == 0 || (x1 && w && aligned16(x1) && aligned16(x2)), SGF_E_INVALID,
              "%s: null or unaligned x1 / x2 / w", fn);
  const bool generic = dlogits != nullptr;
  SGF_REQUIRE(m == 0 || generic || (logits && lse && labels && gout), SGF_E_INVALID,
              "%s: pass dlogits, or logits + lse + labels + gout", fn);
  SGF_REQUIRE(m == 0 || (generic ? lddl >= classes : ldl >= classes), SGF_E_INVALID, "%s: leading dimension < classes", fn);
  SGF_REQUIRE(m == 0 || (workspace && workspace_bytes >= sgf_head_rows_bwd_workspace_bytes(m, d, classes)), SGF_E_WORKSPACE,
              "%s: workspace too small", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m == 0) {            // (m > 0: k_hr_dw_sum writes every element of both)
    SGF_CHECK_HIP(hipMemsetAsync(db, 0, static_cast<size_t>(classes) * sizeof(float), st));
    SGF_CHECK_HIP(hipMemsetAsync(dw, 0, static_cast<size_t>(classes) * d * sizeof(float), st));
  }
  if (n == 0) return SGF_OK;
  const bool fill_here = idx == nullptr && m > 0;    // prefix form: zeros streamed by the kernel's own launch
  if (!fill_here) {
    void* const dst[2] = {dx1, dx2};
    const int64_t ldd[2] = {ldd1, ldd2};
    for (int i = 0; i < 2; ++i) {
      if (!dst[i]) continue;
      if (ldd[i] == d)
        SGF_CHECK_HIP(hipMemsetAsync(dst[i], 0, static_cast<size_t>(n) * d * esz, st));
      else
        SGF_CHECK_HIP(hipMemset2DAsync(dst[i], static_cast<size_t>(ldd[i]) * esz, 0, static_cast<size_t>(d) * esz,
                                       static_cast<size_t>(n), st));
    }
  }
  if (m == 0) return SGF_OK;
  const int ntiles = static_cast<int>(hr_tiles(m));
  int zblocks = 0;
  if (fill_here && n > m) {
    const int64_t units = (n - m) * (static_cast<int64_t>(d) * static_cast<int64_t>(esz) / 16);
    int64_t zb = (units + kHrThreads * 4 - 1) / (kHrThreads * 4);
    if (zb > kHrZeroBlocks) zb = kHrZeroBlocks;
    zblocks = static_cast<int>(zb < 1 ? 1 : zb);
  }
  HrBwd p;
  p.w = w, p.idx = idx, p.n = n, p.m = m, p.d = d, p.c = classes, p.a = a, p.b = b;
  p.dlogits = dlogits, p.lddl = lddl, p.logits = logits, p.ldl = ldl, p.lse = lse, p.labels = labels, p.gout = gout;
  p.inv_denom = inv_denom, p.dx1 = dx1, p.ldd1 = ldd1, p.dx2 = dx2, p.ldd2 = ldd2;
  p.g = static_cast<float*>(workspace);
  p.ntiles = ntiles;
  float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                         align_up(static_cast<size_t>(m) * classes * sizeof(float), 256));
  int64_t slice_rows;
  int slices;
  hr_slices(m, slice_rows, slices);
  const dim3 dgrid((classes + kHrDwClasses - 1) / kHrDwClasses, slices);
  const int dthreads = (d + 63) / 64 * 64;
  if (dtype == SGF_BF16) {
    hipLaunchKernelGGL(k_hr_bwd<uint16_t>, dim3(ntiles + zblocks), dim3(kHrThreads), 0, st, p);
    SGF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hr_dw_part<uint16_t>, dgrid, dim3(dthreads), 0, st, static_cast<const uint16_t*>(x1), ld1, a,
                       static_cast<const uint16_t*>(x2), ld2, b, idx, n, m, d, classes, p.g, slice_rows, part);
  } else {
    hipLaunchKernelGGL(k_hr_bwd<float>, dim3(ntiles + zblocks), dim3(kHrThreads), 0, st, p);
    SGF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hr_dw_part<float>, dgrid, dim3(dthreads), 0, st, static_cast<const float*>(x1), ld1, a,
                       static_cast<const float*>(x2), ld2, b, idx, n, m, d, classes, p.g, slice_rows, part);
  }
  SGF_LAUNCH_CHECK();
  const int e = classes * (d + 1);
  hipLaunchKernelGGL(k_hr_dw_sum, dim3((e + kHrThreads - 1) / kHrThreads), dim3(kHrThreads), 0, st, part, slices, d, classes,
                     dw, db);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}
