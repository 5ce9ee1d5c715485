// bce.hip — N4b: BCEWithLogitsLoss on the training rows (large/main.py:130-137, large/main-batch.py:101-105,
// medium/main.py:158-166), forward and backward in one pass each.
//
// The selected rows form an [m, c] matrix; its elements are numbered p = j * c + k and handed out to threads in
// lane-consecutive order (thread t of a block chunk takes unit t), so the lanes of a wave run ALONG a row: a 112-column
// fp32 row is read by 28 consecutive lanes with 16-byte loads, and for c = 2 one wave has 32 gathered rows in flight (as
// k_nll_fwd16 keeps several: one row per wave waits a full random-row latency per row).  The dense form (idx == NULL) is
// the same kernel with r = j — a streaming pass — which also makes it equal to the row form with idx = 0..n-1 bit for bit.
// A unit is 4 consecutive columns when c % 4 == 0 and every operand is aligned for it (16-byte accesses on fp32), else
// one element.  Deterministic: every thread adds its units in a fixed order, a block adds its threads in a fixed tree,
// one wave adds the block partials in a fixed order.  expf / log1pf (no fast intrinsics), fp32 throughout.
#include "common.h"

namespace sgf {
namespace {

constexpr int kThreads = 256;
constexpr int kBceMaxBlocks = 2048;  // 8 blocks per CU

// unit u of the selected [m, c] matrix -> (selected row j, unit within the row); 32-bit division where the count allows
__device__ __forceinline__ void split_unit(int64_t u, int per_row, bool small, int64_t& j, int& q) {
  if (small) {
    const uint32_t jj = static_cast<uint32_t>(u) / static_cast<uint32_t>(per_row);
    j = jj;
    q = static_cast<int>(static_cast<uint32_t>(u) - jj * static_cast<uint32_t>(per_row));
  } else {
    j = u / per_row;
    q = static_cast<int>(u - j * per_row);
  }
}

// target kinds (include/sgf.h): fp32 [n, c], int64 0/1 [n, c], int64 class index [n] (one-hot row formed here; an index
// outside [0, c) equals no column k, so the row is all zero — it is only ever COMPARED, never used as an address)
template <int TK>
__device__ __forceinline__ float target1(const void* __restrict__ tgt, int64_t ldt, int64_t r, int k) {
  if constexpr (TK == SGF_BCE_TARGET_F32) {
    return static_cast<const float*>(tgt)[r * ldt + k];
  } else if constexpr (TK == SGF_BCE_TARGET_I64) {
    return static_cast<float>(static_cast<const int64_t*>(tgt)[r * ldt + k]);
  } else {
    return static_cast<const int64_t*>(tgt)[r] == static_cast<int64_t>(k) ? 1.f : 0.f;
  }
}

template <int TK, int W>
__device__ __forceinline__ void target_unit(const void* __restrict__ tgt, int64_t ldt, int64_t r, int k, float (&t)[W]) {
  if constexpr (W == 1) {
    t[0] = target1<TK>(tgt, ldt, r, k);
  } else if constexpr (TK == SGF_BCE_TARGET_F32) {
    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(tgt) + r * ldt + k);
    t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
  } else if constexpr (TK == SGF_BCE_TARGET_I64) {
    const longlong2* p = reinterpret_cast<const longlong2*>(static_cast<const int64_t*>(tgt) + r * ldt + k);
    const longlong2 a = p[0], b = p[1];
    t[0] = static_cast<float>(a.x), t[1] = static_cast<float>(a.y);
    t[2] = static_cast<float>(b.x), t[3] = static_cast<float>(b.y);
  } else {
    const int64_t y = static_cast<const int64_t*>(tgt)[r];
#pragma unroll
    for (int w = 0; w < W; ++w) t[w] = y == static_cast<int64_t>(k + w) ? 1.f : 0.f;
  }
}

template <typename T, int W>
__device__ __forceinline__ void logits_unit(const T* __restrict__ p, float (&x)[W]) {
  if constexpr (W == 1) {
    x[0] = load1<T>(p);
  } else {
    const float4 v = load4<T>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  }
}

// l(x, t) = max(x, 0) - x t + log1p(exp(-|x|)): no overflow for any finite x (exp's argument is <= 0)
__device__ __forceinline__ float bce_term(float x, float t) {
  return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}
// sigmoid(x) - t with z = exp(-|x|) <= 1: 1 / (1 + z) for x >= 0, z / (1 + z) below — saturates to 1 and to 0 cleanly
__device__ __forceinline__ float bce_grad(float x, float t) {
  const float z = expf(-fabsf(x));
  return (x >= 0.f ? 1.f : z) / (1.f + z) - t;
}

// part[blk] = sum of l over this block's units.  Unit (i * gridDim + blk) * 256 + tid in round i: lane-consecutive.
template <typename T, int TK, int W>
__global__ __launch_bounds__(kThreads) void k_bce_fwd(const T* __restrict__ logits, int64_t ldl, int c,
                                                      const void* __restrict__ tgt, int64_t ldt,
                                                      const int64_t* __restrict__ idx, int64_t units, bool small,
                                                      float* __restrict__ part) {
  constexpr int U = W == 4 ? 2 : 4;  // units whose loads are issued before the first exp
  __shared__ float red[kThreads / 64];
  const int per_row = c / W;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t rounds = (units + step * U - 1) / (step * U);
  float acc = 0.f;
  for (int64_t i = 0; i < rounds; ++i) {
    float x[U][W], t[U][W];
    bool ok[U];
#pragma unroll
    for (int e = 0; e < U; ++e) {
      const int64_t u = (i * U + e) * step + first;
      ok[e] = u < units;
      if (ok[e]) {
        int64_t j;
        int q;
        split_unit(u, per_row, small, j, q);
        const int64_t r = idx ? idx[j] : j;
        logits_unit<T, W>(logits + r * ldl + q * W, x[e]);
        target_unit<TK, W>(tgt, ldt, r, q * W, t[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < U; ++e) {
      if (ok[e]) {
#pragma unroll
        for (int w = 0; w < W; ++w) acc += bce_term(x[e][w], t[e][w]);
      }
    }
  }
  acc = group_sum<64>(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w];
    part[blockIdx.x] = s;
  }
}

// one wave: lane l adds partials l, l + 64, ... in order, then a fixed shuffle tree; the sum is scaled once on the way out
__global__ void k_bce_sum(const float* __restrict__ part, int nblk, float inv_denom, float* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 64) s += part[b];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) out[0] = s * inv_denom;
}

// dlogits[r, k] = scale * (sigmoid(x) - t) on the selected rows (the other rows were zeroed by the caller)
template <typename T, int TK, int W>
__global__ __launch_bounds__(kThreads) void k_bce_bwd(const T* __restrict__ logits, int64_t ldl, int c,
                                                      const void* __restrict__ tgt, int64_t ldt,
                                                      const int64_t* __restrict__ idx, int64_t units, bool small,
                                                      const float* __restrict__ gout, float inv_denom,
                                                      T* __restrict__ dlogits, int64_t ldd) {
  constexpr int U = W == 4 ? 2 : 4;
  const int per_row = c / W;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t rounds = (units + step * U - 1) / (step * U);
  const float scale = gout[0] * inv_denom;
  for (int64_t i = 0; i < rounds; ++i) {
    float x[U][W], t[U][W];
    int64_t at[U];
    bool ok[U];
#pragma unroll
    for (int e = 0; e < U; ++e) {
      const int64_t u = (i * U + e) * step + first;
      ok[e] = u < units;
      if (ok[e]) {
        int64_t j;
        int q;
        split_unit(u, per_row, small, j, q);
        const int64_t r = idx ? idx[j] : j;
        logits_unit<T, W>(logits + r * ldl + q * W, x[e]);
        target_unit<TK, W>(tgt, ldt, r, q * W, t[e]);
        at[e] = r * ldd + q * W;
      }
    }
#pragma unroll
    for (int e = 0; e < U; ++e) {
      if (ok[e]) {
        if constexpr (W == 4) {
          float4 g;
          g.x = scale * bce_grad(x[e][0], t[e][0]);
          g.y = scale * bce_grad(x[e][1], t[e][1]);
          g.z = scale * bce_grad(x[e][2], t[e][2]);
          g.w = scale * bce_grad(x[e][3], t[e][3]);
          store4<T>(dlogits + at[e], g);
        } else {
          store1<T>(dlogits + at[e], scale * bce_grad(x[e][0], t[e][0]));
        }
      }
    }
  }
}

inline bool aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// 4-column units: every row of every operand starts on a 4-element boundary of its own type
inline bool quad_ok(int c, int dtype, const void* logits, int64_t ldl, const void* tgt, int64_t ldt, int target_kind) {
  const size_t esz = dtype == SGF_BF16 ? 2 : 4;
  if (c % 4 != 0 || ldl % 4 != 0 || !aligned(logits, 4 * esz)) return false;
  if (target_kind == SGF_BCE_TARGET_CLASS) return true;
  return ldt % 4 == 0 && aligned(tgt, 16);
}

inline int bce_blocks(int64_t units, int w) {
  const int64_t per_block = static_cast<int64_t>(kThreads) * (w == 4 ? 2 : 4);
  int64_t b = (units + per_block - 1) / per_block;
  if (b > kBceMaxBlocks) b = kBceMaxBlocks;
  if (b < 1) b = 1;
  return static_cast<int>(b);
}

int check_bce(const char* fn, int64_t ldl, int64_t n, int c, int dtype, int64_t ldt, int target_kind, const int64_t* idx,
              int64_t m) {
  SGF_REQUIRE(n >= 0 && m >= 0 && m <= n && c >= 1 && ldl >= c, SGF_E_INVALID,
              "%s: bad sizes n=%lld m=%lld c=%d ldl=%lld", fn, static_cast<long long>(n), static_cast<long long>(m), c,
              static_cast<long long>(ldl));
  SGF_REQUIRE(dtype == SGF_F32 || dtype == SGF_BF16, SGF_E_INVALID, "%s: unknown dtype %d", fn, dtype);
  SGF_REQUIRE(target_kind == SGF_BCE_TARGET_F32 || target_kind == SGF_BCE_TARGET_I64 ||
                  target_kind == SGF_BCE_TARGET_CLASS,
              SGF_E_INVALID, "%s: unknown target_kind %d", fn, target_kind);
  SGF_REQUIRE(target_kind == SGF_BCE_TARGET_CLASS || ldt >= c, SGF_E_INVALID, "%s: ldt=%lld < c=%d", fn,
              static_cast<long long>(ldt), c);
  // (m == 0 with idx == NULL: an empty index vector has no address)
  SGF_REQUIRE(idx || m == n || m == 0, SGF_E_INVALID, "%s: the dense form (idx == NULL) needs m == n (m=%lld n=%lld)", fn,
              static_cast<long long>(m), static_cast<long long>(n));
  return SGF_OK;
}

}  // namespace
}  // namespace sgf

using namespace sgf;

extern "C" size_t sgf_bce_workspace_bytes(int64_t m, int32_t c) {
  (void)m;
  (void)c;
  return static_cast<size_t>(kBceMaxBlocks) * sizeof(float);
}

#define SGF_BCE_KIND(KERNEL, T, W, ...)                                                                   \
  do {                                                                                                    \
    if (target_kind == SGF_BCE_TARGET_F32)                                                                \
      hipLaunchKernelGGL((KERNEL<T, SGF_BCE_TARGET_F32, W>), dim3(nblk), dim3(kThreads), 0, st, __VA_ARGS__);   \
    else if (target_kind == SGF_BCE_TARGET_I64)                                                           \
      hipLaunchKernelGGL((KERNEL<T, SGF_BCE_TARGET_I64, W>), dim3(nblk), dim3(kThreads), 0, st, __VA_ARGS__);   \
    else                                                                                                  \
      hipLaunchKernelGGL((KERNEL<T, SGF_BCE_TARGET_CLASS, W>), dim3(nblk), dim3(kThreads), 0, st, __VA_ARGS__); \
  } while (0)

extern "C" int sgf_bce_fwd(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* target,
                           int64_t ldt, int32_t target_kind, const int64_t* idx, int64_t m, float inv_denom,
                           float* loss_sum, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_bce("sgf_bce_fwd", ldl, n, c, dtype, ldt, target_kind, idx, m)) return rc;
  SGF_REQUIRE(loss_sum, SGF_E_INVALID, "sgf_bce_fwd: null loss_sum");
  SGF_REQUIRE(m == 0 || (logits && target), SGF_E_INVALID, "sgf_bce_fwd: null pointer");
  SGF_REQUIRE(m == 0 || (workspace && workspace_bytes >= sgf_bce_workspace_bytes(m, c)), SGF_E_WORKSPACE,
              "sgf_bce_fwd: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m == 0) {
    SGF_CHECK_HIP(hipMemsetAsync(loss_sum, 0, sizeof(float), st));
    return SGF_OK;
  }
  const bool quad = quad_ok(c, dtype, logits, ldl, target, ldt, target_kind);
  const int64_t units = m * (quad ? c / 4 : c);
  const bool small = units < (static_cast<int64_t>(1) << 31);
  const int nblk = bce_blocks(units, quad ? 4 : 1);
  float* part = static_cast<float*>(workspace);
  if (dtype == SGF_F32) {
    const float* lg = static_cast<const float*>(logits);
    if (quad)
      SGF_BCE_KIND(k_bce_fwd, float, 4, lg, ldl, c, target, ldt, idx, units, small, part);
    else
      SGF_BCE_KIND(k_bce_fwd, float, 1, lg, ldl, c, target, ldt, idx, units, small, part);
  } else {
    const uint16_t* lg = static_cast<const uint16_t*>(logits);
    if (quad)
      SGF_BCE_KIND(k_bce_fwd, uint16_t, 4, lg, ldl, c, target, ldt, idx, units, small, part);
    else
      SGF_BCE_KIND(k_bce_fwd, uint16_t, 1, lg, ldl, c, target, ldt, idx, units, small, part);
  }
  SGF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_bce_sum, dim3(1), dim3(64), 0, st, part, nblk, inv_denom, loss_sum);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}

extern "C" int sgf_bce_bwd(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* target,
                           int64_t ldt, int32_t target_kind, const int64_t* idx, int64_t m, const float* gout,
                           float inv_denom, void* dlogits, int64_t ldd, void* stream) {
  if (int rc = check_bce("sgf_bce_bwd", ldl, n, c, dtype, ldt, target_kind, idx, m)) return rc;
  SGF_REQUIRE(ldd >= c, SGF_E_INVALID, "sgf_bce_bwd: ldd=%lld < c=%d", static_cast<long long>(ldd), c);
  SGF_REQUIRE(n == 0 || (dlogits && gout), SGF_E_INVALID, "sgf_bce_bwd: null pointer");
  SGF_REQUIRE(m == 0 || (logits && target), SGF_E_INVALID, "sgf_bce_bwd: null pointer");
  if (n == 0) return SGF_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t esz = dtype == SGF_BF16 ? 2 : 4;
  if (idx || m == 0) {  // (the dense form writes every row itself)
    if (ldd == c)
      SGF_CHECK_HIP(hipMemsetAsync(dlogits, 0, static_cast<size_t>(n) * c * esz, st));
    else
      SGF_CHECK_HIP(hipMemset2DAsync(dlogits, static_cast<size_t>(ldd) * esz, 0, static_cast<size_t>(c) * esz,
                                     static_cast<size_t>(n), st));
  }
  if (m == 0) return SGF_OK;
  const bool quad = quad_ok(c, dtype, logits, ldl, target, ldt, target_kind) && ldd % 4 == 0 && aligned(dlogits, 4 * esz);
  const int64_t units = m * (quad ? c / 4 : c);
  const bool small = units < (static_cast<int64_t>(1) << 31);
  const int nblk = bce_blocks(units, quad ? 4 : 1);
  if (dtype == SGF_F32) {
    const float* lg = static_cast<const float*>(logits);
    float* dl = static_cast<float*>(dlogits);
    if (quad)
      SGF_BCE_KIND(k_bce_bwd, float, 4, lg, ldl, c, target, ldt, idx, units, small, gout, inv_denom, dl, ldd);
    else
      SGF_BCE_KIND(k_bce_bwd, float, 1, lg, ldl, c, target, ldt, idx, units, small, gout, inv_denom, dl, ldd);
  } else {
    const uint16_t* lg = static_cast<const uint16_t*>(logits);
    uint16_t* dl = static_cast<uint16_t*>(dlogits);
    if (quad)
      SGF_BCE_KIND(k_bce_bwd, uint16_t, 4, lg, ldl, c, target, ldt, idx, units, small, gout, inv_denom, dl, ldd);
    else
      SGF_BCE_KIND(k_bce_bwd, uint16_t, 1, lg, ldl, c, target, ldt, idx, units, small, gout, inv_denom, dl, ldd);
  }
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}
