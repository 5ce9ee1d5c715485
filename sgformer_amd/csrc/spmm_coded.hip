// spmm_coded.hip — the two preparation passes of sgf_spmm_coded (spmm.hip: k_spmm_row_coded): a lossless 12-bit code of the
// bf16 rows of a [n, 256] operand, 384 bytes (3 fetch lines) per row instead of 512 (4), and the CSR values with each source
// row's scale folded in.
//
// The code.  A bf16 value is s | Ek (8 bits) | m (7 bits).  Per row, E = the largest Ek among the finite non-zero elements
// (15 for a row without one); an element is stored as s | e | m with e = Ek - (E - 15) in 1..15, a zero of either sign as
// s | 0 | 0.  Placing e in the LOW four bits of an fp32 exponent field decodes a zero to itself and every other element to
// a normal float of [2^-126, 2^-111): the element is that float times 2^(E - 15), exactly.  The factor is not stored with
// the row — the slot is full — but folded into the CSR value of every entry that reads the row (k_code_values):
// fmaf(v * 2^s, x * 2^-s, acc) is fmaf(v, x, acc) bit for bit while v * 2^s is a normal float (one real product, one
// rounding).  A row ESCAPES (stays dense) when an element is subnormal, Inf or NaN or lies more than 14 binades under the
// row's largest: its scale byte is kCodedEscaped and its slot zero bytes; an entry whose source row escaped, or whose
// scaled value is not a normal float, carries -v instead: the sign bit is the tag (normalised adjacency values are >= 0;
// a stored value with the sign bit set, -0.0 included, is counted in *n_unsupported and the gather then runs the whole
// launch on the dense rows).
//
// The slot (kCodedSlot = 384 bytes, lane l of the gathering wave decodes columns 4l .. 4l+3 from fixed offsets):
//   bytes [0, 256)    dword l:  bits 15..0  s0 | e2 (4) | e0 (4) | m0 (7),  bits 31..16  s1 | e3 | e1 | m1
//   bytes [256, 384)  half  l:  bits  7..0  s2 | m2,  bits 15..8  s3 | m3
// so columns 0 and 1 are two masks of the dword, and columns 2 and 3 one byte permute, one shift and two masks.
#include "common.h"
#include "spmm_shared.h"

namespace sgf {
namespace {

constexpr int kRowsPerWave = 4;     // rows one wave codes, their loads issued together
constexpr int kWaves = 4;

// max over all 64 lanes on the VALU's DPP path, result uniform (the pattern of wave_sum_uniform, common.h: a lane without a
// source takes 0, the identity of an unsigned max)
__device__ __forceinline__ uint32_t wave_max_uniform(uint32_t v) {
  auto dpp = [](uint32_t x, auto ctrl, auto row_mask) {
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), decltype(ctrl)::value,
                                                             decltype(row_mask)::value, 0xf, false));
  };
  auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  v = mx(v, dpp(v, std::integral_constant<int, 0x111>{}, std::integral_constant<int, 0xf>{}));
  v = mx(v, dpp(v, std::integral_constant<int, 0x112>{}, std::integral_constant<int, 0xf>{}));
  v = mx(v, dpp(v, std::integral_constant<int, 0x114>{}, std::integral_constant<int, 0xf>{}));
  v = mx(v, dpp(v, std::integral_constant<int, 0x118>{}, std::integral_constant<int, 0xf>{}));
  v = mx(v, dpp(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xa>{}));
  v = mx(v, dpp(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xc>{}));
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}

__global__ __launch_bounds__(kWaves * 64) void k_code_rows(const uint16_t* __restrict__ x, int64_t ldx, int64_t n,
                                                           uint8_t* __restrict__ coded, uint8_t* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = (static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6)) * kRowsPerWave;
  if (r0 >= n) return;
  uint2 raw[kRowsPerWave];
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    const int64_t r = r0 + k < n ? r0 + k : n - 1;       // (clamped: the ragged last wave re-reads the last row)
    raw[k] = *reinterpret_cast<const uint2*>(x + r * ldx + lane * 4);
  }
#pragma unroll
  for (int k = 0; k < kRowsPerWave; ++k) {
    if (r0 + k >= n) break;                              // wave-uniform
    const uint32_t b[4] = {raw[k].x & 0xffffu, raw[k].x >> 16, raw[k].y & 0xffffu, raw[k].y >> 16};
    uint32_t ek[4], hi = 0, bad = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ek[j] = (b[j] >> 7) & 0xffu;
      bad |= (ek[j] == 255u) | ((ek[j] == 0u) & ((b[j] & 0x7fu) != 0u));
      hi = ek[j] > hi ? ek[j] : hi;
    }
    const uint32_t top = wave_max_uniform(hi);           // 0: the row has no normal element
    const uint32_t E = top != 0u ? top : 15u;
#pragma unroll
    for (int j = 0; j < 4; ++j) bad |= (ek[j] != 0u) & (ek[j] + 14u < E);   // more than 14 binades under the largest
    const bool esc = __ballot(bad != 0) != 0;
    uint32_t w = 0, h = 0;
    if (!esc) {
      uint32_t c[4], e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = ek[j] != 0u ? ek[j] + 15u - E : 0u;
        c[j] = (b[j] & 0x807fu) | (e[j] << 7);
      }
      w = c[0] | (e[2] << 11) | ((c[1] | (e[3] << 11)) << 16);
      h = ((b[2] >> 8) & 0x80u) | (b[2] & 0x7fu) | ((((b[3] >> 8) & 0x80u) | (b[3] & 0x7fu)) << 8);
    }
    uint8_t* slot = coded + (r0 + k) * kCodedSlot;
    reinterpret_cast<uint32_t*>(slot)[lane] = w;
    reinterpret_cast<uint16_t*>(slot + 256)[lane] = static_cast<uint16_t>(h);
    if (lane == 0) scale[r0 + k] = esc ? kCodedEscaped : static_cast<uint8_t>(E);
  }
}

// The number of escaped rows, from the scale bytes: one atomic per block of 4096 rows.  (Counted by the coding kernel itself,
// one atomic per wave with an escaped row, the 60 000 same-address atomics of a products-size Gaussian operand took as long
// as the rest of the pass: 0.76 ms against 0.40 ms for an operand with a tenth of the escapes.)
constexpr int kCountBytesPerThread = 16;

__global__ __launch_bounds__(256) void k_count_escaped(const uint8_t* __restrict__ scale, int64_t n, int32_t* __restrict__ n_escaped) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * kCountBytesPerThread;
  int cnt = 0;
  if (i + kCountBytesPerThread <= n) {
    const uint4 q = *reinterpret_cast<const uint4*>(scale + i);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 4; ++b) cnt += ((w[j] >> (8 * b)) & 0xffu) == kCodedEscaped;
  } else {
    for (int64_t j = i; j < n; ++j) cnt += scale[j] == kCodedEscaped;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  __shared__ int part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = part[0] + part[1] + part[2] + part[3];
    if (total) atomicAdd(n_escaped, total);
  }
}

// val' of one stored entry: val * 2^(E - 15) as an exponent-field addition when val is a normal float > 0, the source row
// is coded and the result is a normal float; else -val, the escape tag (val == 0 becomes -0.0)
__device__ __forceinline__ float code_value(float v, uint32_t E) {
  const uint32_t u = __float_as_uint(v);
  const int ev = static_cast<int>((u >> 23) & 0xffu);
  const int en = ev + static_cast<int>(E) - 15;
  const bool ok = (u >> 31) == 0u && ev >= 1 && ev <= 254 && E != kCodedEscaped && en >= 1 && en <= 254;
  return ok ? __uint_as_float((u & 0x807fffffu) | (static_cast<uint32_t>(en) << 23)) : __uint_as_float(u ^ 0x80000000u);
}

// a stored value the tag cannot mark: its sign bit is set already (any negative value, -0.0, a NaN with the sign bit)
__device__ __forceinline__ int signbit32(float v) { return static_cast<int>(__float_as_uint(v) >> 31); }

constexpr int kValuesPerThread = 4;

__global__ __launch_bounds__(256) void k_code_values(const int32_t* __restrict__ colind, const float* __restrict__ val,
                                                     int64_t nnz, const uint8_t* __restrict__ scale,
                                                     float* __restrict__ val_coded, int32_t* __restrict__ n_unsupported) {
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * kValuesPerThread;
  int neg = 0;
  if (i + kValuesPerThread <= nnz) {
    const int4 c = *reinterpret_cast<const int4*>(colind + i);
    const float4 v = *reinterpret_cast<const float4*>(val + i);
    const uint32_t e0 = scale[c.x], e1 = scale[c.y], e2 = scale[c.z], e3 = scale[c.w];
    float4 o;
    o.x = code_value(v.x, e0);
    o.y = code_value(v.y, e1);
    o.z = code_value(v.z, e2);
    o.w = code_value(v.w, e3);
    *reinterpret_cast<float4*>(val_coded + i) = o;
    neg = signbit32(v.x) + signbit32(v.y) + signbit32(v.z) + signbit32(v.w);
  } else {
    for (int64_t j = i; j < nnz; ++j) {
      const float v = val[j];
      val_coded[j] = code_value(v, scale[colind[j]]);
      neg += signbit32(v);
    }
  }
  // (every lane reaches this point: threads past the end carry neg = 0)
  const unsigned long long any = __ballot(neg != 0);
  if (any) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) neg += __shfl_xor(neg, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(n_unsupported, neg);
  }
}

}  // namespace
}  // namespace sgf

using namespace sgf;

extern "C" size_t sgf_spmm_coded_bytes(int64_t n) {
  if (n < 0) return 0;
  return static_cast<size_t>(n) * kCodedSlot;      // (every load of the gather stays inside its slot: no tail)
}

extern "C" int sgf_spmm_code_rows(const void* x, int64_t ldx, int64_t n, void* coded, uint8_t* scale_u8, int32_t* n_escaped,
                                  void* stream) {
  const char* fn = "sgf_spmm_code_rows";
  SGF_REQUIRE(n >= 0, SGF_E_INVALID, "%s: negative size", fn);
  SGF_REQUIRE(n_escaped, SGF_E_INVALID, "%s: null pointer", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    SGF_CHECK_HIP(hipMemsetAsync(n_escaped, 0, sizeof(int32_t), st));
    return SGF_OK;
  }
  SGF_REQUIRE(x && coded && scale_u8, SGF_E_INVALID, "%s: null pointer", fn);
  SGF_REQUIRE(ldx >= 256 && ldx % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 8 == 0, SGF_E_INVALID,
              "%s: bf16 rows of 256 columns, ldx a multiple of 4, x 8-byte aligned (ldx=%lld)", fn,
              static_cast<long long>(ldx));
  SGF_REQUIRE(reinterpret_cast<uintptr_t>(coded) % 128 == 0, SGF_E_INVALID, "%s: the coded buffer must be 128-byte aligned", fn);
  SGF_REQUIRE(reinterpret_cast<uintptr_t>(scale_u8) % 16 == 0, SGF_E_INVALID, "%s: scale_u8 must be 16-byte aligned", fn);
  constexpr int64_t rows_per_block = kWaves * kRowsPerWave;
  const int64_t nb = (n + rows_per_block - 1) / rows_per_block;
  SGF_REQUIRE(nb < (static_cast<int64_t>(1) << 31), SGF_E_UNSUPPORTED, "%s: n too large for one launch", fn);
  SGF_CHECK_HIP(hipMemsetAsync(n_escaped, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(k_code_rows, dim3(static_cast<unsigned>(nb)), dim3(kWaves * 64), 0, st, static_cast<const uint16_t*>(x),
                     ldx, n, static_cast<uint8_t*>(coded), scale_u8);
  SGF_LAUNCH_CHECK();
  constexpr int64_t count_per_block = 256 * kCountBytesPerThread;
  hipLaunchKernelGGL(k_count_escaped, dim3(static_cast<unsigned>((n + count_per_block - 1) / count_per_block)), dim3(256), 0, st,
                     scale_u8, n, n_escaped);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}

extern "C" int sgf_spmm_code_values(const int32_t* colind, const float* val, int64_t nnz, const uint8_t* scale_u8,
                                    float* val_coded, int32_t* n_unsupported, void* stream) {
  const char* fn = "sgf_spmm_code_values";
  SGF_REQUIRE(nnz >= 0, SGF_E_INVALID, "%s: negative size", fn);
  SGF_REQUIRE(n_unsupported, SGF_E_INVALID, "%s: null pointer", fn);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SGF_REQUIRE(nnz == 0 || (colind && val && scale_u8 && val_coded), SGF_E_INVALID, "%s: null pointer", fn);
  SGF_REQUIRE(reinterpret_cast<uintptr_t>(colind) % 16 == 0 && reinterpret_cast<uintptr_t>(val) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(val_coded) % 16 == 0,
              SGF_E_INVALID, "%s: colind, val and val_coded must be 16-byte aligned", fn);
  constexpr int64_t per_block = 256 * kValuesPerThread;
  const int64_t nb = (nnz + per_block - 1) / per_block;
  SGF_REQUIRE(nb < (static_cast<int64_t>(1) << 31), SGF_E_UNSUPPORTED, "%s: nnz too large for one launch", fn);
  SGF_CHECK_HIP(hipMemsetAsync(n_unsupported, 0, sizeof(int32_t), st));
  if (nnz == 0) return SGF_OK;
  hipLaunchKernelGGL(k_code_values, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, colind, val, nnz, scale_u8, val_coded,
                     n_unsupported);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}
