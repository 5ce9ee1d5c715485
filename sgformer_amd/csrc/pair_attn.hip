// pair_attn.hip — DIFFormer's all-pair sigmoid attention (medium/difformer.py:41-52, kernel='sigmoid') without the
// n x l score tensor (include/sgf.h block N7).  With z = q_i . k_j and S = sigmoid(z), per head:
//
//   sgf_pair_sigmoid_fwd    : r_i = sum_j S,  out_i = sum_j S v_j / r_i
//   sgf_pair_sigmoid_bwd_q  : delta_i = g_i . out_i,  dZ = S (1 - S) (g_i . v_j - delta_i) / r_i,  dq_i = sum_j dZ k_j
//   sgf_pair_sigmoid_bwd_kv : dv_j = sum_i (S / r_i) g_i,  dk_j = sum_i dZ q_i
//
// The scores are bounded, so there is no running maximum and no rescale: a flash-style sweep with plain sums.
//
// gfx950 mapping.  A workgroup is 4 waves; it keeps 128 rows resident (32 per wave: queries in fwd / bwd_q, keys in
// bwd_kv) and sweeps the other side in LDS tiles that all four waves share.  Nothing is summed across workgroups: no
// atomics, no hand-off, every result is a fixed-order sum (bwd_q and bwd_kv both recompute S: seven products, not five).
//   * The first products (z, and g . v in the backward) put the RESIDENT row on the MFMA lane and the swept row in the 16
//     accumulator registers: X[swept][resident].  The second products sum over the swept row, which is X's row index, so
//     the accumulator tile is the next MFMA's B operand as it stands (no lane movement, no LDS round trip): per lane the
//     row constants r_i / delta_i are scalars (fwd, bwd_q) or two LDS broadcasts per register (bwd_kv).
//   * bf16 storage: v_mfma_f32_32x32x16_bf16.  Registers 8s .. 8s+7 of X, converted pairwise, are k-step s of the B
//     operand; element j of lane half h is then X's row 16s + 8(j>>2) + 4h + (j&3).  The swept rows are assigned to X's rows
//     with bits 2 and 3 swapped (swap23), which makes that k order the natural one: the A operand of the second product
//     is one 16-byte read of a transposed LDS image [feature][swept row].  The tile is staged twice, row-major for the
//     first product and transposed for the second.
//   * fp32 storage: v_mfma_f32_32x32x2_f32 (exact fp32 products, one operand register per lane): register q of X is the B
//     operand of one MFMA whose two k are X's rows of the two lane halves; the A operand is a 4-byte read of the
//     row-major image, so one image serves both products.  S and dZ are used unrounded.
//   * fp32 storage under SGF_F32_BF16X3 (the sgf_pair_*_x3_* entries, block N9; arm tag f32x3): the bf16 arm's MFMA, layouts and
//     swap23 order on operands split as a = hi + lo in bf16, three products per product into one fp32 accumulator; the swept
//     tile is split once as it is staged (two bf16 planes per image), the resident rows once into two fragment sets, X as it
//     becomes the B operand.  expf, maxima, row sums, lse and delta are the fp32 arm's; the sums are over the unrounded weights.
//   * sigmoid: u = exp(-z), S = 1 / (1 + u) in fp32.  z >= 17: 1 + u rounds to 1, S = 1.  z <= -88.8: u = inf, S = 0 (no
//     NaN: nothing is multiplied by u).  1 - S is formed from S, so a saturated score has an exactly zero derivative.
//   * tails: a swept row past the end is staged as zeros AND masked (a zero key would score sigmoid(0) = 0.5): keys by a
//     compare on the row index, queries (bwd_kv) by a staged 1 / r = 0.  Resident rows past the end are clamped for the
//     loads and never stored.
//
// The exact softmax attention (block N8) is the second arm of this file: its forward (k_ps_fwd) is the same skeleton with
// an online maximum, and its comment stands in front of it.  The two backward kernels (k_pair_bwd_q, k_pair_bwd_kv) serve
// both arms: what differs between them is a score policy (SigmoidScore, SoftmaxScore).
#include "common.h"

namespace sgf {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kPaThreads = 256;                  // 4 waves
constexpr int kPaRows = 32 * (kPaThreads / 64);  // resident rows per workgroup

struct PaArgs {
  const void *q, *k, *v, *g, *o;   // o: the forward's out (bwd_q)
  int64_t ldq, ldk, ldv, ldg, ldo;
  void *out, *dq, *dk, *dv;
  int64_t ldout, lddq, lddk, lddv;
  float* rowsum;                   // [n, heads]: written by fwd, read by the backward (the softmax arm: lse)
  float* delta;                    // [n, heads]: written by bwd_q, read by bwd_kv
  int64_t n, l;
  int heads, v_heads;
};

__device__ __forceinline__ int swap23(int r) { return (r & 0x13) | ((r & 4) << 1) | ((r & 8) >> 1); }
// swept row (inside a 32-row sub-tile) that register q of lane half hh holds: swap23 of the MFMA's C/D row
__device__ __forceinline__ int slot_of(int q, int hh) { return (q & 3) + 4 * ((q >> 2) & 1) + 8 * hh + 16 * (q >> 3); }

__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const f32x2_t v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));   // v_cvt_pk_bf16_f32, round to nearest even
}

// S = sigmoid(z).  fp32 storage: expf; bf16 storage: the hardware exp2 (S is rounded to 8 bits right after)
template <bool kExact>
__device__ __forceinline__ float sigmoid(float z) {
  const float u = kExact ? expf(-z) : __builtin_amdgcn_exp2f(-1.44269504088896341f * z);
  return __builtin_amdgcn_rcpf(1.0f + u);
}

// The arm of a kernel: its storage type (uint16_t: bf16, float: fp32 with exact fp32 products), or f32x3: fp32 storage whose
// matrix products are three bf16 matrix-core products (SGF_F32_BF16X3; the comment in front of PaImg's f32x3 members).
struct f32x3 {};
template <typename A>
struct pa_elem { using type = A; };
template <>
struct pa_elem<f32x3> { using type = float; };

// the resident row's fragments of the f32x3 arm: the two bf16 terms of a = hi + lo
struct PaSplitFrag {
  bf16x8 hi, lo;
};

// One swept tile of SW rows x D features in LDS: `rm` row-major (pitch D + pad), `tr` transposed [feature][row] (bf16 and
// f32x3).
//
// f32x3: every fp32 element is split once while the tile is staged, hi = bf16_rne(a), lo = bf16_rne(a - hi), lo = 0 where hi
// is not finite (common.h split_bf16x2), into two bf16 images (the `hi` plane, then the `lo` plane) in the bf16 arm's
// layouts; the resident rows are split the same way into two fragment sets, and the accumulator tile of the second products
// (S, P, dZ, W: fp32 in registers) is split as it becomes the B operand.  Every product is hi.hi + hi.lo + lo.hi on
// v_mfma_f32_32x32x16_bf16 into one fp32 accumulator: the dropped lo.lo term is below 2^-16 of |a| |b|.  Everything that
// is not a matrix product (exp, maxima, row sums, lse, delta) is the fp32 arm's code.
template <typename A, int D, int SW>
struct PaImg {
  using T = typename pa_elem<A>::type;               // storage
  static constexpr bool kBf16 = std::is_same<A, uint16_t>::value;
  static constexpr bool kX3 = std::is_same<A, f32x3>::value;
  static constexpr bool kTrans = kBf16 || kX3;       // bf16 matrix cores: the second products read the transposed image
  using L = typename std::conditional<kTrans, uint16_t, float>::type;   // LDS element
  static constexpr int kVec = 16 / static_cast<int>(sizeof(T));
  static constexpr int kPitch = D + (kTrans ? 8 : 4);
  static constexpr int kPitchT = SW + 8;
  static constexpr int kRmPlane = SW * kPitch;
  static constexpr int kTrPlane = D * kPitchT;
  static constexpr int kRm = (kX3 ? 2 : 1) * kRmPlane;
  static constexpr int kTr = kTrans ? (kX3 ? 2 : 1) * kTrPlane : 4;
  static constexpr int kFrags = kTrans ? D / 16 : D / 2;
  using Frag = typename std::conditional<kX3, PaSplitFrag, typename std::conditional<kBf16, bf16x8, float>::type>::type;

  // rows row0 .. row0 + SW - 1 of src (already at the head's first column); rows >= nrows are zeros
  template <bool RM, bool TR>
  static __device__ __forceinline__ void stage(const T* __restrict__ src, int64_t ld, int64_t row0, int64_t nrows, L* rm,
                                               L* tr) {
    constexpr int CH = D / kVec;
    for (int idx = threadIdx.x; idx < SW * CH; idx += kPaThreads) {
      const int row = idx % SW, c = idx / SW;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row0 + row < nrows) v = *reinterpret_cast<const uint4*>(src + (row0 + row) * ld + kVec * c);
      if constexpr (kX3) {
        uint2 h, l;
        split_bf16x2(__uint_as_float(v.x), __uint_as_float(v.y), h.x, l.x);
        split_bf16x2(__uint_as_float(v.z), __uint_as_float(v.w), h.y, l.y);
        if constexpr (RM) {
          *reinterpret_cast<uint2*>(rm + row * kPitch + 4 * c) = h;
          *reinterpret_cast<uint2*>(rm + kRmPlane + row * kPitch + 4 * c) = l;
        }
        if constexpr (TR) {
          const uint32_t wh[2] = {h.x, h.y}, wl[2] = {l.x, l.y};
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            tr[(4 * c + 2 * e) * kPitchT + row] = static_cast<L>(wh[e] & 0xffffu);
            tr[(4 * c + 2 * e + 1) * kPitchT + row] = static_cast<L>(wh[e] >> 16);
            tr[kTrPlane + (4 * c + 2 * e) * kPitchT + row] = static_cast<L>(wl[e] & 0xffffu);
            tr[kTrPlane + (4 * c + 2 * e + 1) * kPitchT + row] = static_cast<L>(wl[e] >> 16);
          }
        }
      } else {
        if constexpr (RM) *reinterpret_cast<uint4*>(rm + row * kPitch + kVec * c) = v;
        if constexpr (TR && kBf16) {
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            tr[(8 * c + 2 * e) * kPitchT + row] = static_cast<T>(w[e] & 0xffffu);
            tr[(8 * c + 2 * e + 1) * kPitchT + row] = static_cast<T>(w[e] >> 16);
          }
        }
      }
    }
  }

  // the resident row's fragments (B operand of the first products): row points at the head's first column of that row
  static __device__ __forceinline__ void load_frags(const T* __restrict__ row, int hh, Frag* f) {
    if constexpr (kX3) {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) {
        const float4 a = *reinterpret_cast<const float4*>(row + 16 * s + 8 * hh);
        const float4 b = *reinterpret_cast<const float4*>(row + 16 * s + 8 * hh + 4);
        union {
          bf16x8 v;
          uint32_t u[4];
        } h, l;
        split_bf16x2(a.x, a.y, h.u[0], l.u[0]);
        split_bf16x2(a.z, a.w, h.u[1], l.u[1]);
        split_bf16x2(b.x, b.y, h.u[2], l.u[2]);
        split_bf16x2(b.z, b.w, h.u[3], l.u[3]);
        f[s].hi = h.v;
        f[s].lo = l.v;
      }
    } else if constexpr (kBf16) {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) f[s] = *reinterpret_cast<const bf16x8*>(row + 16 * s + 8 * hh);
    } else {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) f[s] = row[2 * s + hh];
    }
  }

  // this lane's share of frags . row (the other lane half holds the rest); `frow`: the row the fragments were loaded from
  // (f32x3 reads it again: the dot is taken from the unsplit fp32 values)
  static __device__ __forceinline__ float dot_frags(const Frag* f, const T* __restrict__ frow, const T* __restrict__ row,
                                                    int hh) {
    float acc = 0.f;
    if constexpr (kX3) {
#pragma unroll
      for (int s = 0; s < kFrags; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(frow[16 * s + 8 * hh + j], row[16 * s + 8 * hh + j], acc);
    } else if constexpr (kBf16) {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) {
        const bf16x8 o = *reinterpret_cast<const bf16x8*>(row + 16 * s + 8 * hh);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc = fmaf(bf16_to_f32(static_cast<uint16_t>(f[s][j])), bf16_to_f32(static_cast<uint16_t>(o[j])), acc);
      }
    } else {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) acc = fmaf(f[s], row[2 * s + hh], acc);
    }
    return acc;
  }

  // X[swept row][resident row] = sum over the features, sub-tile st: lane r reads LDS row swap23(r)
  static __device__ __forceinline__ f32x16 dot(const L* rm, int st, int r, int hh, const Frag* b) {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    const L* a = rm + (32 * st + swap23(r)) * kPitch + (kTrans ? 8 * hh : hh);
    if constexpr (kX3) {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a + 16 * s);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(a + kRmPlane + 16 * s);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b[s].hi, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b[s].lo, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b[s].hi, acc, 0, 0, 0);
      }
    } else if constexpr (kBf16) {
#pragma unroll
      for (int s = 0; s < kFrags; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(a + 16 * s), b[s], acc, 0, 0, 0);
    } else {
#pragma unroll
      for (int s = 0; s < kFrags; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * s], b[s], acc, 0, 0, 0);
    }
    return acc;
  }

  // out[t][feature 32 t + .][resident row] += sum over the swept rows of image[row][feature] x[row][resident row]
  static __device__ __forceinline__ void acc(const L* rm, const L* tr, int st, const f32x16& x, f32x16* out, int r, int hh) {
    if constexpr (kX3) {
      union {
        bf16x8 v;
        uint32_t u[4];
      } xh[2], xl[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) split_bf16x2(x[8 * s + 2 * i], x[8 * s + 2 * i + 1], xh[s].u[i], xl[s].u[i]);
#pragma unroll
      for (int t = 0; t < D / 32; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const L* a = tr + (32 * t + r) * kPitchT + 32 * st + 16 * s + 8 * hh;
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a);
          const bf16x8 al = *reinterpret_cast<const bf16x8*>(a + kTrPlane);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xh[s].v, out[t], 0, 0, 0);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, xl[s].v, out[t], 0, 0, 0);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, xh[s].v, out[t], 0, 0, 0);
        }
    } else if constexpr (kBf16) {
      union {
        bf16x8 v;
        uint32_t u[4];
      } xb[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) xb[s].u[i] = pk_bf16(x[8 * s + 2 * i], x[8 * s + 2 * i + 1]);
#pragma unroll
      for (int t = 0; t < D / 32; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(tr + (32 * t + r) * kPitchT + 32 * st + 16 * s + 8 * hh);
          out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[s].v, out[t], 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const T* a = rm + (32 * st + slot_of(q, hh)) * kPitch + r;
#pragma unroll
        for (int t = 0; t < D / 32; ++t) out[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[32 * t], x[q], out[t], 0, 0, 0);
      }
    }
  }

  // features 32 t + 8 g + 4 hh .. + 3 of this lane's resident row, as 4-element stores
  template <bool DIV>
  static __device__ __forceinline__ void store(T* __restrict__ row, const f32x16* a, int hh, float den) {
#pragma unroll
    for (int t = 0; t < D / 32; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float4 v = make_float4(a[t][4 * g], a[t][4 * g + 1], a[t][4 * g + 2], a[t][4 * g + 3]);
        if constexpr (DIV) v = make_float4(v.x / den, v.y / den, v.z / den, v.w / den);
        store4<T>(row + 32 * t + 8 * g + 4 * hh, v);
      }
  }
};

// swept rows per stage: two sub-tiles where the LDS images stay below 64 KiB (f32x3 holds two planes per image: two
// sub-tiles up to D = 64)
template <typename A, int WHICH, int D>
constexpr int pa_sweep() {
  if (WHICH == 2) return 32;
  return std::is_same<A, uint16_t>::value || (std::is_same<A, f32x3>::value && D <= 64) ? 64 : 32;
}

template <typename A, int D>
__global__ __launch_bounds__(kPaThreads) void k_pa_fwd(const PaArgs p) {
  constexpr int SW = pa_sweep<A, 0, D>();
  using I = PaImg<A, D, SW>;
  using T = typename I::T;
  using L = typename I::L;
  __shared__ __attribute__((aligned(16))) L ks[I::kRm];
  __shared__ __attribute__((aligned(16))) L vs[I::kTrans ? 4 : I::kRm];
  __shared__ __attribute__((aligned(16))) L vt[I::kTr];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int h = blockIdx.y, hv = p.v_heads == 1 ? 0 : h;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kPaRows + 32 * wid + r;
  const int64_t ic = i < p.n ? i : p.n - 1;
  const T* kp = static_cast<const T*>(p.k) + h * D;
  const T* vp = static_cast<const T*>(p.v) + hv * D;
  typename I::Frag qf[I::kFrags];
  I::load_frags(static_cast<const T*>(p.q) + ic * p.ldq + h * D, hh, qf);
  f32x16 o[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) o[t][q] = 0.f;
  float rs = 0.f, den = 0.f;
  for (int64_t j0 = 0; j0 < p.l; j0 += SW) {
    I::template stage<true, false>(kp, p.ldk, j0, p.l, ks, nullptr);
    I::template stage<!I::kTrans, true>(vp, p.ldv, j0, p.l, vs, vt);
    __syncthreads();
#pragma unroll
    for (int st = 0; st < SW / 32; ++st) {
      const int64_t lim = p.l - j0 - 32 * st;        // swept rows of this sub-tile that exist
      if (lim > 0) {                                 // (workgroup-uniform)
        f32x16 x = I::dot(ks, st, r, hh, qf);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float s = slot_of(q, hh) < lim ? sigmoid<!I::kBf16>(x[q]) : 0.f;
          rs += s;                                   // r: fp32, before the operand's rounding to bf16
          if constexpr (I::kBf16) den += __uint_as_float(pk_bf16(s, 0.f) << 16);   // what the numerator's weights sum to
          x[q] = s;
        }
        I::acc(vs, vt, st, x, o, r, hh);
      }
    }
    __syncthreads();
  }
  rs += __shfl_xor(rs, 32, 64);
  // bf16: the numerator holds the ROUNDED weights, so it is divided by their sum — out stays a convex combination of the
  // value rows (one key: out = v exactly), which is what keeps g . v - delta free of rounding noise in the backward
  den = I::kBf16 ? den + __shfl_xor(den, 32, 64) : rs;
  if (i < p.n) {
    I::template store<true>(static_cast<T*>(p.out) + i * p.ldout + h * D, o, hh, den);
    if (hh == 0) p.rowsum[i * p.heads + h] = rs;
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// The exact softmax arm (include/sgf.h block N8; medium/ablation/oursSOFT.py): the same skeleton, layout and staging with
// an online maximum.  With z = scale q_i . k_j, per head:
//
//   sgf_pair_softmax_fwd    : m_i = max_j z,  r_i = sum_j exp(z - m_i),  out_i = sum_j exp(z - m_i) v_j / r_i,
//                             lse_i = m_i + log r_i
//   sgf_pair_softmax_bwd_q  : P = exp(z - lse_i),  delta_i = g_i . out_i,  dZ = scale P (g_i . v_j - delta_i),
//                             dq_i = sum_j dZ k_j
//   sgf_pair_softmax_bwd_kv : dv_j = sum_i P g_i,  dk_j = sum_i dZ q_i
//
//   * The resident row is the lane, so m, r and the rescale factor c = exp(m - m') are one scalar per lane.  The two lane
//     halves hold different swept rows of the same resident row: one exchange of the stage's maximum (all its sub-tiles)
//     before P is formed gives both the same m, hence the same c, and their partial r add up at the end as they stand.
//   * A key past l is -inf BEFORE the maximum: it takes no part in it and exp(-inf - m) is exactly 0.  Key j0 of a stage
//     always exists, so after the exchange the stage maximum is finite in every lane: m' is finite from the first stage on
//     and exp(-inf - m') = 0 is the first stage's c (never -inf - -inf).  z - m' <= 0 everywhere: nothing overflows for
//     any finite z, and a row whose earlier stages underflow entirely just rescales zeros.
//   * The backward launches recompute P from lse: no running maximum.  A swept query past n (bwd_kv) is staged with
//     lse = +inf: P = exp(0 - inf) = 0, and its g row is zeros.
//   * bf16 storage: P (fwd) and P, dZ (bwd) are rounded only as operands of the second products; r, lse, delta are fp32.
//     out divides the numerator by the sum of the ROUNDED weights, as the sigmoid forward does and for the same reason.
//   * exp: expf for fp32 storage, the hardware exp2 for bf16 storage (sigmoid<kExact>'s rule).
template <bool kExact>
__device__ __forceinline__ float pa_exp(float t) {
  return kExact ? expf(t) : __builtin_amdgcn_exp2f(1.44269504088896341f * t);
}

// D = 128: m, the held score tiles and the rescale put the unbounded allocation at 261 (bf16) / 283 (fp32) registers, one
// wave per SIMD where the sigmoid forward runs two; asked for two waves the compiler fits 206 / 210 without a spill (f32x3: 243).
template <typename A, int D>
__global__ __launch_bounds__(kPaThreads, D == 128 ? 2 : 1) void k_ps_fwd(const PaArgs p, const float scale) {
  constexpr int SW = pa_sweep<A, 0, D>();
  using I = PaImg<A, D, SW>;
  using T = typename I::T;
  using L = typename I::L;
  __shared__ __attribute__((aligned(16))) L ks[I::kRm];
  __shared__ __attribute__((aligned(16))) L vs[I::kTrans ? 4 : I::kRm];
  __shared__ __attribute__((aligned(16))) L vt[I::kTr];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int h = blockIdx.y, hv = p.v_heads == 1 ? 0 : h;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kPaRows + 32 * wid + r;
  const int64_t ic = i < p.n ? i : p.n - 1;
  const T* kp = static_cast<const T*>(p.k) + h * D;
  const T* vp = static_cast<const T*>(p.v) + hv * D;
  typename I::Frag qf[I::kFrags];
  I::load_frags(static_cast<const T*>(p.q) + ic * p.ldq + h * D, hh, qf);
  f32x16 o[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) o[t][q] = 0.f;
  float m = -INFINITY, rs = 0.f, den = 0.f;
  for (int64_t j0 = 0; j0 < p.l; j0 += SW) {
    I::template stage<true, false>(kp, p.ldk, j0, p.l, ks, nullptr);
    I::template stage<!I::kTrans, true>(vp, p.ldv, j0, p.l, vs, vt);
    __syncthreads();
    f32x16 x[SW / 32];
    float tm = -INFINITY;
#pragma unroll
    for (int st = 0; st < SW / 32; ++st) {
      const int64_t lim = p.l - j0 - 32 * st;        // swept rows of this sub-tile that exist (workgroup-uniform)
      if (lim > 0) {
        x[st] = I::dot(ks, st, r, hh, qf);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float z = slot_of(q, hh) < lim ? scale * x[st][q] : -INFINITY;
          x[st][q] = z;
          tm = fmaxf(tm, z);
        }
      }
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));          // both lane halves: the same maximum (finite: key j0 exists)
    const float mn = fmaxf(m, tm);
    const float c = pa_exp<!I::kBf16>(m - mn);       // first stage: exp(-inf - finite) = 0
    m = mn;
    rs *= c;
    den *= c;
#pragma unroll
    for (int t = 0; t < D / 32; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) o[t][q] *= c;
#pragma unroll
    for (int st = 0; st < SW / 32; ++st) {
      if (p.l - j0 - 32 * st > 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float pr = pa_exp<!I::kBf16>(x[st][q] - mn);                       // a masked key: exp(-inf) = 0
          rs += pr;                                                               // r: fp32, before the operand's rounding
          if constexpr (I::kBf16) den += __uint_as_float(pk_bf16(pr, 0.f) << 16);
          x[st][q] = pr;
        }
        I::acc(vs, vt, st, x[st], o, r, hh);
      }
    }
    __syncthreads();
  }
  rs += __shfl_xor(rs, 32, 64);
  den = I::kBf16 ? den + __shfl_xor(den, 32, 64) : rs;
  if (i < p.n) {
    I::template store<true>(static_cast<T*>(p.out) + i * p.ldout + h * D, o, hh, den);
    if (hh == 0) p.rowsum[i * p.heads + h] = m + logf(rs);       // lse
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// The backward kernels of both arms.  They recompute the scores from q, k and the forward's saved fp32 row value (`rowsum`:
// the sigmoid's r_i, the softmax's lse_i); a score policy holds what differs between the arms and nothing else:
//   row_const(saved) : the per-row constant rc the pair formula uses (held per lane in bwd_q, staged in LDS in bwd_kv)
//   kPastEnd         : rc of a swept query row past n (bwd_kv), chosen so that the row adds nothing
//   bwd<kExact>(z = q_i . k_j, gv = g_i . v_j, delta_i, rc, scale) -> w, the weight of g_i in dv_j, and dz = dL/dz;
//                      kExact: fp32 storage (expf), else the hardware exp2
// The expressions are kept as one statement each: the compiler contracts multiplies and adds inside a statement.
struct SigmoidScore {
  static constexpr float kPastEnd = 0.f;             // 1 / r = 0: w = dz = 0 (the staged zero rows alone would score 0.5)
  static __device__ __forceinline__ float row_const(float rowsum) { return 1.0f / rowsum; }
  // dZ = S (1 - S) (g . v - delta) / r.  1 - S is formed from S, so a saturated score has an exactly zero derivative
  template <bool kExact>
  static __device__ __forceinline__ void bwd(float z, float gv, float delta, float rinv, float, float& w, float& dz) {
    const float s = sigmoid<kExact>(z);
    w = s * rinv;
    dz = s * (1.0f - s) * ((gv - delta) * rinv);
  }
};

struct SoftmaxScore {
  static constexpr float kPastEnd = INFINITY;        // lse = +inf: P = exp(0 - inf) = 0, and the row's g is zeros
  static __device__ __forceinline__ float row_const(float lse) { return lse; }
  // P = exp(scale z - lse): no running maximum.  dZ = scale P (g . v - delta)
  template <bool kExact>
  static __device__ __forceinline__ void bwd(float z, float gv, float delta, float lse, float scale, float& w, float& dz) {
    const float pr = pa_exp<kExact>(scale * z - lse);
    w = pr;
    dz = scale * pr * (gv - delta);
  }
};

template <typename A, int D, typename Score>
__global__ __launch_bounds__(kPaThreads) void k_pair_bwd_q(const PaArgs p, const float scale) {
  constexpr int SW = pa_sweep<A, 1, D>();
  using I = PaImg<A, D, SW>;
  using T = typename I::T;
  using L = typename I::L;
  __shared__ __attribute__((aligned(16))) L ks[I::kRm];
  __shared__ __attribute__((aligned(16))) L vs[I::kRm];
  __shared__ __attribute__((aligned(16))) L kt[I::kTr];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const int h = blockIdx.y, hv = p.v_heads == 1 ? 0 : h;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kPaRows + 32 * wid + r;
  const int64_t ic = i < p.n ? i : p.n - 1;
  const T* kp = static_cast<const T*>(p.k) + h * D;
  const T* vp = static_cast<const T*>(p.v) + hv * D;
  typename I::Frag qf[I::kFrags], gf[I::kFrags];
  I::load_frags(static_cast<const T*>(p.g) + ic * p.ldg + h * D, hh, gf);
  const T* grow = static_cast<const T*>(p.g) + ic * p.ldg + h * D;
  float delta = I::dot_frags(gf, grow, static_cast<const T*>(p.o) + ic * p.ldo + h * D, hh);
  delta += __shfl_xor(delta, 32, 64);
  if (i < p.n && hh == 0) p.delta[i * p.heads + h] = delta;
  if (!p.dq) return;                                 // (uniform: delta only)
  I::load_frags(static_cast<const T*>(p.q) + ic * p.ldq + h * D, hh, qf);
  const float rc = Score::row_const(p.rowsum[ic * p.heads + h]);
  f32x16 dq[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) dq[t][q] = 0.f;
  for (int64_t j0 = 0; j0 < p.l; j0 += SW) {
    I::template stage<true, true>(kp, p.ldk, j0, p.l, ks, kt);
    I::template stage<true, false>(vp, p.ldv, j0, p.l, vs, nullptr);
    __syncthreads();
#pragma unroll
    for (int st = 0; st < SW / 32; ++st) {
      const int64_t lim = p.l - j0 - 32 * st;
      if (lim > 0) {
        f32x16 x = I::dot(ks, st, r, hh, qf);
        const f32x16 pv = I::dot(vs, st, r, hh, gf);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float w, dz;
          Score::template bwd<!I::kBf16>(x[q], pv[q], delta, rc, scale, w, dz);
          x[q] = slot_of(q, hh) < lim ? dz : 0.f;
        }
        I::acc(ks, kt, st, x, dq, r, hh);
      }
    }
    __syncthreads();
  }
  if (i < p.n) I::template store<false>(static_cast<T*>(p.dq) + i * p.lddq + h * D, dq, hh, 1.f);
}

template <typename A, int D, typename Score>
__global__ __launch_bounds__(kPaThreads) void k_pair_bwd_kv(const PaArgs p, const float scale) {
  constexpr int SW = pa_sweep<A, 2, D>();
  using I = PaImg<A, D, SW>;
  using T = typename I::T;
  using L = typename I::L;
  __shared__ __attribute__((aligned(16))) L qs[I::kRm];
  __shared__ __attribute__((aligned(16))) L gs[I::kRm];
  __shared__ __attribute__((aligned(16))) L qt[I::kTr];
  __shared__ __attribute__((aligned(16))) L gt[I::kTr];
  __shared__ float rc_s[SW], delta_s[SW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5;
  const bool shared_v = p.v_heads != p.heads;        // one value head: this workgroup walks every head, dv sums over them
  const int h_begin = shared_v ? 0 : blockIdx.y, h_end = shared_v ? p.heads : h_begin + 1;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kPaRows + 32 * wid + r;
  const int64_t jc = j < p.l ? j : p.l - 1;
  typename I::Frag kf[I::kFrags], vf[I::kFrags];
  I::load_frags(static_cast<const T*>(p.v) + jc * p.ldv + (shared_v ? 0 : h_begin) * D, hh, vf);
  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) dv[t][q] = 0.f;
  for (int h = h_begin; h < h_end; ++h) {
    I::load_frags(static_cast<const T*>(p.k) + jc * p.ldk + h * D, hh, kf);
#pragma unroll
    for (int t = 0; t < D / 32; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) dk[t][q] = 0.f;
    const T* qp = static_cast<const T*>(p.q) + h * D;
    const T* gp = static_cast<const T*>(p.g) + h * D;
    for (int64_t i0 = 0; i0 < p.n; i0 += SW) {
      I::template stage<true, true>(qp, p.ldq, i0, p.n, qs, qt);
      I::template stage<true, true>(gp, p.ldg, i0, p.n, gs, gt);
      if (threadIdx.x < SW) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < p.n;
        rc_s[threadIdx.x] = in ? Score::row_const(p.rowsum[i * p.heads + h]) : Score::kPastEnd;   // past the end: adds nothing
        delta_s[threadIdx.x] = in ? p.delta[i * p.heads + h] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int st = 0; st < SW / 32; ++st) {
        if (p.n - i0 - 32 * st > 0) {
          f32x16 x = I::dot(qs, st, r, hh, kf);
          f32x16 pv = I::dot(gs, st, r, hh, vf);
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int sl = 32 * st + slot_of(q, hh);
            const float rc = rc_s[sl], de = delta_s[sl];
            float w, dz;
            Score::template bwd<!I::kBf16>(x[q], pv[q], de, rc, scale, w, dz);
            x[q] = w;
            pv[q] = dz;
          }
          I::acc(gs, gt, st, x, dv, r, hh);
          I::acc(qs, qt, st, pv, dk, r, hh);
        }
      }
      __syncthreads();
    }
    if (j < p.l) {
      I::template store<false>(static_cast<T*>(p.dk) + j * p.lddk + h * D, dk, hh, 1.f);
      if (!shared_v) I::template store<false>(static_cast<T*>(p.dv) + j * p.lddv + h * D, dv, hh, 1.f);
    }
  }
  if (shared_v && j < p.l) I::template store<false>(static_cast<T*>(p.dv) + j * p.lddv, dv, hh, 1.f);
}

// x3: the sgf_pair_*_x3_* families, which take SGF_F32_BF16X3 and nothing else (the exact families never take it)
inline bool pa_shape_ok(int heads, int v_heads, int d, int dtype, bool x3 = false) {
  if (x3 ? dtype != SGF_F32_BF16X3 : (dtype != SGF_F32 && dtype != SGF_BF16)) return false;
  if (d != 32 && d != 64 && d != 128) return false;
  return heads >= 1 && heads <= 8 && (v_heads == 1 || v_heads == heads);
}

inline bool pa_aligned(const void* p, int64_t ld, int64_t per16) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % per16 == 0; }

// sizes, head counts, width and dtype of all three launches
int check_pa(const char* fn, bool x3, int64_t n, int64_t l, int heads, int v_heads, int d, int dtype) {
  SGF_REQUIRE(n >= 0 && l >= 0, SGF_E_INVALID, "%s: negative size n=%lld l=%lld", fn, static_cast<long long>(n),
              static_cast<long long>(l));
  SGF_REQUIRE(v_heads == 1 || v_heads == heads, SGF_E_INVALID, "%s: v_heads=%d must be 1 or heads=%d", fn, v_heads, heads);
  SGF_REQUIRE(pa_shape_ok(heads, v_heads, d, dtype, x3), SGF_E_UNSUPPORTED,
              "%s: needs d in {32, 64, 128}, 1 <= heads <= 8 and %s (heads=%d, d=%d, dtype %d)", fn,
              x3 ? "SGF_F32_BF16X3" : "SGF_F32 or SGF_BF16", heads, d, dtype);
  SGF_REQUIRE(n < (static_cast<int64_t>(1) << 31) && l < (static_cast<int64_t>(1) << 31), SGF_E_UNSUPPORTED,
              "%s: more than 2^31 - 1 rows", fn);
  return SGF_OK;
}

struct PaOperand {
  const char* name;
  const void* p;
  int64_t ld;
  int width;
};

// null pointers, then the widths, then the alignment: all before the first HIP call
int check_pa_rows(const char* fn, const PaOperand* ops, int count, int dtype) {
  for (int i = 0; i < count; ++i) SGF_REQUIRE(ops[i].p, SGF_E_INVALID, "%s: null pointer (%s)", fn, ops[i].name);
  for (int i = 0; i < count; ++i)
    SGF_REQUIRE(ops[i].ld >= ops[i].width, SGF_E_INVALID, "%s: leading dimension smaller than the width (%s: %lld < %d)", fn,
                ops[i].name, static_cast<long long>(ops[i].ld), ops[i].width);
  const int per16 = dtype == SGF_BF16 ? 8 : 4;
  for (int i = 0; i < count; ++i)
    SGF_REQUIRE(pa_aligned(ops[i].p, ops[i].ld, per16), SGF_E_INVALID,
                "%s: rows must be 16-byte aligned (pointers %% 16, leading dims %% %d elements; %s)", fn, per16, ops[i].name);
  return SGF_OK;
}

// The arms of the entries: what the forward saves per row, what l == 0 would ask for, and whether the family is the
// split-bf16 one (sgf_pair_*_x3_*: SGF_F32_BF16X3 only).
struct PaArm {
  bool softmax;
  const char *saved, *no_keys;
  bool x3;
};
constexpr PaArm kSigmoidArm = {false, "rowsum", "a row sum over no keys", false};
constexpr PaArm kSoftmaxArm = {true, "lse", "a softmax over no keys", false};
constexpr PaArm kSigmoidArmX3 = {false, "rowsum", "a row sum over no keys", true};
constexpr PaArm kSoftmaxArmX3 = {true, "lse", "a softmax over no keys", true};

// check_pa, then the score scale of the softmax arm
int check_pa_arm(const char* fn, const PaArm& arm, float scale, int64_t n, int64_t l, int heads, int v_heads, int d, int dtype) {
  if (int rc = check_pa(fn, arm.x3, n, l, heads, v_heads, d, dtype)) return rc;
  SGF_REQUIRE(!arm.softmax || (std::isfinite(scale) && scale > 0.f), SGF_E_INVALID, "%s: scale must be finite and positive (%g)",
              fn, static_cast<double>(scale));
  return SGF_OK;
}

// one launch over the storage dtype (SGF_F32_BF16X3: the f32x3 kernels), the width and the arm; the score scale is the second
// kernel argument of every kernel but the sigmoid forward (the sigmoid policy never reads it)
template <template <typename, int> class Launch>
int pa_dispatch(const PaArm& arm, int d, int dtype, const PaArgs& a, float scale, dim3 grid, hipStream_t st) {
  auto launch = [&](auto t) {
    using T = decltype(t);
    if (d == 32) Launch<T, 32>::run(arm.softmax, a, scale, grid, st);
    else if (d == 64) Launch<T, 64>::run(arm.softmax, a, scale, grid, st);
    else Launch<T, 128>::run(arm.softmax, a, scale, grid, st);
    SGF_LAUNCH_CHECK();
    return static_cast<int>(SGF_OK);
  };
  return dtype == SGF_F32_BF16X3 ? launch(f32x3{}) : by_dtype(dtype, launch);
}
template <typename T, int D>
struct PaFwd {
  static void run(bool softmax, const PaArgs& a, float scale, dim3 grid, hipStream_t st) {
    if (softmax) hipLaunchKernelGGL((k_ps_fwd<T, D>), grid, dim3(kPaThreads), 0, st, a, scale);
    else hipLaunchKernelGGL((k_pa_fwd<T, D>), grid, dim3(kPaThreads), 0, st, a);
  }
};
template <typename T, int D>
struct PaBwdQ {
  static void run(bool softmax, const PaArgs& a, float scale, dim3 grid, hipStream_t st) {
    if (softmax) hipLaunchKernelGGL((k_pair_bwd_q<T, D, SoftmaxScore>), grid, dim3(kPaThreads), 0, st, a, scale);
    else hipLaunchKernelGGL((k_pair_bwd_q<T, D, SigmoidScore>), grid, dim3(kPaThreads), 0, st, a, scale);
  }
};
template <typename T, int D>
struct PaBwdKv {
  static void run(bool softmax, const PaArgs& a, float scale, dim3 grid, hipStream_t st) {
    if (softmax) hipLaunchKernelGGL((k_pair_bwd_kv<T, D, SoftmaxScore>), grid, dim3(kPaThreads), 0, st, a, scale);
    else hipLaunchKernelGGL((k_pair_bwd_kv<T, D, SigmoidScore>), grid, dim3(kPaThreads), 0, st, a, scale);
  }
};

inline unsigned pa_tiles(int64_t rows) { return static_cast<unsigned>((rows + kPaRows - 1) / kPaRows); }

// delta fp32 [n, heads]; nothing of size l, nothing of size n x l
size_t pa_workspace_bytes(int64_t n, int64_t l, int heads) {
  if (n < 0 || l < 0 || heads < 1) return 0;
  return static_cast<size_t>(n) * heads * sizeof(float);
}

int64_t pa_lap_rows(const char* fn, int which, int heads, int d, int dtype, int laps, bool x3 = false) {
  if (which < 0 || which > 2 || laps < 1 || !pa_shape_ok(heads, heads, d, dtype, x3)) {
    set_error("%s: which=%d (0 fwd, 1 bwd_q, 2 bwd_kv), laps=%d, heads=%d, d=%d, dtype %d", fn, which, laps, heads, d, dtype);
    return -1;
  }
  return 0;      // every workgroup of the three kernels owns one resident tile: there is no second lap
}

// The three launches of both arms (`saved`: rowsum or lse).  Order of the checks: sizes, head counts, shape and dtype, the
// softmax's scale; n == 0 is a no-op; l == 0; null pointers, widths, alignment; `saved`; the workspace.
int pa_fwd(const char* fn, const PaArm& arm, float scale, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
           int64_t ldv, int64_t n, int64_t l, int heads, int v_heads, int d, int dtype, void* out, int64_t ldo, float* saved,
           void* stream) {
  if (int rc = check_pa_arm(fn, arm, scale, n, l, heads, v_heads, d, dtype)) return rc;
  if (n == 0) return SGF_OK;
  SGF_REQUIRE(l > 0, SGF_E_INVALID, "%s: l == 0 (%s)", fn, arm.no_keys);
  const PaOperand ops[] = {{"q", q, ldq, heads * d}, {"k", k, ldk, heads * d}, {"v", v, ldv, v_heads * d}, {"out", out, ldo, heads * d}};
  if (int rc = check_pa_rows(fn, ops, 4, dtype)) return rc;
  SGF_REQUIRE(saved, SGF_E_INVALID, "%s: null pointer (%s)", fn, arm.saved);
  PaArgs a = {};
  a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv, a.out = out, a.ldout = ldo, a.rowsum = saved;
  a.n = n, a.l = l, a.heads = heads, a.v_heads = v_heads;
  return pa_dispatch<PaFwd>(arm, d, dtype, a, scale, dim3(pa_tiles(n), heads), static_cast<hipStream_t>(stream));
}

int pa_bwd_q(const char* fn, const PaArm& arm, float scale, const void* g, int64_t ldg, const void* out, int64_t ldo,
             const float* saved, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n,
             int64_t l, int heads, int v_heads, int d, int dtype, void* dq, int64_t lddq, void* workspace, size_t workspace_bytes,
             void* stream) {
  if (int rc = check_pa_arm(fn, arm, scale, n, l, heads, v_heads, d, dtype)) return rc;
  if (n == 0) return SGF_OK;
  SGF_REQUIRE(l > 0, SGF_E_INVALID, "%s: l == 0 (%s)", fn, arm.no_keys);
  const PaOperand ops[] = {{"g", g, ldg, heads * d},   {"out", out, ldo, heads * d}, {"q", q, ldq, heads * d},
                           {"k", k, ldk, heads * d},   {"v", v, ldv, v_heads * d},   {"dq", dq, lddq, heads * d}};
  if (int rc = check_pa_rows(fn, ops, dq ? 6 : 5, dtype)) return rc;      // dq == NULL: delta only
  SGF_REQUIRE(saved, SGF_E_INVALID, "%s: null pointer (%s)", fn, arm.saved);
  SGF_REQUIRE(workspace && workspace_bytes >= pa_workspace_bytes(n, l, heads), SGF_E_WORKSPACE, "%s: workspace %zu < %zu", fn,
              workspace ? workspace_bytes : static_cast<size_t>(0), pa_workspace_bytes(n, l, heads));
  PaArgs a = {};
  a.g = g, a.ldg = ldg, a.o = out, a.ldo = ldo, a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv;
  a.rowsum = const_cast<float*>(saved), a.delta = static_cast<float*>(workspace), a.dq = dq, a.lddq = lddq;
  a.n = n, a.l = l, a.heads = heads, a.v_heads = v_heads;
  return pa_dispatch<PaBwdQ>(arm, d, dtype, a, scale, dim3(pa_tiles(n), heads), static_cast<hipStream_t>(stream));
}

int pa_bwd_kv(const char* fn, const PaArm& arm, float scale, const void* g, int64_t ldg, const float* saved, const void* q,
              int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l, int heads, int v_heads,
              int d, int dtype, void* dk, int64_t lddk, void* dv, int64_t lddv, const void* workspace, size_t workspace_bytes,
              void* stream) {
  if (int rc = check_pa_arm(fn, arm, scale, n, l, heads, v_heads, d, dtype)) return rc;
  if (n == 0) return SGF_OK;
  SGF_REQUIRE(l > 0, SGF_E_INVALID, "%s: l == 0 (%s)", fn, arm.no_keys);
  const PaOperand ops[] = {{"g", g, ldg, heads * d},   {"q", q, ldq, heads * d},     {"k", k, ldk, heads * d},
                           {"v", v, ldv, v_heads * d}, {"dk", dk, lddk, heads * d},  {"dv", dv, lddv, v_heads * d}};
  if (int rc = check_pa_rows(fn, ops, 6, dtype)) return rc;
  SGF_REQUIRE(saved, SGF_E_INVALID, "%s: null pointer (%s)", fn, arm.saved);
  SGF_REQUIRE(workspace && workspace_bytes >= pa_workspace_bytes(n, l, heads), SGF_E_WORKSPACE, "%s: workspace %zu < %zu", fn,
              workspace ? workspace_bytes : static_cast<size_t>(0), pa_workspace_bytes(n, l, heads));
  PaArgs a = {};
  a.g = g, a.ldg = ldg, a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv;
  a.rowsum = const_cast<float*>(saved), a.delta = static_cast<float*>(const_cast<void*>(workspace));
  a.dk = dk, a.lddk = lddk, a.dv = dv, a.lddv = lddv;
  a.n = n, a.l = l, a.heads = heads, a.v_heads = v_heads;
  return pa_dispatch<PaBwdKv>(arm, d, dtype, a, scale, dim3(pa_tiles(l), v_heads == heads ? heads : 1),
                              static_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace sgf

using namespace sgf;

// ---- block N7: the sigmoid arm ---------------------------------------------------------------------------------------
extern "C" int32_t sgf_pair_sigmoid_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype) {
  return pa_shape_ok(heads, v_heads, d, dtype) ? 1 : 0;
}

extern "C" size_t sgf_pair_sigmoid_workspace_bytes(int64_t n, int64_t l, int32_t heads) { return pa_workspace_bytes(n, l, heads); }

extern "C" int64_t sgf_pair_sigmoid_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps) {
  return pa_lap_rows("sgf_pair_sigmoid_lap_rows", which, heads, d, dtype, laps);
}

extern "C" int sgf_pair_sigmoid_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* out,
                                    int64_t ldo, float* rowsum, void* stream) {
  return pa_fwd("sgf_pair_sigmoid_fwd", kSigmoidArm, 1.0f, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d, dtype, out, ldo,
                rowsum, stream);
}

extern "C" int sgf_pair_sigmoid_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* rowsum,
                                      const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                      int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* dq,
                                      int64_t lddq, void* workspace, size_t workspace_bytes, void* stream) {
  return pa_bwd_q("sgf_pair_sigmoid_bwd_q", kSigmoidArm, 1.0f, g, ldg, out, ldo, rowsum, q, ldq, k, ldk, v, ldv, n, l, heads,
                  v_heads, d, dtype, dq, lddq, workspace, workspace_bytes, stream);
}

extern "C" int sgf_pair_sigmoid_bwd_kv(const void* g, int64_t ldg, const float* rowsum, const void* q, int64_t ldq,
                                       const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                                       int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* dk, int64_t lddk,
                                       void* dv, int64_t lddv, const void* workspace, size_t workspace_bytes, void* stream) {
  return pa_bwd_kv("sgf_pair_sigmoid_bwd_kv", kSigmoidArm, 1.0f, g, ldg, rowsum, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d,
                   dtype, dk, lddk, dv, lddv, workspace, workspace_bytes, stream);
}

// ---- block N8: the exact softmax arm ---------------------------------------------------------------------------------
extern "C" int32_t sgf_pair_softmax_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype) {
  return pa_shape_ok(heads, v_heads, d, dtype) ? 1 : 0;
}

extern "C" size_t sgf_pair_softmax_workspace_bytes(int64_t n, int64_t l, int32_t heads) { return pa_workspace_bytes(n, l, heads); }

extern "C" int64_t sgf_pair_softmax_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps) {
  return pa_lap_rows("sgf_pair_softmax_lap_rows", which, heads, d, dtype, laps);
}

extern "C" int sgf_pair_softmax_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale,
                                    void* out, int64_t ldo, float* lse, void* stream) {
  return pa_fwd("sgf_pair_softmax_fwd", kSoftmaxArm, scale, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d, dtype, out, ldo, lse,
                stream);
}

extern "C" int sgf_pair_softmax_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* lse,
                                      const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                      int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype,
                                      float scale, void* dq, int64_t lddq, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return pa_bwd_q("sgf_pair_softmax_bwd_q", kSoftmaxArm, scale, g, ldg, out, ldo, lse, q, ldq, k, ldk, v, ldv, n, l, heads,
                  v_heads, d, dtype, dq, lddq, workspace, workspace_bytes, stream);
}

extern "C" int sgf_pair_softmax_bwd_kv(const void* g, int64_t ldg, const float* lse, const void* q, int64_t ldq,
                                       const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                                       int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale, void* dk,
                                       int64_t lddk, void* dv, int64_t lddv, const void* workspace, size_t workspace_bytes,
                                       void* stream) {
  return pa_bwd_kv("sgf_pair_softmax_bwd_kv", kSoftmaxArm, scale, g, ldg, lse, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d,
                   dtype, dk, lddk, dv, lddv, workspace, workspace_bytes, stream);
}

// ---- block N9: the sigmoid arm on split-bf16 products (SGF_F32_BF16X3 only) -----------------------------------------
extern "C" int32_t sgf_pair_sigmoid_x3_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype) {
  return pa_shape_ok(heads, v_heads, d, dtype, true) ? 1 : 0;
}

extern "C" int64_t sgf_pair_sigmoid_x3_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps) {
  return pa_lap_rows("sgf_pair_sigmoid_x3_lap_rows", which, heads, d, dtype, laps, true);
}

extern "C" int sgf_pair_sigmoid_x3_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* out,
                                    int64_t ldo, float* rowsum, void* stream) {
  return pa_fwd("sgf_pair_sigmoid_x3_fwd", kSigmoidArmX3, 1.0f, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d, dtype, out, ldo,
                rowsum, stream);
}

extern "C" int sgf_pair_sigmoid_x3_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* rowsum,
                                      const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                      int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* dq,
                                      int64_t lddq, void* workspace, size_t workspace_bytes, void* stream) {
  return pa_bwd_q("sgf_pair_sigmoid_x3_bwd_q", kSigmoidArmX3, 1.0f, g, ldg, out, ldo, rowsum, q, ldq, k, ldk, v, ldv, n, l, heads,
                  v_heads, d, dtype, dq, lddq, workspace, workspace_bytes, stream);
}

extern "C" int sgf_pair_sigmoid_x3_bwd_kv(const void* g, int64_t ldg, const float* rowsum, const void* q, int64_t ldq,
                                       const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                                       int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* dk, int64_t lddk,
                                       void* dv, int64_t lddv, const void* workspace, size_t workspace_bytes, void* stream) {
  return pa_bwd_kv("sgf_pair_sigmoid_x3_bwd_kv", kSigmoidArmX3, 1.0f, g, ldg, rowsum, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d,
                   dtype, dk, lddk, dv, lddv, workspace, workspace_bytes, stream);
}

// ---- block N9: the exact softmax arm on split-bf16 products (SGF_F32_BF16X3 only) -----------------------------------
extern "C" int32_t sgf_pair_softmax_x3_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype) {
  return pa_shape_ok(heads, v_heads, d, dtype, true) ? 1 : 0;
}

extern "C" int64_t sgf_pair_softmax_x3_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps) {
  return pa_lap_rows("sgf_pair_softmax_x3_lap_rows", which, heads, d, dtype, laps, true);
}

extern "C" int sgf_pair_softmax_x3_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale,
                                    void* out, int64_t ldo, float* lse, void* stream) {
  return pa_fwd("sgf_pair_softmax_x3_fwd", kSoftmaxArmX3, scale, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d, dtype, out, ldo, lse,
                stream);
}

extern "C" int sgf_pair_softmax_x3_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* lse,
                                      const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                      int64_t n, int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype,
                                      float scale, void* dq, int64_t lddq, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return pa_bwd_q("sgf_pair_softmax_x3_bwd_q", kSoftmaxArmX3, scale, g, ldg, out, ldo, lse, q, ldq, k, ldk, v, ldv, n, l, heads,
                  v_heads, d, dtype, dq, lddq, workspace, workspace_bytes, stream);
}

extern "C" int sgf_pair_softmax_x3_bwd_kv(const void* g, int64_t ldg, const float* lse, const void* q, int64_t ldq,
                                       const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                                       int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale, void* dk,
                                       int64_t lddk, void* dv, int64_t lddv, const void* workspace, size_t workspace_bytes,
                                       void* stream) {
  return pa_bwd_kv("sgf_pair_softmax_x3_bwd_kv", kSoftmaxArmX3, scale, g, ldg, lse, q, ldq, k, ldk, v, ldv, n, l, heads, v_heads, d,
                   dtype, dk, lddk, dv, lddv, workspace, workspace_bytes, stream);
}
