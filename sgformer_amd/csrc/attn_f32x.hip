// attn_f32x.hip — the row passes of the one-head attention from the un-projected input (sgf_attn_h_fwd, _bwd_apply,
// _bwd_reduce; fp32 storage) with every [N, d] x [d, d] / [N, d]^T [N, d] product formed as THREE bf16 matrix-core
// products: SGF_F32_BF16X3, what torch.set_float32_matmul_precision('high' / 'medium') asks for.
//
// Each fp32 operand is split as a = hi + lo (common.h split_bf16x2; lo = 0 where hi is not finite) and
//     a b  ~  hi_a hi_b + hi_a lo_b + lo_a hi_b
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (error model: DESIGN.md §4).  The exact kernels
// (k_attn_apply<float, DP, 4|5|6>, k_attn_reduce<float, DP, 3>, csrc/attn.hip) run v_mfma_f32_32x32x2_f32 at 1/16 of that
// rate and are matrix-pipe-bound at d = 256.
//
// ONLY the matrix products are split.  The row dots (h.w, g.o), 1 / den, dnum = g / den, dden, the three vector sums of the
// reduce and the epilogue's vectors (m, w, ds) are the exact kernels' fp32 VALU arithmetic.
//
//   k_attn_h_apply_f32x   the skeleton of k_linear_f32x (csrc/linear_f32x.hip): the d x d matrix split once into the waves'
//                         registers, row tiles split once in the staging pass into hi / lo bf16 planes in LDS, row-wise
//                         epilogue out = ar[n] * acc + br[n] * cvec[j] (+ out) with the per-row scalars of k_attn_apply.
//                         The backward stays TWO launches (dh = dnum M^T + dden w, then dh += h D + ds): one launch would
//                         need both split matrices resident, 2 x 128 VGPRs per wave at d = 256 — the whole register file
//                         of a wave at two waves per SIMD, with nothing left for the operands and the accumulator.
//   k_attn_h_reduce_f32x  the skeleton of k_gram_f32x (csrc/gram_f32x.hip) with a third stream: h, g and o come in through
//                         registers, dnum = g / den and dden = -(g.o) / den are formed there, the column sums ride along in
//                         fp32, and h / dnum land in LDS as [column][row] bf16 images.  A row of the staging pass is spread
//                         over d / 32 waves, so the row dot g.o is added across them through LDS (in wave order:
//                         deterministic), in the images' 16-byte column pads — at d = 256 the images fill the whole LDS.
//                         Per-block partials in the layout of reduce_shared.h, added by attn.hip's k_hbwd_finalize.
#include "reduce_shared.h"

namespace sgf {
namespace {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 zero4f() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float dot4f(const float4& a, const float4& b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

// ------------------------------------------------------------------------------------------------------------------------
// apply:  out[n, d] = ar[n] * (A[n, d] B[d, d]) + br[n] * cvec  (+ out)
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kHFwd = 0;    // A = h,          B = M,   ar = br = 1 / den, cvec = m;   den = h.w + beta is written
constexpr int kHBwd1 = 1;   // A = g / den,    B = M^T, ar = 1, br = dden = -(g.o) / den, cvec = w
constexpr int kHBwd2 = 2;   // A = h,          B = D,   ar = br = 1, cvec = ds, out += ...

struct HApplyArgs {
  const float* a;      // h (HFwd, HBwd2) or g (HBwd1)
  const float* a2;     // HBwd1: o
  float* out;
  int64_t lda, lda2, ldo;
  const float* bmat;   // [d, d] row-major
  const float* cvec;   // [d]
  const float* dvec;   // HFwd: w
  const float* beta;   // HFwd: device scalar
  float* den;          // [n]: written by HFwd, read by HBwd1
  int64_t n;
  int32_t d;
  int32_t trans_b;     // B[k][j] = bmat[j * d + k]
};

// K-halves per column strip and block size: as k_linear_f32x (at DP = 256 a wave keeps its strip's whole K, 128 VGPRs)
template <int DP>
constexpr int hx_kh() { return DP == 256 ? 1 : 2; }
template <int DP>
constexpr int hx_threads() { return 512 * hx_kh<DP>(); }

template <int DP, int MODE>
__global__ __launch_bounds__(hx_threads<DP>()) void k_attn_h_apply_f32x(HApplyArgs p) {
  constexpr int KH = hx_kh<DP>();
  constexpr int NT = hx_threads<DP>();
  constexpr int NS = DP / 32;         // 32-column strips
  constexpr int RS = 8 / NS;          // row sub-blocks
  constexpr int RT = 32 * RS;         // rows per tile (128 / 64 / 32)
  constexpr int F4 = DP / 4;
  constexpr int RPP = NT / F4;        // rows covered per staging pass
  constexpr int NP = RT / RPP;        // staging passes (2, or 4 at DP = 256)
  constexpr int LD = DP + 4;          // fp32 accumulator rows
  constexpr int LH = DP + 8;          // bf16 plane rows
  constexpr int KW = DP / KH;         // k range of a wave
  constexpr int KS = KW / 16;         // its k-steps of 16
  constexpr int PLANE = RT * LH;      // bf16 elements per plane
  // [buf][hi, lo][RT][LH] bf16 (= 2 PLANE floats), [kh][RT][LD] fp32, [buf][ar | br][RT]
  __shared__ __attribute__((aligned(16))) float smem[2 * PLANE + KH * RT * LD + 4 * RT];
  uint16_t* const ldsA = reinterpret_cast<uint16_t*>(smem);
  float* const ldsC = smem + 2 * PLANE;
  float* const ldsR = ldsC + KH * RT * LD;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i31 = lane & 31;
  const int hi = lane >> 5;
  const int kh = wave % KH;
  const int ws = (wave / KH) % NS;
  const int wr = (wave / KH) / NS;
  const int d = p.d;

  // resident piece of the matrix, split: element e of bh[s] / bl[s] = B[KW kh + 16 s + 8 hi + e][32 ws + i31]
  bf16x8 bh[KS], bl[KS];
  {
    const int j = 32 * ws + i31;
    auto bval = [&](int k) -> float {
      if (k >= d || j >= d) return 0.f;
      return p.trans_b ? p.bmat[static_cast<int64_t>(j) * d + k] : p.bmat[static_cast<int64_t>(k) * d + j];
    };
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      u32x4 h, l;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = KW * kh + 16 * s + 8 * hi + 2 * t;
        uint32_t hh, ll;
        split_bf16x2(bval(k), bval(k + 1), hh, ll);
        h[t] = hh;
        l[t] = ll;
      }
      bh[s] = __builtin_bit_cast(bf16x8, h);
      bl[s] = __builtin_bit_cast(bf16x8, l);
    }
  }

  // staging / epilogue geometry (same thread map for both); a row's F4 chunks sit in one wave
  const int scol = (tid % F4) * 4;
  const int srow0 = tid / F4;
  const bool scol_ok = scol < d;
  const float4 zc = scol_ok ? *reinterpret_cast<const float4*>(p.cvec + scol) : zero4f();
  const float4 zd = (MODE == kHFwd && scol_ok) ? *reinterpret_cast<const float4*>(p.dvec + scol) : zero4f();
  const float hbeta = MODE == kHFwd ? p.beta[0] : 0.f;

  const float* pa = p.a + scol;
  const float* pa2 = MODE == kHBwd1 ? p.a2 + scol : nullptr;
  float* po = p.out + scol;

  float4 ra[NP], ra2[NP];
  float rden[NP];
  const int64_t ntiles = (p.n + RT - 1) / RT;

  auto issue = [&](int64_t tile) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t row = tile * RT + srow0 + i * RPP;
      const bool ok = scol_ok && row < p.n;
      ra[i] = ok ? *reinterpret_cast<const float4*>(pa + row * p.lda) : zero4f();
      if (MODE == kHBwd1) {
        ra2[i] = ok ? *reinterpret_cast<const float4*>(pa2 + row * p.lda2) : zero4f();
        rden[i] = (row < p.n) ? p.den[row] : 1.f;
      }
    }
  };
  auto commit = [&](int buf, int64_t tile) {
    float* rs = ldsR + buf * 2 * RT;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int lrow = srow0 + i * RPP;
      const int64_t row = tile * RT + lrow;
      float4 w = ra[i];
      float ar = 1.f, br = 1.f;
      if (MODE == kHFwd) {
        const float den = group_sum<F4>(dot4f(ra[i], zd)) + hbeta;
        ar = 1.0f / den;
        br = ar;
        if (scol == 0 && row < p.n) p.den[row] = den;
      } else if (MODE == kHBwd1) {
        const float gdo = group_sum<F4>(dot4f(ra[i], ra2[i]));
        const float inv = 1.0f / rden[i];
        w = make_float4(ra[i].x * inv, ra[i].y * inv, ra[i].z * inv, ra[i].w * inv);
        br = -gdo * inv;
      }
      uint2 h, l;
      split_bf16x2(w.x, w.y, h.x, l.x);
      split_bf16x2(w.z, w.w, h.y, l.y);
      uint16_t* dst = ldsA + (2 * buf * RT + lrow) * LH + scol;
      *reinterpret_cast<uint2*>(dst) = h;
      *reinterpret_cast<uint2*>(dst + PLANE) = l;
      if (scol == 0) {
        rs[lrow] = ar;
        rs[RT + lrow] = br;
      }
    }
  };

  int64_t tile = blockIdx.x;
  int buf = 0;
  if (tile < ntiles) {
    issue(tile);
    commit(0, tile);
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
    {
      const float* rs = ldsR + buf * 2 * RT;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int lrow = srow0 + i * RPP;
        const int64_t row = tile * RT + lrow;
        if (scol_ok && row < p.n) {
          const float4 c0 = *reinterpret_cast<const float4*>(&ldsC[lrow * LD + scol]);
          const float4 c1 = KH == 2 ? *reinterpret_cast<const float4*>(&ldsC[(RT + lrow) * LD + scol]) : zero4f();
          const float ar = rs[lrow], br = rs[RT + lrow];
          float4 v = make_float4(ar * (c0.x + c1.x), ar * (c0.y + c1.y), ar * (c0.z + c1.z), ar * (c0.w + c1.w));
          v.x += br * zc.x; v.y += br * zc.y; v.z += br * zc.z; v.w += br * zc.w;
          if (MODE == kHBwd2) {
            const float4 o = *reinterpret_cast<const float4*>(po + row * p.ldo);
            v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
          }
          *reinterpret_cast<float4*>(po + row * p.ldo) = v;
        }
      }
    }
    if (has_next) commit(buf ^ 1, next);
    __syncthreads();
    buf ^= 1;
  }
}

template <int MODE>
int launch_h_apply(const HApplyArgs& p, int DP, hipStream_t st) {
  const int RT = 32 * (8 / (DP / 32));
  const int64_t ntiles = (p.n + RT - 1) / RT;
  const int nblk = static_cast<int>(ntiles < kRedMaxBlocks ? ntiles : kRedMaxBlocks);
  if (DP == 64) hipLaunchKernelGGL((k_attn_h_apply_f32x<64, MODE>), dim3(nblk), dim3(hx_threads<64>()), 0, st, p);
  else if (DP == 128) hipLaunchKernelGGL((k_attn_h_apply_f32x<128, MODE>), dim3(nblk), dim3(hx_threads<128>()), 0, st, p);
  else hipLaunchKernelGGL((k_attn_h_apply_f32x<256, MODE>), dim3(nblk), dim3(hx_threads<256>()), 0, st, p);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// reduce:  C[d x d] = h^T dnum, colsum = sum h dden, second vector = sum dnum, scalar = sum dden
// ------------------------------------------------------------------------------------------------------------------------
constexpr int kHrThreads = 512;                 // 8 waves = 2 per SIMD

struct HReduceArgs {
  const float* h;
  const float* g;
  const float* o;
  const float* den;   // [n]
  int64_t ldh, ldg, ldo;
  int64_t n;
  int32_t d;
  float* partial;     // [gridDim.x][kRedPartialStride]
};

// A stage holds 8192 elements of each operand: ROWS = 32 / 64 / 128 rows of DP = 256 / 128 / 64 columns, as four
// [column][row] bf16 images (h hi, h lo, dnum hi, dnum lo) whose columns are ROWS + 8 bf16 apart (16 bytes of pad: the
// ds_read_b128 fragments of 16 consecutive columns cover the 64 banks once).  Two stages: 160 / 144 / 136 KiB.
// Wave blocks of C are 64 x 32 NTB; where C has fewer than eight of them (DP < 256) the spare waves take the k-steps of a
// stage in turn (RG row groups), as k_attn_reduce does; their tiles are added in LDS before the partial is written.
template <int DP>
struct HrGeom {
  static constexpr int ROWS = 8192 / DP;
  static constexpr int RQ = ROWS / 4;                  // 4-row groups of the staging pass
  static constexpr int PITCH = ROWS + 8;
  static constexpr int IMAGE = DP * PITCH;
  static constexpr int STAGE = 4 * IMAGE;
  static constexpr int NTB = DP == 256 ? 4 : 2;        // 32-column tiles per wave block
  static constexpr int NBD = DP / (32 * NTB);          // wave blocks per row of C
  static constexpr int NBLK = (DP / 64) * NBD;         // wave blocks of C (8 / 4 / 1)
  static constexpr int RG = 8 / NBLK;                  // row groups (1 / 2 / 8)
  static constexpr int KSTEPS = ROWS / 16;             // MFMA k-steps per stage (2 / 4 / 8)
  static constexpr int SPG = KSTEPS / RG;              // per row group (2 / 2 / 1)
};

template <int DP>
__global__ __launch_bounds__(kHrThreads) void k_attn_h_reduce_f32x(HReduceArgs p) {
  using G = HrGeom<DP>;
  constexpr int ROWS = G::ROWS, RQ = G::RQ, PITCH = G::PITCH, IMAGE = G::IMAGE, STAGE = G::STAGE, NTB = G::NTB;
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int blk = wave % G::NBLK, grp = wave / G::NBLK;
  const int wm = blk / G::NBD, wd = blk % G::NBD;        // this wave's 64 x 32 NTB block of C
  const int i31 = lane & 31, hh = lane >> 5;

  // staging: rows 4 r4 .. 4 r4 + 3, columns 4 c4 .. 4 c4 + 3 of the three streams.  A wave takes 8 row groups x 8 column
  // chunks (as k_gram_f32x: 128 contiguous bytes of a row per 8 lanes), the waves tile the stage CB chunk blocks wide
  constexpr int CB = DP / 32;
  const int rr = lane & 7;
  const int r4 = rr + 8 * (wave / CB), c4 = (lane >> 3) + 8 * (wave % CB);
  const int col = 4 * c4;
  const bool col_ok = col < p.d;
  float vh[4][4], vg[4][4], vo[4][4], vden[4];
  float cs[4] = {0.f, 0.f, 0.f, 0.f};    // sum h dden
  float csb[4] = {0.f, 0.f, 0.f, 0.f};   // sum dnum
  float sden = 0.f;                      // sum dden (the threads of column chunk 0: one per row)
  const int64_t total = (p.n + ROWS - 1) / ROWS;

  // the row dots' exchange: float4 f = 8 wave + rr in the pad of column f of the first image (never staged, never read as a
  // fragment)
  auto red4 = [&](int f) -> float4* { return reinterpret_cast<float4*>(smem + f * PITCH + ROWS); };

  auto issue = [&](int64_t t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = t * ROWS + 4 * r4 + i;
      const bool ok = col_ok && row < p.n;
      const float4 x = ok ? *reinterpret_cast<const float4*>(p.h + row * p.ldh + col) : zero4f();
      const float4 y = ok ? *reinterpret_cast<const float4*>(p.g + row * p.ldg + col) : zero4f();
      const float4 z = ok ? *reinterpret_cast<const float4*>(p.o + row * p.ldo + col) : zero4f();
      vh[i][0] = x.x; vh[i][1] = x.y; vh[i][2] = x.z; vh[i][3] = x.w;
      vg[i][0] = y.x; vg[i][1] = y.y; vg[i][2] = y.z; vg[i][3] = y.w;
      vo[i][0] = z.x; vo[i][1] = z.y; vo[i][2] = z.z; vo[i][3] = z.w;
      vden[i] = row < p.n ? p.den[row] : 1.f;
    }
  };
  // this wave's share of g.o for the stage's rows: added over the lanes that hold the same rows, then left for commit()
  auto dots = [&]() {
    float4 pd;
    float* pdv = reinterpret_cast<float*>(&pd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = vg[i][0] * vo[i][0] + vg[i][1] * vo[i][1] + vg[i][2] * vo[i][2] + vg[i][3] * vo[i][3];
      s += __shfl_xor(s, 8, 64);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      pdv[i] = s;
    }
    if (lane < 8) *red4(8 * wave + rr) = pd;
  };
  auto commit = [&](int buf) {
    float gdo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CB; ++j) {           // the CB waves that hold these rows, in wave order
      const float4 v = *red4(8 * ((wave / CB) * CB + j) + rr);
      gdo[0] += v.x; gdo[1] += v.y; gdo[2] += v.z; gdo[3] += v.w;
    }
    float inv[4], dden[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      inv[i] = 1.0f / vden[i];
      dden[i] = -gdo[i] * inv[i];
      if (c4 == 0) sden += dden[i];      // rows past n: g = o = 0, dden = 0
    }
    uint16_t* base = smem + buf * STAGE + col * PITCH + 4 * r4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float dn[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dn[i] = vg[i][q] * inv[i];
        cs[q] += vh[i][q] * dden[i];
        csb[q] += dn[i];
      }
      uint2 h, l;
      split_bf16x2(vh[0][q], vh[1][q], h.x, l.x);
      split_bf16x2(vh[2][q], vh[3][q], h.y, l.y);
      *reinterpret_cast<uint2*>(base + q * PITCH) = h;
      *reinterpret_cast<uint2*>(base + IMAGE + q * PITCH) = l;
      split_bf16x2(dn[0], dn[1], h.x, l.x);
      split_bf16x2(dn[2], dn[3], h.y, l.y);
      *reinterpret_cast<uint2*>(base + 2 * IMAGE + q * PITCH) = h;
      *reinterpret_cast<uint2*>(base + 3 * IMAGE + q * PITCH) = l;
    }
  };

  // accumulator tiles that hold valid columns (wave-uniform): rows 64 wm + 32 mt < d, columns 32 NTB wd + 32 kt < d
  const int rem_a = p.d - 64 * wm, rem_b = p.d - 32 * NTB * wd;
  const int nta = rem_a <= 0 ? 0 : (rem_a > 32 ? 2 : 1);
  const int ntb = rem_b <= 0 ? 0 : (rem_b >= 32 * NTB ? NTB : (rem_b + 31) / 32);

  f32x16 acc[2][NTB];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][kt][r] = 0.f;

  int64_t t = blockIdx.x;
  int buf = 0;
  if (t < total) {
    issue(t);
    dots();
    __syncthreads();
    commit(0);
  }
  __syncthreads();
  for (; t < total; t += gridDim.x) {
    const int64_t next = t + gridDim.x;
    const bool has_next = next < total;     // block-uniform
    if (has_next) issue(next);
    // lane (i31, hh) of k-step s: column i31 of the tile, rows 16 s + 8 hh .. + 7
    const uint16_t* fa = smem + buf * STAGE + (64 * wm + i31) * PITCH + 8 * hh;
    const uint16_t* fb = smem + buf * STAGE + 2 * IMAGE + (32 * NTB * wd + i31) * PITCH + 8 * hh;
#pragma unroll 1
    for (int si = 0; si < G::SPG; ++si) {
      const int s = grp + G::RG * si;
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        ah[mt] = *reinterpret_cast<const bf16x8*>(fa + 32 * mt * PITCH + 16 * s);
        al[mt] = *reinterpret_cast<const bf16x8*>(fa + IMAGE + 32 * mt * PITCH + 16 * s);
      }
#pragma unroll
      for (int kt = 0; kt < NTB; ++kt) {
        const bf16x8 bh = *reinterpret_cast<const bf16x8*>(fb + 32 * kt * PITCH + 16 * s);
        const bf16x8 bl = *reinterpret_cast<const bf16x8*>(fb + IMAGE + 32 * kt * PITCH + 16 * s);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
          if (mt < nta && kt < ntb) {
            acc[mt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh, acc[mt][kt], 0, 0, 0);
            acc[mt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl, acc[mt][kt], 0, 0, 0);
            acc[mt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh, acc[mt][kt], 0, 0, 0);
          }
      }
    }
    if (has_next) {
      dots();
      __syncthreads();
      commit(buf ^ 1);
    }
    __syncthreads();
    buf ^= 1;
  }

  float* part = p.partial + static_cast<int64_t>(blockIdx.x) * kRedPartialStride;
  if (G::RG == 1) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = 64 * wm + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh;
          part[i * DP + 32 * NTB * wd + 32 * kt + i31] = acc[mt][kt][r];
        }
  } else {
    // the row groups' tiles are added here, in group order, so that the partial is one DP x DP tile for every DP (the
    // finalize then walks an eighth / a half of the partials' bytes); the last barrier of the loop ended every LDS read
    constexpr int TW = 32 * NTB;
    float* tile = reinterpret_cast<float*>(smem);          // [wave = grp * NBLK + blk][64][TW]
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int kt = 0; kt < NTB; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          tile[(wave * 64 + 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * hh) * TW + 32 * kt + i31] = acc[mt][kt][r];
    __syncthreads();
    for (int e = tid; e < G::NBLK * 64 * TW; e += kHrThreads) {
      const int b = e / (64 * TW), i = (e / TW) % 64, j = e % TW;
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < G::RG; ++g) s += tile[((g * G::NBLK + b) * 64 + i) * TW + j];
      part[(64 * (b / G::NBD) + i) * DP + TW * (b % G::NBD) + j] = s;
    }
    __syncthreads();
  }
  // the vector sums: the RQ threads of a column chunk add theirs in row-group order (deterministic)
  float* red = reinterpret_cast<float*>(smem);      // [RQ][DP] + [RQ]; the last barrier of the loop ended every LDS read
  *reinterpret_cast<float4*>(&red[r4 * DP + col]) = make_float4(cs[0], cs[1], cs[2], cs[3]);
  if (c4 == 0) red[RQ * DP + r4] = sden;
  __syncthreads();
  if (tid < DP / 4) {
    float4 s = zero4f();
#pragma unroll 8
    for (int g = 0; g < RQ; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(&red[g * DP + 4 * tid]);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(part + kRedTileElems + 4 * tid) = s;
  }
  if (tid == 64) {
    float s = 0.f;
    for (int g = 0; g < RQ; ++g) s += red[RQ * DP + g];
    part[kRedTileElems + DP] = s;
  }
  __syncthreads();
  *reinterpret_cast<float4*>(&red[r4 * DP + col]) = make_float4(csb[0], csb[1], csb[2], csb[3]);
  __syncthreads();
  if (tid < DP / 4) {
    float4 s = zero4f();
#pragma unroll 8
    for (int g = 0; g < RQ; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(&red[g * DP + 4 * tid]);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(part + kRedVecB + 4 * tid) = s;
  }
}

inline int hx_padded(int d) { return d <= 64 ? 64 : (d <= 128 ? 128 : 256); }
inline bool hx_aligned(const void* p, int64_t ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0; }

}  // namespace

bool attn_h_f32x_supported(int d) { return d >= 4 && d <= 256 && d % 4 == 0; }

int attn_h_f32x_fwd(const float* h, int64_t ldh, int64_t n, int d, const float* M, const float* m, const float* w,
                    const float* beta, float* out, int64_t ldo, float* den, hipStream_t st) {
  SGF_REQUIRE(attn_h_f32x_supported(d) && n > 0, SGF_E_UNSUPPORTED, "sgf_attn_h_fwd: d=%d unsupported for SGF_F32_BF16X3", d);
  SGF_REQUIRE(hx_aligned(h, ldh) && hx_aligned(out, ldo), SGF_E_INVALID, "sgf_attn_h_fwd: alignment");
  HApplyArgs a{};
  a.a = h; a.lda = ldh;
  a.out = out; a.ldo = ldo;
  a.bmat = M; a.trans_b = 0; a.cvec = m; a.dvec = w; a.beta = beta;
  a.den = den; a.n = n; a.d = d;
  return launch_h_apply<kHFwd>(a, hx_padded(d), st);
}

int attn_h_f32x_bwd_apply(const float* h, int64_t ldh, const float* g, int64_t ldg, const float* o, int64_t ldo,
                          const float* den, int64_t n, int d, const float* M, const float* w, const float* D,
                          const float* ds, float* dh, int64_t lddh, hipStream_t st) {
  SGF_REQUIRE(attn_h_f32x_supported(d) && n > 0, SGF_E_UNSUPPORTED, "sgf_attn_h_bwd_apply: d=%d unsupported for SGF_F32_BF16X3",
              d);
  SGF_REQUIRE(hx_aligned(h, ldh) && hx_aligned(g, ldg) && hx_aligned(o, ldo) && hx_aligned(dh, lddh), SGF_E_INVALID,
              "sgf_attn_h_bwd_apply: operands must be 4-element aligned");
  const int DP = hx_padded(d);
  HApplyArgs a{};
  a.n = n; a.d = d;
  a.den = const_cast<float*>(den);
  a.out = dh; a.ldo = lddh;
  // dh = dnum M^T + dden w
  a.a = g; a.lda = ldg;
  a.a2 = o; a.lda2 = ldo;
  a.bmat = M; a.trans_b = 1; a.cvec = w;
  int rc = launch_h_apply<kHBwd1>(a, DP, st);
  if (rc != SGF_OK) return rc;
  // dh += h D + ds
  a.a = h; a.lda = ldh;
  a.a2 = nullptr; a.lda2 = 0;
  a.bmat = D; a.trans_b = 0; a.cvec = ds;
  return launch_h_apply<kHBwd2>(a, DP, st);
}

int attn_h_f32x_bwd_reduce(const float* h, int64_t ldh, const float* g, int64_t ldg, const float* o, int64_t ldo,
                           const float* den, int64_t n, int d, float* partial, int* nblk, int* DP_out, int* RG_out,
                           hipStream_t st) {
  SGF_REQUIRE(attn_h_f32x_supported(d) && n > 0, SGF_E_UNSUPPORTED,
              "sgf_attn_h_bwd_reduce: d=%d unsupported for SGF_F32_BF16X3", d);
  SGF_REQUIRE(hx_aligned(h, ldh) && hx_aligned(g, ldg) && hx_aligned(o, ldo), SGF_E_INVALID,
              "sgf_attn_h_bwd_reduce: h/g/o must be 4-element aligned with ld %% 4 == 0");
  const int DP = hx_padded(d);
  HReduceArgs a{h, g, o, den, ldh, ldg, ldo, n, d, partial};
  const int rows = 8192 / DP;
  const int64_t total = (n + rows - 1) / rows;
  const int nb = static_cast<int>(total < kRedMaxBlocks ? total : kRedMaxBlocks);
  if (DP == 64) {
    hipLaunchKernelGGL(k_attn_h_reduce_f32x<64>, dim3(nb), dim3(kHrThreads), 0, st, a);
    *RG_out = 1;
  } else if (DP == 128) {
    hipLaunchKernelGGL(k_attn_h_reduce_f32x<128>, dim3(nb), dim3(kHrThreads), 0, st, a);
    *RG_out = 1;
  } else {
    hipLaunchKernelGGL(k_attn_h_reduce_f32x<256>, dim3(nb), dim3(kHrThreads), 0, st, a);
    *RG_out = 1;
  }
  SGF_LAUNCH_CHECK();
  *nblk = nb;
  *DP_out = DP;
  return SGF_OK;
}

}  // namespace sgf
