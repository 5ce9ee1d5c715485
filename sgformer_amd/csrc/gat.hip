// gat.hip — attention over the stored entries of a CSR (torch_geometric 1.7.2 GATConv; include/sgf.h block N10).
//
//   sgf_gat_scores    al[n, h] = <xw[n, h, :], att_l[h, :]>, ar likewise: one pass over xw
//   sgf_gat_fwd       per target row: z = al[src] + ar[tgt], s = leaky_relu(z), softmax over the row with an online maximum
//                     (the entries are walked once), out = sum p~ xw[src]; writes out, lse and norm = (m, 1 / l)
//   sgf_gat_bwd_dst   per target row: delta = sum p~ dp and dar (three single-pass row sums), dp = <g[tgt], xw[src]>
//   sgf_gat_bwd_src   per row of the TRANSPOSED CSR (a source and its targets): dal and dxw, the two att terms included
//
// No atomics: every sum runs in stored order inside one group of lanes, so every result is bit-reproducible.  Nothing of
// size [E, H] or [E, H, C] exists: the weights are recomputed from al, ar and norm, the keep decisions from the seed.
//
// Geometry.  A row of H * C values is owned by a group of G lanes (8, 16, 32 or 64: 64 / G rows per wave, 256 / G per
// workgroup).  The group is cut into Hp = H rounded up to a power of two equal parts of Lh = G / Hp lanes, one part per head, and
// a lane holds K chunks of 4 consecutive channels of ITS head (chunk sub + k Lh of the head's C / 4), so
//   * a gathered row is read as 16-byte (fp32) or 8-byte (bf16) pieces, Lh neighbouring lanes reading Lh neighbouring pieces;
//   * a score z = al + ar, the softmax state (m, l) and the keep decision are per lane: the forward has no cross-lane step in
//     its loop; the per-entry, per-head dot product of the backward kernels is K local chunks and log2(Lh) butterfly steps;
//   * U entries are in flight per group (U K loads per lane before the first use), 64 / G groups per wave.
// A row of any length is walked by its one group: correct, and a latency tail on hubs (no long-row queue here).
#include "common.h"

#include <cmath>

namespace sgf {
namespace {

constexpr int kGatThreads = 256;
constexpr int kGatMaxBlocks = kNumCU * 8;      // the grid is capped: a workgroup walks its rows in laps (sgf_gat_lap_rows)
constexpr uint32_t kGatTag = 0x53474154u;      // third counter word of the keep decisions ("SGAT"; sgf_dropout: 0x5347464d)

struct GatArgs {
  const int64_t* rowptr;     // of the walked CSR: the forward one (fwd, bwd_dst) or the transposed one (bwd_src)
  const int32_t* colind;
  const void* xw;  int64_t ldx;
  const void* g;   int64_t ldg;
  const float *al, *ar, *att_l, *att_r, *bias, *norm, *delta_in, *dar_in;
  void* out;       int64_t ldo;      // fwd: out; bwd_src: dxw
  float *lse, *norm_out, *delta, *dar, *dal, *al_out, *ar_out;
  int64_t n_walk;            // rows of the walked CSR
  int64_t n_rows;            // targets
  int heads, c, lh_log2, mean;
  float slope, p, keep_scale, inv_h;
  uint64_t seed;
};

// 1 / (1 - p) where u >= p keeps, else 0, for entry (target i, source j) and head h: Philox4x32-10, key = seed, counter
// (i, j, kGatTag, h / 4), word h % 4 — the same function of (i, j, h) in the forward CSR and in the transposed one
__device__ __forceinline__ float gat_keep(uint64_t seed, uint32_t i, uint32_t j, int h, float p, float keep_scale) {
  uint32_t c[4] = {i, j, kGatTag, static_cast<uint32_t>(h >> 2)};
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const int w = h & 3;
  const uint32_t word = w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3];
  const float u = static_cast<float>(word >> 8) * (1.0f / 16777216.0f);   // [0, 1)
  return u >= p ? keep_scale : 0.f;
}

// what a lane owns: its head, and chunk sub + k Lh of the head's C / 4 chunks for k < K
template <int G, int K>
struct GatLane {
  int slot, h, sub, lh, cph, col0;
  bool head_ok;
  __device__ __forceinline__ GatLane(const GatArgs& a) {
    const int gl = threadIdx.x & (G - 1);
    slot = threadIdx.x / G;
    lh = 1 << a.lh_log2;
    h = gl >> a.lh_log2;
    sub = gl & (lh - 1);
    head_ok = h < a.heads;
    cph = a.c >> 2;
    col0 = h * a.c;
  }
  __device__ __forceinline__ bool ok(int k) const { return head_ok && sub + k * lh < cph; }
  __device__ __forceinline__ int ccol(int k) const { return 4 * (sub + k * lh); }   // first channel of chunk k in a row of C
  __device__ __forceinline__ int col(int k) const { return col0 + ccol(k); }        // ... in a row of H * C
  // sum over the lanes of this lane's head (a butterfly: every lane of the head gets the same bits)
  __device__ __forceinline__ float head_sum(float v) const {
    for (int off = lh >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
  }
};

__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}
__device__ __forceinline__ void axpy4(float w, float4 x, float4& acc) {
  acc.x = fmaf(w, x.x, acc.x);
  acc.y = fmaf(w, x.y, acc.y);
  acc.z = fmaf(w, x.z, acc.z);
  acc.w = fmaf(w, x.w, acc.w);
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

#define SGF_GAT_ROW_LOOP(n)                                                                                   \
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * (kGatThreads / G); base < (n);                       \
       base += static_cast<int64_t>(gridDim.x) * (kGatThreads / G))

// ---- 1: al, ar -----------------------------------------------------------------------------------------------------------
template <typename T, int G, int K>
__global__ __launch_bounds__(kGatThreads) void k_gat_scores(GatArgs a) {
  const GatLane<G, K> ln(a);
  const T* xw = static_cast<const T*>(a.xw);
  float4 wl[K], wr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    wl[k] = ln.ok(k) ? *reinterpret_cast<const float4*>(a.att_l + ln.col(k)) : zero4();
    wr[k] = ln.ok(k) ? *reinterpret_cast<const float4*>(a.att_r + ln.col(k)) : zero4();
  }
  SGF_GAT_ROW_LOOP(a.n_walk) {
    const int64_t i = base + ln.slot;
    if (i >= a.n_walk) continue;
    float sl = 0.f, sr = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float4 x = ln.ok(k) ? load4<T>(xw + i * a.ldx + ln.col(k)) : zero4();
      sl = dot4(x, wl[k], sl);
      sr = dot4(x, wr[k], sr);
    }
    sl = ln.head_sum(sl);
    sr = ln.head_sum(sr);
    if (ln.head_ok && ln.sub == 0) {
      a.al_out[i * a.heads + ln.h] = sl;
      a.ar_out[i * a.heads + ln.h] = sr;
    }
  }
}

// ---- 2: forward ----------------------------------------------------------------------------------------------------------
template <typename T, int G, int K, int U>
__global__ __launch_bounds__(kGatThreads) void k_gat_fwd(GatArgs a) {
  const GatLane<G, K> ln(a);
  const T* xw = static_cast<const T*>(a.xw);
  T* out = static_cast<T*>(a.out);
  const bool drop = a.p > 0.f;
  SGF_GAT_ROW_LOOP(a.n_walk) {
    const int64_t i = base + ln.slot;
    if (i >= a.n_walk) continue;
    const int64_t e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    const float ar_i = ln.head_ok ? a.ar[i * a.heads + ln.h] : 0.f;
    float m = -INFINITY, l = 0.f;
    float4 acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = zero4();
    for (int64_t e = e0; e < e1; e += U) {
      int32_t j[U];
      float s[U];
      float4 x[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u) j[u] = e + u < e1 ? a.colind[e + u] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          x[u][k] = (ln.ok(k) && j[u] >= 0) ? load4<T>(xw + static_cast<int64_t>(j[u]) * a.ldx + ln.col(k)) : zero4();
        const float z = ((ln.head_ok && j[u] >= 0) ? a.al[static_cast<int64_t>(j[u]) * a.heads + ln.h] : 0.f) + ar_i;
        s[u] = j[u] >= 0 ? (z > 0.f ? z : a.slope * z) : -INFINITY;
      }
      float mb = s[0];
#pragma unroll
      for (int u = 1; u < U; ++u) mb = fmaxf(mb, s[u]);
      if (mb > m) {                 // the maximum rises: rescale what is summed so far (first batch: exp(-inf) = 0 times 0)
        const float c = expf(m - mb);
        l *= c;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k].x *= c, acc[k].y *= c, acc[k].z *= c, acc[k].w *= c;
        m = mb;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float w = expf(s[u] - m);          // an entry past the row: exp(-inf) = 0
        l += w;                                  // the normaliser is over the undropped weights
        float wt = w;
        if (drop && j[u] >= 0)
          wt *= gat_keep(a.seed, static_cast<uint32_t>(i), static_cast<uint32_t>(j[u]), ln.h, a.p, a.keep_scale);
#pragma unroll
        for (int k = 0; k < K; ++k) axpy4(wt, x[u][k], acc[k]);
      }
    }
    const bool any = e1 > e0;       // an empty row: zero aggregate, lse 0, norm (0, 0)
    if (ln.head_ok && ln.sub == 0) {
      const int64_t o = i * a.heads + ln.h;
      a.lse[o] = any ? m + logf(l) : 0.f;
      a.norm_out[2 * o] = any ? m : 0.f;
      a.norm_out[2 * o + 1] = any ? 1.0f / l : 0.f;
    }
    const float den = any ? l : 1.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float4 o = make_float4(acc[k].x / den, acc[k].y / den, acc[k].z / den, acc[k].w / den);
      if (a.mean) {
        // mean over the heads: a butterfly over the Hp parts of the group (lanes of a head past H hold zeros)
        for (int off = ln.lh; off < G; off <<= 1) {
          o.x += __shfl_xor(o.x, off, 64);
          o.y += __shfl_xor(o.y, off, 64);
          o.z += __shfl_xor(o.z, off, 64);
          o.w += __shfl_xor(o.w, off, 64);
        }
        o.x *= a.inv_h, o.y *= a.inv_h, o.z *= a.inv_h, o.w *= a.inv_h;
      }
      const int col = a.mean ? ln.ccol(k) : ln.col(k);
      if (ln.ok(k) && (!a.mean || ln.h == 0)) {
        if (a.bias != nullptr) {
          const float4 b = *reinterpret_cast<const float4*>(a.bias + col);
          o.x += b.x, o.y += b.y, o.z += b.z, o.w += b.w;
        }
        store4<T>(out + i * a.ldo + col, o);
      }
    }
  }
}

// p, the slope factor and the keep factor of one entry from the saved per-node values
struct GatWeight {
  float p, sl, kf;
};
__device__ __forceinline__ GatWeight gat_weight(const GatArgs& a, bool drop, float al_j, float ar_i, float m_i, float linv_i,
                                                uint32_t i, uint32_t j, int h) {
  const float z = al_j + ar_i;
  GatWeight w;
  w.sl = z > 0.f ? 1.f : a.slope;
  w.p = expf(z * w.sl - m_i) * linv_i;
  w.kf = drop ? gat_keep(a.seed, i, j, h, a.p, a.keep_scale) : 1.f;
  return w;
}

// ---- 3: backward, target side: delta = A, dar = B - A S with A = sum p~ dp, B = sum p~ dp sl, S = sum p sl ------------------
template <typename T, int G, int K, int U>
__global__ __launch_bounds__(kGatThreads) void k_gat_bwd_dst(GatArgs a) {
  const GatLane<G, K> ln(a);
  const T* xw = static_cast<const T*>(a.xw);
  const T* g = static_cast<const T*>(a.g);
  const bool drop = a.p > 0.f;
  SGF_GAT_ROW_LOOP(a.n_walk) {
    const int64_t i = base + ln.slot;
    if (i >= a.n_walk) continue;
    const int64_t e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    const int64_t ih = i * a.heads + ln.h;
    const float ar_i = ln.head_ok ? a.ar[ih] : 0.f;
    const float m_i = ln.head_ok ? a.norm[2 * ih] : 0.f, linv_i = ln.head_ok ? a.norm[2 * ih + 1] : 0.f;
    float4 gi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      gi[k] = ln.ok(k) ? load4<T>(g + i * a.ldg + (a.mean ? ln.ccol(k) : ln.col(k))) : zero4();
      if (a.mean) gi[k].x *= a.inv_h, gi[k].y *= a.inv_h, gi[k].z *= a.inv_h, gi[k].w *= a.inv_h;
    }
    float A = 0.f, B = 0.f, S = 0.f;
    for (int64_t e = e0; e < e1; e += U) {
      int32_t j[U];
      float4 x[U][K];
      float alj[U];
#pragma unroll
      for (int u = 0; u < U; ++u) j[u] = e + u < e1 ? a.colind[e + u] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < K; ++k)
          x[u][k] = (ln.ok(k) && j[u] >= 0) ? load4<T>(xw + static_cast<int64_t>(j[u]) * a.ldx + ln.col(k)) : zero4();
        alj[u] = (ln.head_ok && j[u] >= 0) ? a.al[static_cast<int64_t>(j[u]) * a.heads + ln.h] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float dp = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) dp = dot4(gi[k], x[u][k], dp);
        dp = ln.head_sum(dp);
        if (j[u] >= 0) {
          const GatWeight w = gat_weight(a, drop, alj[u], ar_i, m_i, linv_i, static_cast<uint32_t>(i),
                                         static_cast<uint32_t>(j[u]), ln.h);
          const float t = w.p * w.kf * dp;
          A += t;
          B += t * w.sl;
          S += w.p * w.sl;
        }
      }
    }
    if (ln.head_ok && ln.sub == 0) {
      a.delta[ih] = A;
      a.dar[ih] = B - A * S;
    }
  }
}

// ---- 4: backward, source side: row j of the transposed CSR, entries = its targets i ----------------------------------------
template <typename T, int G, int K, int U>
__global__ __launch_bounds__(kGatThreads) void k_gat_bwd_src(GatArgs a) {
  const GatLane<G, K> ln(a);
  const T* xw = static_cast<const T*>(a.xw);
  const T* g = static_cast<const T*>(a.g);
  T* dxw = static_cast<T*>(a.out);
  const bool drop = a.p > 0.f;
  SGF_GAT_ROW_LOOP(a.n_walk) {
    const int64_t j = base + ln.slot;
    if (j >= a.n_walk) continue;
    const int64_t e0 = a.rowptr[j], e1 = a.rowptr[j + 1];
    const int64_t jh = j * a.heads + ln.h;
    const float al_j = ln.head_ok ? a.al[jh] : 0.f;
    float4 xj[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      xj[k] = ln.ok(k) ? load4<T>(xw + j * a.ldx + ln.col(k)) : zero4();
      acc[k] = zero4();
    }
    double dal = 0.0;      // thousands of terms whose quanta differ by the square of the targets' degrees: summed in fp64, rounded once
    for (int64_t e = e0; e < e1; e += U) {
      int32_t i[U];
      float4 gu[U][K];
      float ari[U], mi[U], linv[U], dlt[U];
#pragma unroll
      for (int u = 0; u < U; ++u) i[u] = e + u < e1 ? a.colind[e + u] : -1;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool on = i[u] >= 0;
#pragma unroll
        for (int k = 0; k < K; ++k)
          gu[u][k] = (ln.ok(k) && on) ? load4<T>(g + static_cast<int64_t>(i[u]) * a.ldg + (a.mean ? ln.ccol(k) : ln.col(k)))
                                      : zero4();
        const int64_t ih = static_cast<int64_t>(on ? i[u] : 0) * a.heads + ln.h;
        const bool rd = ln.head_ok && on;
        ari[u] = rd ? a.ar[ih] : 0.f;
        mi[u] = rd ? a.norm[2 * ih] : 0.f;
        linv[u] = rd ? a.norm[2 * ih + 1] : 0.f;
        dlt[u] = rd ? a.delta_in[ih] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (a.mean) {
#pragma unroll
          for (int k = 0; k < K; ++k) gu[u][k].x *= a.inv_h, gu[u][k].y *= a.inv_h, gu[u][k].z *= a.inv_h, gu[u][k].w *= a.inv_h;
        }
        float dp = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) dp = dot4(gu[u][k], xj[k], dp);
        dp = ln.head_sum(dp);
        if (i[u] >= 0) {
          const GatWeight w = gat_weight(a, drop, al_j, ari[u], mi[u], linv[u], static_cast<uint32_t>(i[u]),
                                         static_cast<uint32_t>(j), ln.h);
          dal += static_cast<double>(w.p * (w.kf * dp - dlt[u]) * w.sl);
          const float pt = w.p * w.kf;
#pragma unroll
          for (int k = 0; k < K; ++k) axpy4(pt, gu[u][k], acc[k]);
        }
      }
    }
    const float dal_j = static_cast<float>(dal);
    if (ln.head_ok && ln.sub == 0) a.dal[jh] = dal_j;
    // the score terms of dxw: al = <xw, att_l> and ar = <xw, att_r> (a source that is also a target: j < n_rows)
    const float dar_j = (ln.head_ok && a.dar_in != nullptr && j < a.n_rows) ? a.dar_in[jh] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!ln.ok(k)) continue;
      float4 o = acc[k];
      if (a.att_l != nullptr) axpy4(dal_j, *reinterpret_cast<const float4*>(a.att_l + ln.col(k)), o);
      if (a.att_r != nullptr) axpy4(dar_j, *reinterpret_cast<const float4*>(a.att_r + ln.col(k)), o);
      store4<T>(dxw + j * a.ldo + ln.col(k), o);
    }
  }
}

// ---- host: geometry, checks, launches ------------------------------------------------------------------------------------
struct GatGeom {
  int g, k, lh_log2;
};

inline bool gat_shape_ok(int heads, int c, int dtype) {
  if (dtype != SGF_F32 && dtype != SGF_BF16) return false;
  return heads >= 1 && heads <= 8 && c >= 4 && c % 4 == 0 && static_cast<int64_t>(heads) * c <= 1024;
}

// (shape checked) the smallest group that holds Hp parts of C / 4 chunks with K = 1, else the whole wave with K chunks per lane
inline GatGeom gat_geom(int heads, int c) {
  int hp = 1, hp_log2 = 0;
  while (hp < heads) hp *= 2, ++hp_log2;
  const int cph = c / 4, need = hp * cph;
  GatGeom gg;
  gg.g = need <= 8 ? 8 : need <= 16 ? 16 : need <= 32 ? 32 : 64;
  int g_log2 = 0;
  while ((1 << g_log2) < gg.g) ++g_log2;
  gg.lh_log2 = g_log2 - hp_log2;
  const int lh = 1 << gg.lh_log2;
  const int k = (cph + lh - 1) / lh;       // <= 8: Hp C <= 2 H C <= 2048
  gg.k = k <= 4 ? k : 8;
  return gg;
}

inline int64_t gat_lap(const GatGeom& gg) { return static_cast<int64_t>(kGatMaxBlocks) * (kGatThreads / gg.g); }

inline unsigned gat_grid(const GatGeom& gg, int64_t n) {
  const int64_t rpb = kGatThreads / gg.g, blocks = (n + rpb - 1) / rpb;
  return static_cast<unsigned>(blocks < kGatMaxBlocks ? blocks : kGatMaxBlocks);
}

template <int G_, int K_>
struct GatShape {
  static constexpr int G = G_, K = K_, U = K_ <= 2 ? 4 : (K_ <= 4 ? 2 : 1);
};

// f(GatShape<G, K>{}) for the geometry of a checked shape
template <typename F>
int gat_by_geom(const GatGeom& gg, F&& f) {
  switch (gg.g * 16 + gg.k) {
    case 8 * 16 + 1: return f(GatShape<8, 1>{});
    case 16 * 16 + 1: return f(GatShape<16, 1>{});
    case 32 * 16 + 1: return f(GatShape<32, 1>{});
    case 64 * 16 + 1: return f(GatShape<64, 1>{});
    case 64 * 16 + 2: return f(GatShape<64, 2>{});
    case 64 * 16 + 3: return f(GatShape<64, 3>{});
    case 64 * 16 + 4: return f(GatShape<64, 4>{});
    case 64 * 16 + 8: return f(GatShape<64, 8>{});
  }
  set_error("sgf_gat: no kernel for a group of %d lanes with %d chunks", gg.g, gg.k);
  return SGF_E_UNSUPPORTED;
}

enum GatKernel { kGatScores = 0, kGatFwd = 1, kGatBwdDst = 2, kGatBwdSrc = 3 };

int gat_launch(GatKernel which, int dtype, const GatGeom& gg, const GatArgs& a, hipStream_t st) {
  const dim3 grid(gat_grid(gg, a.n_walk)), block(kGatThreads);
  return by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    return gat_by_geom(gg, [&](auto shape) {
      using S = decltype(shape);
      switch (which) {
        case kGatScores: hipLaunchKernelGGL((k_gat_scores<T, S::G, S::K>), grid, block, 0, st, a); break;
        case kGatFwd: hipLaunchKernelGGL((k_gat_fwd<T, S::G, S::K, S::U>), grid, block, 0, st, a); break;
        case kGatBwdDst: hipLaunchKernelGGL((k_gat_bwd_dst<T, S::G, S::K, S::U>), grid, block, 0, st, a); break;
        case kGatBwdSrc: hipLaunchKernelGGL((k_gat_bwd_src<T, S::G, S::K, S::U>), grid, block, 0, st, a); break;
      }
      SGF_LAUNCH_CHECK();
      return static_cast<int>(SGF_OK);
    });
  });
}

// sizes, shape and dtype, the scalars: before the pointers, and for an empty problem too
int check_gat(const char* fn, int64_t n_rows, int64_t n_src, int heads, int c, int dtype) {
  SGF_REQUIRE(n_rows >= 0 && n_src >= 0, SGF_E_INVALID, "%s: negative size n_rows=%lld n_src=%lld", fn,
              static_cast<long long>(n_rows), static_cast<long long>(n_src));
  SGF_REQUIRE(gat_shape_ok(heads, c, dtype), SGF_E_UNSUPPORTED,
              "%s: needs 1 <= heads <= 8, c %% 4 == 0, heads * c <= 1024 and SGF_F32 or SGF_BF16 (heads=%d, c=%d, dtype %d)", fn,
              heads, c, dtype);
  SGF_REQUIRE(n_rows < (static_cast<int64_t>(1) << 31) && n_src < (static_cast<int64_t>(1) << 31), SGF_E_UNSUPPORTED,
              "%s: more than 2^31 - 1 rows", fn);
  return SGF_OK;
}

int check_gat_scalars(const char* fn, float slope, float p_drop) {
  SGF_REQUIRE(std::isfinite(slope), SGF_E_INVALID, "%s: negative_slope must be finite (%g)", fn, static_cast<double>(slope));
  SGF_REQUIRE(p_drop >= 0.f && p_drop <= 1.f, SGF_E_INVALID, "%s: p_drop must be in [0, 1] (%g)", fn,
              static_cast<double>(p_drop));
  return SGF_OK;
}

struct GatOperand {
  const char* name;
  const void* p;
  int64_t ld;      // of a row operand; -1: a plain array (null check only)
  int width;
};

// null pointers, then the widths, then the alignment of the row operands: all before the first HIP call
int check_gat_operands(const char* fn, const GatOperand* ops, int count, int dtype) {
  for (int i = 0; i < count; ++i) SGF_REQUIRE(ops[i].p, SGF_E_INVALID, "%s: null pointer (%s)", fn, ops[i].name);
  for (int i = 0; i < count; ++i)
    SGF_REQUIRE(ops[i].ld < 0 || ops[i].ld >= ops[i].width, SGF_E_INVALID,
                "%s: leading dimension smaller than the width (%s: %lld < %d)", fn, ops[i].name,
                static_cast<long long>(ops[i].ld), ops[i].width);
  const int bytes = dtype == SGF_BF16 ? 8 : 16;        // what a lane moves: 4 channels
  for (int i = 0; i < count; ++i)
    SGF_REQUIRE(ops[i].ld < 0 || (reinterpret_cast<uintptr_t>(ops[i].p) % bytes == 0 && ops[i].ld % 4 == 0), SGF_E_INVALID,
                "%s: rows must be %d-byte aligned (pointers %% %d, leading dims %% 4 elements; %s)", fn, bytes, bytes,
                ops[i].name);
  return SGF_OK;
}

void gat_fill(GatArgs& a, const GatGeom& gg, int heads, int c, int mean, float slope, float p_drop, uint64_t seed) {
  a.heads = heads, a.c = c, a.lh_log2 = gg.lh_log2, a.mean = mean ? 1 : 0;
  a.slope = slope, a.p = p_drop, a.keep_scale = p_drop < 1.f ? 1.0f / (1.0f - p_drop) : 0.f, a.inv_h = 1.0f / static_cast<float>(heads);
  a.seed = seed;
}

}  // namespace
}  // namespace sgf

using namespace sgf;

// ---- block N10 -----------------------------------------------------------------------------------------------------------
extern "C" int32_t sgf_gat_supported(int32_t heads, int32_t c, int32_t dtype) { return gat_shape_ok(heads, c, dtype) ? 1 : 0; }

extern "C" int64_t sgf_gat_lap_rows(int32_t heads, int32_t c, int32_t dtype, int32_t which) {
  if (which < 0 || which > 3 || !gat_shape_ok(heads, c, dtype)) {
    set_error("sgf_gat_lap_rows: which=%d (0 scores, 1 fwd, 2 bwd_dst, 3 bwd_src), heads=%d, c=%d, dtype %d", which, heads, c,
              dtype);
    return -1;
  }
  return gat_lap(gat_geom(heads, c));      // the four kernels share the geometry and the cap
}

extern "C" int sgf_gat_scores(const void* xw, int64_t ldx, const float* att_l, const float* att_r, int64_t n, int32_t heads,
                              int32_t c, int32_t dtype, float* al, float* ar, void* stream) {
  const char* fn = "sgf_gat_scores";
  if (int rc = check_gat(fn, n, n, heads, c, dtype)) return rc;
  if (n == 0) return SGF_OK;
  const GatOperand ops[] = {{"xw", xw, ldx, heads * c}, {"att_l", att_l, -1, 0}, {"att_r", att_r, -1, 0}, {"al", al, -1, 0},
                            {"ar", ar, -1, 0}};
  if (int rc = check_gat_operands(fn, ops, 5, dtype)) return rc;
  SGF_REQUIRE(reinterpret_cast<uintptr_t>(att_l) % 16 == 0 && reinterpret_cast<uintptr_t>(att_r) % 16 == 0, SGF_E_INVALID,
              "%s: att_l / att_r must be 16-byte aligned", fn);
  const GatGeom gg = gat_geom(heads, c);
  GatArgs a = {};
  gat_fill(a, gg, heads, c, 0, 0.f, 0.f, 0);
  a.xw = xw, a.ldx = ldx, a.att_l = att_l, a.att_r = att_r, a.al_out = al, a.ar_out = ar, a.n_walk = n, a.n_rows = n;
  return gat_launch(kGatScores, dtype, gg, a, static_cast<hipStream_t>(stream));
}

extern "C" int sgf_gat_fwd(const int64_t* rowptr, const int32_t* colind, const void* xw, int64_t ldx, const float* al,
                           const float* ar, const float* bias, int64_t n_rows, int64_t n_src, int32_t heads, int32_t c,
                           int32_t dtype, int32_t mean_heads, float negative_slope, float p_drop, uint64_t seed, void* out,
                           int64_t ldo, float* lse, float* norm, void* stream) {
  const char* fn = "sgf_gat_fwd";
  if (int rc = check_gat(fn, n_rows, n_src, heads, c, dtype)) return rc;
  if (int rc = check_gat_scalars(fn, negative_slope, p_drop)) return rc;
  if (n_rows == 0) return SGF_OK;
  const GatOperand ops[] = {{"rowptr", rowptr, -1, 0}, {"colind", colind, -1, 0}, {"xw", xw, ldx, heads * c},
                            {"out", out, ldo, mean_heads ? c : heads * c}, {"al", al, -1, 0}, {"ar", ar, -1, 0},
                            {"lse", lse, -1, 0}, {"norm", norm, -1, 0}};
  if (int rc = check_gat_operands(fn, ops, 8, dtype)) return rc;
  SGF_REQUIRE(reinterpret_cast<uintptr_t>(bias) % 16 == 0, SGF_E_INVALID, "%s: bias must be 16-byte aligned", fn);
  const GatGeom gg = gat_geom(heads, c);
  GatArgs a = {};
  gat_fill(a, gg, heads, c, mean_heads, negative_slope, p_drop, seed);
  a.rowptr = rowptr, a.colind = colind, a.xw = xw, a.ldx = ldx, a.al = al, a.ar = ar, a.bias = bias, a.out = out, a.ldo = ldo;
  a.lse = lse, a.norm_out = norm, a.n_walk = n_rows, a.n_rows = n_rows;
  return gat_launch(kGatFwd, dtype, gg, a, static_cast<hipStream_t>(stream));
}

extern "C" int sgf_gat_bwd_dst(const int64_t* rowptr, const int32_t* colind, const void* g, int64_t ldg, const void* xw,
                               int64_t ldx, const float* al, const float* ar, const float* norm, int64_t n_rows, int64_t n_src,
                               int32_t heads, int32_t c, int32_t dtype, int32_t mean_heads, float negative_slope, float p_drop,
                               uint64_t seed, float* delta, float* dar, void* stream) {
  const char* fn = "sgf_gat_bwd_dst";
  if (int rc = check_gat(fn, n_rows, n_src, heads, c, dtype)) return rc;
  if (int rc = check_gat_scalars(fn, negative_slope, p_drop)) return rc;
  if (n_rows == 0) return SGF_OK;
  const GatOperand ops[] = {{"rowptr", rowptr, -1, 0}, {"colind", colind, -1, 0}, {"g", g, ldg, mean_heads ? c : heads * c},
                            {"xw", xw, ldx, heads * c}, {"al", al, -1, 0}, {"ar", ar, -1, 0}, {"norm", norm, -1, 0},
                            {"delta", delta, -1, 0}, {"dar", dar, -1, 0}};
  if (int rc = check_gat_operands(fn, ops, 9, dtype)) return rc;
  const GatGeom gg = gat_geom(heads, c);
  GatArgs a = {};
  gat_fill(a, gg, heads, c, mean_heads, negative_slope, p_drop, seed);
  a.rowptr = rowptr, a.colind = colind, a.g = g, a.ldg = ldg, a.xw = xw, a.ldx = ldx, a.al = al, a.ar = ar, a.norm = norm;
  a.delta = delta, a.dar = dar, a.n_walk = n_rows, a.n_rows = n_rows;
  return gat_launch(kGatBwdDst, dtype, gg, a, static_cast<hipStream_t>(stream));
}

extern "C" int sgf_gat_bwd_src(const int64_t* t_rowptr, const int32_t* t_colind, const void* g, int64_t ldg, const void* xw,
                               int64_t ldx, const float* al, const float* ar, const float* norm, const float* delta,
                               const float* dar, const float* att_l, const float* att_r, int64_t n_rows, int64_t n_src,
                               int32_t heads, int32_t c, int32_t dtype, int32_t mean_heads, float negative_slope, float p_drop,
                               uint64_t seed, float* dal, void* dxw, int64_t lddx, void* stream) {
  const char* fn = "sgf_gat_bwd_src";
  if (int rc = check_gat(fn, n_rows, n_src, heads, c, dtype)) return rc;
  if (int rc = check_gat_scalars(fn, negative_slope, p_drop)) return rc;
  if (n_src == 0) return SGF_OK;
  const GatOperand ops[] = {{"t_rowptr", t_rowptr, -1, 0}, {"t_colind", t_colind, -1, 0}, {"g", g, ldg, mean_heads ? c : heads * c},
                            {"xw", xw, ldx, heads * c}, {"dxw", dxw, lddx, heads * c}, {"al", al, -1, 0}, {"ar", ar, -1, 0},
                            {"norm", norm, -1, 0}, {"delta", delta, -1, 0}, {"dal", dal, -1, 0}};
  if (int rc = check_gat_operands(fn, ops, 10, dtype)) return rc;
  // att_l / att_r / dar may be null: dxw then has no score term of that side
  SGF_REQUIRE(reinterpret_cast<uintptr_t>(att_l) % 16 == 0 && reinterpret_cast<uintptr_t>(att_r) % 16 == 0, SGF_E_INVALID,
              "%s: att_l / att_r must be 16-byte aligned", fn);
  SGF_REQUIRE(att_r == nullptr || dar != nullptr, SGF_E_INVALID, "%s: null pointer (dar, with att_r given)", fn);
  const GatGeom gg = gat_geom(heads, c);
  GatArgs a = {};
  gat_fill(a, gg, heads, c, mean_heads, negative_slope, p_drop, seed);
  a.rowptr = t_rowptr, a.colind = t_colind, a.g = g, a.ldg = ldg, a.xw = xw, a.ldx = ldx, a.al = al, a.ar = ar, a.norm = norm;
  a.delta_in = delta, a.dar_in = dar, a.att_l = att_l, a.att_r = att_r, a.dal = dal, a.out = dxw, a.ldo = lddx;
  a.n_walk = n_src, a.n_rows = n_rows;
  return gat_launch(kGatBwdSrc, dtype, gg, a, static_cast<hipStream_t>(stream));
}
