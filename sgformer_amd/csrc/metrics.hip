// metrics.hip — N5: the trainers' evaluation metrics (large/data_utils.py:199-246: eval_f1, eval_acc, eval_rocauc) as
// INTEGER counts formed on the device.  The host turns the counts into the metric with one division per column.
//
// sgf_rocauc_counts — per label column the Mann-Whitney counts of the AUC.  Three steps, no host sync:
//   1. k_auc_keys: one streaming pass over the selected [m, c] logits / labels (lanes run along a row, as csrc/bce.hip)
//      writes one 64-bit key per element,
//          [ column | status:3 | order-preserving fp32 score:32 | positive:1 ]
//      status 0 = a 0 / 1 label with a comparable score; bit 0 = label neither 0 nor 1, bit 1 = NaN score, bit 2 = NaN label.
//   2. rocprim::radix_sort_keys over all m * c keys.  The column sits in the top bits, so column k ends up as the m
//      consecutive keys [k m, (k + 1) m) — its valid elements first, by score, negatives before positives inside a tie —
//      whatever m and c are: one column of millions of rows (the binary data sets) is sorted by the whole chip.
//   3. k_auc_rank: one block per 2048 consecutive sorted keys of a column.  With a = first and b = one-past-last position
//      of an element's tie group, twice its mid-rank is a + b + 1, and
//          U2 = sum over positives (a + b + 1)  -  P (P + 1)        (Mann-Whitney, ties counted half).
//      a comes from a block max-scan over the tie-group heads; the group's positives are its tail [pa, b), so the sum is
//      formed at the group's LAST element as (b - pa) (a + b + 1), which needs one key of look-ahead and no backward scan.
//      A group that reaches into the chunk from the left finds a and pa with a 64-ary search of the sorted column (one
//      wave, four probes deep at a million rows): tie groups of any length, across threads and blocks, cost the same.
//   All sums are integers (64-bit integer atomics per block, then k_auc_final): exact whatever the launch geometry.
//
// sgf_argmax_count — { labelled rows, rows whose argmax equals the label } in one pass over the selected rows: G lanes
// share a row (G = the power of two >= c, at most 64), each forms max over its columns of the packed pair
// (order-preserving score with NaN above everything, 2^32 - 1 - column), a shuffle tree takes the maximum: the first
// maximal column, the first NaN if there is one — torch.argmax on the CPU.  Per-block integer partials, summed in order.
#include "common.h"

#include <rocprim/rocprim.hpp>

namespace sgf {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 8 blocks per CU
constexpr int kItems = 8;         // sorted keys per thread of k_auc_rank
constexpr int kChunk = kThreads * kItems;
constexpr int kStatusShift = 33, kColShift = 36;

// SGF_ROCAUC_STAGES=1 / 2: stop sgf_rocauc_counts after the key pass / after the sort (the counts are then NOT the
// contract's) — scripts/metrics_probe.py times the three stages between HIP events by difference.  Default: all three.
EnvInt g_stages{"SGF_ROCAUC_STAGES", 3};

// fp32 -> uint32 whose unsigned order is the float order; -0.0 == +0.0 (canonicalised before the bit transform)
__device__ __forceinline__ uint32_t order_key(float x) {
  if (x == 0.f) x = 0.f;
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void split_elem(int64_t u, int c, bool small, int64_t& j, int& k) {
  if (small) {
    const uint32_t jj = static_cast<uint32_t>(u) / static_cast<uint32_t>(c);
    j = jj;
    k = static_cast<int>(static_cast<uint32_t>(u) - jj * static_cast<uint32_t>(c));
  } else {
    j = u / c;
    k = static_cast<int>(u - j * c);
  }
}

template <typename T, int TK>
__global__ __launch_bounds__(kThreads) void k_auc_keys(const T* __restrict__ logits, int64_t ldl, int64_t n, int c,
                                                       const void* __restrict__ tgt, int64_t ldt,
                                                       const int64_t* __restrict__ idx, int64_t total, bool small,
                                                       uint64_t* __restrict__ keys) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kThreads;
  for (int64_t u = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; u < total; u += step) {
    int64_t j;
    int k;
    split_elem(u, c, small, j, k);
    const int64_t r = idx ? idx[j] : j;
    uint32_t status = 1, pos = 0, score = 0;   // (a row number outside [0, n) is not read: it counts as `other`)
    if (r >= 0 && r < n) {
      const float x = load1<T>(logits + r * ldl + k);
      status = 0;
      if constexpr (TK == SGF_METRIC_TARGET_F32) {
        const float t = static_cast<const float*>(tgt)[r * ldt + k];
        if (t != t) status = 4;
        else if (t == 1.f) pos = 1;
        else if (t != 0.f) status = 1;
      } else {
        const int64_t t = static_cast<const int64_t*>(tgt)[r * ldt + k];
        if (t == 1) pos = 1;
        else if (t != 0) status = 1;
      }
      if (status != 4 && x != x) status |= 2;
      if (status == 0) score = order_key(x);
      else pos = 0;
    }
    keys[u] = (static_cast<uint64_t>(k) << kColShift) | (static_cast<uint64_t>(status) << kStatusShift) |
              (static_cast<uint64_t>(score) << 1) | pos;
  }
}

// Smallest q in [0, hi] with (col[q] >> sh) >= t, for a sorted column and a position hi known to satisfy it.  One wave:
// 64 evenly spaced probes per round, the range shrinks 64-fold.  Every lane returns the same value.
__device__ __forceinline__ int wave_lower_bound(const uint64_t* __restrict__ col, int hi, uint64_t t, int sh, int lane) {
  int lo = 0;
  while (lo < hi) {
    const int span = hi - lo;
    const int step = (span + 63) / 64;
    const int64_t p = static_cast<int64_t>(lo) + static_cast<int64_t>(lane) * step;
    const bool ge = p >= hi || (col[p] >> sh) >= t;
    const unsigned long long mask = __ballot(ge);
    const int first = mask ? __ffsll(mask) - 1 : 64;
    if (first == 0) {
      hi = lo;
    } else {
      int64_t nhi = static_cast<int64_t>(lo) + static_cast<int64_t>(first) * step;
      if (nhi > hi) nhi = hi;
      lo = static_cast<int>(static_cast<int64_t>(lo) + static_cast<int64_t>(first - 1) * step + 1);
      hi = static_cast<int>(nhi);
    }
  }
  return lo;
}

struct Heads {
  int a, pa;   // last tie-group head / last head of a run of equal (score, label) at or before an element; -1 = none yet
};
struct HeadsMax {
  __device__ __forceinline__ Heads operator()(const Heads& x, const Heads& y) const {
    return Heads{x.a > y.a ? x.a : y.a, x.pa > y.pa ? x.pa : y.pa};
  }
};

// acc[k] = { P, Nn, sum over positives (a + b + 1), other, nan_scores, unlabelled } += this chunk's share
__global__ __launch_bounds__(kThreads) void k_auc_rank(const uint64_t* __restrict__ keys, int64_t m, int nchunk,
                                                       unsigned long long* __restrict__ acc) {
  using Scan = rocprim::block_scan<Heads, kThreads>;
  __shared__ uint64_t sk[kChunk + kChunk / kItems + 2];   // thread t's 8 keys at t * 9 .. t * 9 + 7: no bank conflict
  __shared__ typename Scan::storage_type scan_st;
  __shared__ int carry[2];
  __shared__ unsigned long long red[kThreads / 64][6];
  const int col_i = blockIdx.x / nchunk, ch = blockIdx.x - col_i * nchunk;
  const uint64_t* col = keys + static_cast<int64_t>(col_i) * m;
  const int q0 = ch * kChunk;                                   // (m < 2^31: positions fit an int)
  const int cnt = static_cast<int>(m - q0 < kChunk ? m - q0 : kChunk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int p = tid; p < cnt; p += kThreads) sk[p + (p >> 3)] = col[q0 + p];
  // the keys on either side of the chunk, or a value no key of this column's valid part can equal in its upper bits
  if (tid == 0) sk[kChunk + kChunk / kItems] = q0 > 0 ? col[q0 - 1] : ~0ull;
  if (tid == 64) sk[kChunk + kChunk / kItems + 1] = static_cast<int64_t>(q0) + cnt < m ? col[q0 + cnt] : ~0ull;
  __syncthreads();
  const uint64_t left = sk[kChunk + kChunk / kItems], right = sk[kChunk + kChunk / kItems + 1];
  const uint64_t k0 = sk[0];
  // a run that reaches in from the left starts in an earlier chunk: search the sorted column for its first position
  if (wave == 0 && (left >> 1) == (k0 >> 1)) {
    const int a0 = wave_lower_bound(col, q0, k0 >> 1, 1, lane);
    if (lane == 0) carry[0] = a0;
  }
  if (wave == 1 && left == k0) {
    const int pa0 = wave_lower_bound(col, q0, k0, 0, lane);
    if (lane == 0) carry[1] = pa0;
  }
  uint64_t key[kItems + 2];
  const int base = tid * kItems;
  key[0] = tid == 0 ? left : sk[(base - 1) + ((base - 1) >> 3)];
#pragma unroll
  for (int i = 0; i < kItems; ++i) key[i + 1] = base + i < cnt ? sk[base + i + tid] : ~0ull;
  // (the key after a thread's last one: the next thread's first, or the right neighbour of the chunk)
  if (base + kItems < cnt) key[kItems + 1] = sk[base + kItems + tid + 1];
  else key[kItems + 1] = right;
  Heads mine{-1, -1};
#pragma unroll
  for (int i = 0; i < kItems; ++i) {
    if (base + i < cnt) {
      if ((key[i] >> 1) != (key[i + 1] >> 1)) mine.a = q0 + base + i;
      if (key[i] != key[i + 1]) mine.pa = q0 + base + i;
    }
  }
  Heads before;
  Scan().exclusive_scan(mine, before, Heads{-1, -1}, scan_st, HeadsMax());
  __syncthreads();                                              // (carry[] is visible; scan storage is done with)
  int a = before.a >= 0 ? before.a : carry[0];
  int pa = before.pa >= 0 ? before.pa : carry[1];
  unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < kItems; ++i) {
    if (base + i < cnt) {
      const uint64_t kk = key[i + 1];
      const int q = q0 + base + i;
      if ((key[i] >> 1) != (kk >> 1)) a = q;
      if (key[i] != kk) pa = q;
      const uint32_t status = static_cast<uint32_t>(kk >> kStatusShift) & 7u;
      const bool positive = (kk & 1ull) != 0;
      // (the key after position m - 1 is the all-ones sentinel, which differs from every key: a tail, as it is)
      const bool tail = (kk >> 1) != (key[i + 2] >> 1);
      if (status == 0) {
        v[positive ? 0 : 1] += 1;
        if (positive && tail)
          v[2] += static_cast<unsigned long long>(q + 1 - pa) * (static_cast<unsigned long long>(a) + q + 2ull);
      } else {
        v[3] += status & 1u;
        v[4] += (status >> 1) & 1u;
        v[5] += (status >> 2) & 1u;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 6; ++s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[s] += __shfl_xor(v[s], off, 64);
    if (lane == 0) red[wave][s] = v[s];
  }
  __syncthreads();
  if (tid < 6) {
    unsigned long long s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w][tid];
    if (s) atomicAdd(acc + static_cast<int64_t>(col_i) * 6 + tid, s);
  }
}

// counts[k][2]: sum of (a + b + 1) over the positives -> U2 = that - P (P + 1)
__global__ void k_auc_final(int64_t* __restrict__ counts, int c) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < c) {
    const int64_t p = counts[static_cast<int64_t>(k) * 6];
    counts[static_cast<int64_t>(k) * 6 + 2] -= p * (p + 1);
  }
}

template <typename T, int LK, int G>
__global__ __launch_bounds__(kThreads) void k_argmax(const T* __restrict__ logits, int64_t ldl, int64_t n, int c,
                                                     const void* __restrict__ labels, int64_t lds,
                                                     const int64_t* __restrict__ idx, int64_t m,
                                                     unsigned long long* __restrict__ part) {
  constexpr int kRows = kThreads / G;   // rows of one block round
  __shared__ unsigned long long red[kThreads / 64][2];
  const int sub = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kRows;
  const int64_t rounds = (m + step - 1) / step;
  unsigned long long labelled = 0, correct = 0;
  for (int64_t i = 0; i < rounds; ++i) {               // (uniform trip count: the shuffles below need every lane)
    const int64_t j = i * step + static_cast<int64_t>(blockIdx.x) * kRows + grp;
    int64_t r = -1;
    if (j < m) r = idx ? idx[j] : j;
    const bool ok = r >= 0 && r < n;                   // (a row number outside [0, n) is not read and not counted)
    unsigned long long best = 0;
    if (ok) {
      const T* row = logits + r * ldl;
      for (int k = sub; k < c; k += G) {
        const float x = load1<T>(row + k);
        const uint32_t key = x != x ? 0xffffffffu : order_key(x);
        const unsigned long long cand = (static_cast<unsigned long long>(key) << 32) | (0xffffffffu - static_cast<uint32_t>(k));
        best = cand > best ? cand : best;
      }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if (ok && sub == 0) {
      const uint32_t pred = 0xffffffffu - static_cast<uint32_t>(best);
      if constexpr (LK == SGF_METRIC_TARGET_F32) {
        const float l = static_cast<const float*>(labels)[r * lds];
        if (l == l) {
          labelled += 1;
          correct += static_cast<float>(pred) == l ? 1 : 0;
        }
      } else {
        labelled += 1;
        correct += static_cast<const int64_t*>(labels)[r * lds] == static_cast<int64_t>(pred) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    labelled += __shfl_xor(labelled, off, 64);
    correct += __shfl_xor(correct, off, 64);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = labelled, red[threadIdx.x >> 6][1] = correct;
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    part[static_cast<int64_t>(blockIdx.x) * 2 + threadIdx.x] = s;
  }
}

// one wave: lane l adds block partials l, l + 64, ... in order, then a fixed shuffle tree
__global__ void k_argmax_sum(const unsigned long long* __restrict__ part, int nblk, int64_t* __restrict__ counts) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  unsigned long long a = 0, b = 0;
  for (int i = threadIdx.x; i < nblk; i += 64) a += part[2 * i], b += part[2 * i + 1];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off, 64), b += __shfl_xor(b, off, 64);
  if (threadIdx.x == 0) counts[0] = static_cast<int64_t>(a), counts[1] = static_cast<int64_t>(b);
}

int col_bits(int c) {
  int bits = 0;
  while ((int64_t{1} << bits) < c) ++bits;
  return bits;
}

struct AucPlan {   // workspace: [keys | sorted keys | rocprim temp]
  size_t keys_a, keys_b, tmp, tmp_bytes, total;
};

int auc_plan(int64_t m, int c, AucPlan* p) {
  const size_t count = static_cast<size_t>(m) * static_cast<size_t>(c);
  size_t sort_bytes = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, sort_bytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                          count, 0u, static_cast<unsigned int>(kColShift + col_bits(c)));
  if (e != hipSuccess) {
    set_error("rocprim::radix_sort_keys size query failed: %s", hipGetErrorString(e));
    return SGF_E_HIP;
  }
  p->tmp_bytes = align_up(sort_bytes, 256) + 256;
  size_t off = 0;
  p->keys_a = off;  off += align_up(count * 8, 256) + 256;
  p->keys_b = off;  off += align_up(count * 8, 256) + 256;
  p->tmp = off;     off += p->tmp_bytes;
  p->total = off;
  return SGF_OK;
}

int check_rows(const char* fn, int64_t ldl, int64_t n, int c, int dtype, int kind, const int64_t* idx, int64_t m) {
  SGF_REQUIRE(n >= 0 && m >= 0 && c >= 1 && ldl >= c, SGF_E_INVALID, "%s: bad sizes n=%lld m=%lld c=%d ldl=%lld", fn,
              static_cast<long long>(n), static_cast<long long>(m), c, static_cast<long long>(ldl));
  SGF_REQUIRE(m < (int64_t{1} << 31), SGF_E_INVALID, "%s: m=%lld rows, the limit is 2^31 - 1", fn, static_cast<long long>(m));
  SGF_REQUIRE(dtype == SGF_F32 || dtype == SGF_BF16, SGF_E_INVALID, "%s: unknown dtype %d", fn, dtype);
  SGF_REQUIRE(kind == SGF_METRIC_TARGET_F32 || kind == SGF_METRIC_TARGET_I64, SGF_E_INVALID, "%s: unknown target kind %d", fn,
              kind);
  SGF_REQUIRE(idx || m == n || m == 0, SGF_E_INVALID, "%s: the dense form (idx == NULL) needs m == n (m=%lld n=%lld)", fn,
              static_cast<long long>(m), static_cast<long long>(n));
  return SGF_OK;
}

}  // namespace
}  // namespace sgf

using namespace sgf;

extern "C" size_t sgf_rocauc_workspace_bytes(int64_t m, int32_t c) {
  if (m <= 0 || c < 1) return 0;
  AucPlan p;
  if (auc_plan(m, c, &p) != SGF_OK) return 0;
  return p.total;
}

extern "C" int sgf_rocauc_counts(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* target,
                                 int64_t ldt, int32_t target_kind, const int64_t* idx, int64_t m, int64_t* counts,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_rows("sgf_rocauc_counts", ldl, n, c, dtype, target_kind, idx, m)) return rc;
  SGF_REQUIRE(ldt >= c, SGF_E_INVALID, "sgf_rocauc_counts: ldt=%lld < c=%d", static_cast<long long>(ldt), c);
  SGF_REQUIRE(c < (1 << 27), SGF_E_INVALID, "sgf_rocauc_counts: c=%d columns, the limit is 2^27 - 1", c);
  SGF_REQUIRE(counts, SGF_E_INVALID, "sgf_rocauc_counts: null counts");
  SGF_REQUIRE(m == 0 || (logits && target), SGF_E_INVALID, "sgf_rocauc_counts: null pointer");
  SGF_REQUIRE(m == 0 || workspace, SGF_E_WORKSPACE, "sgf_rocauc_counts: null workspace");
  hipStream_t st = static_cast<hipStream_t>(stream);
  SGF_CHECK_HIP(hipMemsetAsync(counts, 0, static_cast<size_t>(c) * 6 * sizeof(int64_t), st));
  if (m == 0) return SGF_OK;
  const int nchunk = static_cast<int>((m + kChunk - 1) / kChunk);
  SGF_REQUIRE(static_cast<int64_t>(nchunk) * c < (int64_t{1} << 31), SGF_E_INVALID,
              "sgf_rocauc_counts: m * c = %lld * %d is too large for one launch", static_cast<long long>(m), c);
  AucPlan p;
  if (int rc = auc_plan(m, c, &p)) return rc;
  SGF_REQUIRE(workspace_bytes >= p.total, SGF_E_WORKSPACE, "sgf_rocauc_counts: workspace %zu < %zu", workspace_bytes, p.total);
  char* ws = static_cast<char*>(workspace);
  uint64_t* ka = reinterpret_cast<uint64_t*>(ws + p.keys_a);
  uint64_t* kb = reinterpret_cast<uint64_t*>(ws + p.keys_b);
  const int64_t total = m * c;
  const bool small = total < (int64_t{1} << 31);
  int64_t nb = (total + kThreads * 4 - 1) / (kThreads * 4);
  const int nblk = static_cast<int>(nb > kMaxBlocks ? kMaxBlocks : nb);
#define SGF_AUC_KEYS(T, PTR)                                                                                              \
  do {                                                                                                                    \
    if (target_kind == SGF_METRIC_TARGET_F32)                                                                             \
      hipLaunchKernelGGL((k_auc_keys<T, SGF_METRIC_TARGET_F32>), dim3(nblk), dim3(kThreads), 0, st, PTR, ldl, n, c, target, \
                         ldt, idx, total, small, ka);                                                                     \
    else                                                                                                                  \
      hipLaunchKernelGGL((k_auc_keys<T, SGF_METRIC_TARGET_I64>), dim3(nblk), dim3(kThreads), 0, st, PTR, ldl, n, c, target, \
                         ldt, idx, total, small, ka);                                                                     \
  } while (0)
  if (dtype == SGF_F32)
    SGF_AUC_KEYS(float, static_cast<const float*>(logits));
  else
    SGF_AUC_KEYS(uint16_t, static_cast<const uint16_t*>(logits));
#undef SGF_AUC_KEYS
  SGF_LAUNCH_CHECK();
  const int stages = g_stages.get();
  if (stages == 1) return SGF_OK;
  size_t tb = p.tmp_bytes;
  SGF_CHECK_HIP(rocprim::radix_sort_keys(ws + p.tmp, tb, ka, kb, static_cast<size_t>(total), 0u,
                                         static_cast<unsigned int>(kColShift + col_bits(c)), st));
  if (stages == 2) return SGF_OK;
  hipLaunchKernelGGL(k_auc_rank, dim3(static_cast<unsigned int>(nchunk) * c), dim3(kThreads), 0, st, kb, m, nchunk,
                     reinterpret_cast<unsigned long long*>(counts));
  SGF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_auc_final, dim3((c + kThreads - 1) / kThreads), dim3(kThreads), 0, st, counts, c);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}

extern "C" size_t sgf_argmax_workspace_bytes(int64_t m, int32_t c) {
  (void)m;
  (void)c;
  return static_cast<size_t>(kMaxBlocks) * 2 * sizeof(unsigned long long);
}

namespace {
template <typename T, int LK, int G>
void launch_argmax(const void* logits, int64_t ldl, int64_t n, int c, const void* labels, int64_t lds, const int64_t* idx,
                   int64_t m, unsigned long long* part, int* nblk_out, hipStream_t st) {
  constexpr int kRows = kThreads / G;
  int64_t nb = (m + kRows - 1) / kRows;
  const int nblk = static_cast<int>(nb > kMaxBlocks ? kMaxBlocks : nb);
  *nblk_out = nblk;
  hipLaunchKernelGGL((k_argmax<T, LK, G>), dim3(nblk), dim3(kThreads), 0, st, static_cast<const T*>(logits), ldl, n, c, labels,
                     lds, idx, m, part);
}

template <typename T, int LK>
void launch_argmax_g(int g, const void* logits, int64_t ldl, int64_t n, int c, const void* labels, int64_t lds,
                     const int64_t* idx, int64_t m, unsigned long long* part, int* nblk, hipStream_t st) {
  switch (g) {
    case 1: launch_argmax<T, LK, 1>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
    case 2: launch_argmax<T, LK, 2>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
    case 4: launch_argmax<T, LK, 4>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
    case 8: launch_argmax<T, LK, 8>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
    case 16: launch_argmax<T, LK, 16>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
    case 32: launch_argmax<T, LK, 32>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
    default: launch_argmax<T, LK, 64>(logits, ldl, n, c, labels, lds, idx, m, part, nblk, st); break;
  }
}
}  // namespace

extern "C" int sgf_argmax_count(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* labels,
                                int64_t label_stride, int32_t label_kind, const int64_t* idx, int64_t m, int64_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_rows("sgf_argmax_count", ldl, n, c, dtype, label_kind, idx, m)) return rc;
  SGF_REQUIRE(label_stride >= 1, SGF_E_INVALID, "sgf_argmax_count: label_stride=%lld < 1", static_cast<long long>(label_stride));
  SGF_REQUIRE(counts, SGF_E_INVALID, "sgf_argmax_count: null counts");
  SGF_REQUIRE(m == 0 || (logits && labels), SGF_E_INVALID, "sgf_argmax_count: null pointer");
  SGF_REQUIRE(m == 0 || (workspace && workspace_bytes >= sgf_argmax_workspace_bytes(m, c)), SGF_E_WORKSPACE,
              "sgf_argmax_count: workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (m == 0) {
    SGF_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    return SGF_OK;
  }
  int g = 1;
  while (g < c && g < 64) g <<= 1;
  unsigned long long* part = static_cast<unsigned long long*>(workspace);
  int nblk = 0;
  if (dtype == SGF_F32) {
    if (label_kind == SGF_METRIC_TARGET_F32)
      launch_argmax_g<float, SGF_METRIC_TARGET_F32>(g, logits, ldl, n, c, labels, label_stride, idx, m, part, &nblk, st);
    else
      launch_argmax_g<float, SGF_METRIC_TARGET_I64>(g, logits, ldl, n, c, labels, label_stride, idx, m, part, &nblk, st);
  } else {
    if (label_kind == SGF_METRIC_TARGET_F32)
      launch_argmax_g<uint16_t, SGF_METRIC_TARGET_F32>(g, logits, ldl, n, c, labels, label_stride, idx, m, part, &nblk, st);
    else
      launch_argmax_g<uint16_t, SGF_METRIC_TARGET_I64>(g, logits, ldl, n, c, labels, label_stride, idx, m, part, &nblk, st);
  }
  SGF_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_argmax_sum, dim3(1), dim3(64), 0, st, part, nblk, counts);
  SGF_LAUNCH_CHECK();
  return SGF_OK;
}
