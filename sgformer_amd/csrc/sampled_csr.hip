// sampled_csr.hip — N2 + T1 together: the normalised CSR of a neighbour-sampled batch, and its transpose, straight from what
// the sampler emits (csrc/sampler.hip) instead of from the general edge-list path (csrc/csr.hip).
//
// Reference, per sampled batch (100M/nb-sample.py:27-35 calling 100M/ours.py:72-79 = large/ours.py:26-33 in every
// GraphConvLayer.forward, and large/ours.py:34 under autograd for the transpose): degree + argsort of the batch edge list, and
// torch_sparse's own transposition in the backward.  sgf_csr_build / sgf_csr_transpose run those as a degree histogram, a scan
// and an LSD radix sort of 64-bit (target, source) keys each, and the transpose ends in a symmetry flag the caller reads on
// the host — in the middle of the first backward of every training step.
//
// What the sampler guarantees makes most of that unnecessary.  A batch's edges come hop after hop, in frontier order inside a
// hop, and every node is a frontier node exactly once, so
//   * edge_dst_local is non-decreasing over the whole batch         -> rowptr[j] = lower bound of j in edge_dst_local;
//   * a row has at most max(fanouts) entries                        -> ordering a row = ranking <= max_fanout sources.
// Build (2 launches, sized by the CAPACITIES; the node and edge counts are read on the device from the sampler's `counts`,
// so the entry runs before the batch's one host read):
//   k_rows    : one thread per node — binary search for the row start, a forward walk over the row for its length
//               (= the in-degree); nodes behind the last target (the last hop's nodes: most of a batch) skip the search;
//   k_entries : one thread per sampled edge — its rank among the sources of its row (smaller source first, equal sources in
//               edge order: duplicates are kept) is its slot; val = norm_value (common.h: the IEEE expression of csr.hip).
// Transpose (3 launches + one rocPRIM sort; host-known n / nnz; any CSR whose rows are in ascending source order):
//   sort      : stable LSD radix sort (rocPRIM) of the pairs (source, forward entry number) on the ceil(log2 n) significant
//               bits of the 32-bit source — forward entries are in (target, source) order, so a STABLE sort by source alone
//               leaves them in (source, target) order; 4 + 4 bytes per entry and ~20 key bits instead of 8-byte keys with
//               32 + ~20 bits;
//   k_bounds  : t_rowptr[s] = lower bound of s in the sorted sources (no histogram, no scan);
//   k_gather  : t_colind = the row of the forward entry (binary search in rowptr), t_val = the forward entry's value.
// No atomics in this file's kernels: every output element is written by exactly one thread from its own inputs.  rocPRIM's
// sort counts digits with integer atomics inside, but it is stable, so the result is deterministic whatever the launch
// geometry.  Transposed rows are as long as they come (a popular source): nothing here depends on a row length.
// Integer / latency-bound work on 1e5 .. 1e6 entries; no MFMA.
#include "common.h"

#include <rocprim/rocprim.hpp>

namespace sgf {
namespace {

constexpr int kThreads = 256;
// k_entries ranks a row in O(len^2) loads, so the entry takes the caller's bound on the row length and refuses large ones.
// The bound is advisory inside the kernels: a row longer than it is still placed correctly, only slower.
constexpr int kMaxFanout = 256;

inline int grid_for(int64_t n) {
  int64_t b = (n + kThreads - 1) / kThreads;
  const int64_t cap = static_cast<int64_t>(kNumCU) * 16;   // grid-stride the rest
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return static_cast<int>(b);
}

// first position p in [0, len) with a[p] >= key (len when there is none); a non-decreasing
template <typename T>
__device__ __forceinline__ int64_t lower_bound(const T* __restrict__ a, int64_t len, int64_t key) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (static_cast<int64_t>(a[mid]) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rowptr[0 .. nn], deg[0 .. nn): nn = counts[0], ne = counts[1] (clamped to the capacities the launch was sized for)
__global__ __launch_bounds__(kThreads) void k_rows(const int32_t* __restrict__ dst, const int64_t* __restrict__ counts,
                                                   int64_t node_cap, int64_t edge_cap, int64_t* __restrict__ rowptr,
                                                   int32_t* __restrict__ deg) {
  const int64_t nn = clamp64(counts[0], 0, node_cap), ne = clamp64(counts[1], 0, edge_cap);
  const int64_t last = ne > 0 ? dst[ne - 1] : -1;          // no edge points at a node behind this one
  int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (; j <= nn; j += stride) {
    if (j == nn) { rowptr[j] = ne; continue; }
    if (j > last) { rowptr[j] = ne; deg[j] = 0; continue; }
    const int64_t b = lower_bound(dst, ne, j);
    int64_t e = b;
    while (e < ne && dst[e] == j) ++e;
    rowptr[j] = b;
    deg[j] = static_cast<int32_t>(e - b);
  }
}

// entry i of the edge list -> slot rowptr[t] + (rank of its source inside row t)
__global__ __launch_bounds__(kThreads) void k_entries(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                      const int64_t* __restrict__ counts, int64_t node_cap, int64_t edge_cap,
                                                      const int64_t* __restrict__ rowptr, const int32_t* __restrict__ deg,
                                                      int32_t* __restrict__ colind, float* __restrict__ val) {
  const int64_t nn = clamp64(counts[0], 0, node_cap), ne = clamp64(counts[1], 0, edge_cap);
  int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (; i < ne; i += stride) {
    const int64_t t = dst[i];
    if (t < 0 || t >= nn) continue;                        // (not a sampler's edge list: nothing to place)
    const int64_t b = rowptr[t];
    const int32_t dt = deg[t];
    const int64_t e = b + dt;
    if (i < b || i >= e) continue;                         // (targets not in order: the precondition does not hold)
    const int32_t s = src[i];
    int32_t rank = 0;
    for (int64_t k = b; k < e; ++k) {
      const int32_t sk = src[k];
      rank += (sk < s || (sk == s && k < i)) ? 1 : 0;
    }
    colind[b + rank] = s;
    val[b + rank] = (s >= 0 && s < nn) ? norm_value(dt, deg[s]) : 0.0f;
  }
}

// t_rowptr[0 .. n]: where source s starts in the sorted source array
__global__ __launch_bounds__(kThreads) void k_bounds(const int32_t* __restrict__ sorted_src, int64_t nnz, int64_t n,
                                                     int64_t* __restrict__ t_rowptr) {
  int64_t s = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (; s <= n; s += stride) t_rowptr[s] = s == n ? nnz : lower_bound(sorted_src, nnz, s);
}

// transposed entry q = forward entry order[q]: its column is that entry's row, its value that entry's value
__global__ __launch_bounds__(kThreads) void k_gather(const int32_t* __restrict__ order, const int64_t* __restrict__ rowptr,
                                                     const float* __restrict__ val, int64_t n, int64_t nnz,
                                                     int32_t* __restrict__ t_colind, float* __restrict__ t_val) {
  int64_t q = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kThreads;
  for (; q < nnz; q += stride) {
    const int64_t i = clamp64(order[q], 0, nnz - 1);
    // the row r with rowptr[r] <= i < rowptr[r + 1]: one before the first row that starts behind i (empty rows repeat a start)
    const int64_t r = clamp64(lower_bound(rowptr, n + 1, i + 1) - 1, 0, n - 1);
    t_colind[q] = static_cast<int32_t>(r);
    t_val[q] = val[i];
  }
}

inline unsigned source_bits(int64_t n) {
  unsigned b = 1;
  while ((static_cast<int64_t>(1) << b) < n && b < 31) ++b;
  return b;
}

struct TPlan {        // workspace: [sorted sources | forward entry numbers in sorted order | rocPRIM temp]
  size_t keys, order, tmp, total, tmp_bytes;
};

int t_plan(int64_t n, int64_t nnz, TPlan* p) {
  size_t sort_bytes = 0;
  if (nnz > 0) {
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                                             rocprim::counting_iterator<int32_t>(0), static_cast<int32_t*>(nullptr),
                                             static_cast<size_t>(nnz), 0u, source_bits(n));
    if (e != hipSuccess) {
      set_error("rocprim::radix_sort_pairs size query failed: %s", hipGetErrorString(e));
      return SGF_E_HIP;
    }
  }
  p->tmp_bytes = align_up(sort_bytes, 256) + 256;
  size_t off = 0;
  p->keys = off;   off += align_up(static_cast<size_t>(nnz) * 4, 256);
  p->order = off;  off += align_up(static_cast<size_t>(nnz) * 4, 256);
  p->tmp = off;    off += p->tmp_bytes;
  p->total = off;
  return SGF_OK;
}

}  // namespace
}  // namespace sgf

extern "C" int32_t sgf_sampled_csr_supported(int32_t max_fanout) {
  return max_fanout >= 0 && max_fanout <= sgf::kMaxFanout ? 1 : 0;
}

// the build needs no scratch: every kernel writes the caller's outputs directly
extern "C" size_t sgf_sampled_csr_build_workspace_bytes(int64_t node_cap, int64_t edge_cap) {
  (void)node_cap;
  (void)edge_cap;
  return 0;
}

extern "C" int sgf_sampled_csr_build(const int32_t* edge_src_local, const int32_t* edge_dst_local, const int64_t* counts,
                                     int64_t node_cap, int64_t edge_cap, int32_t max_fanout, int64_t* rowptr_b, int32_t* colind_b,
                                     float* val_b, int32_t* deg_b, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace sgf;
  (void)workspace;
  (void)workspace_bytes;
  SGF_REQUIRE(node_cap >= 0 && edge_cap >= 0 && max_fanout >= 0, SGF_E_INVALID,
              "sgf_sampled_csr_build: negative size (node_cap %lld, edge_cap %lld, max_fanout %d)", static_cast<long long>(node_cap),
              static_cast<long long>(edge_cap), max_fanout);
  SGF_REQUIRE(counts && rowptr_b && deg_b && (edge_cap == 0 || (edge_src_local && edge_dst_local && colind_b && val_b)), SGF_E_INVALID,
              "sgf_sampled_csr_build: null pointer");
  SGF_REQUIRE(node_cap < (int64_t{1} << 31) - 2 && edge_cap < (int64_t{1} << 31) - 2, SGF_E_UNSUPPORTED,
              "sgf_sampled_csr_build: capacities must be < 2^31 - 2");
  SGF_REQUIRE(sgf_sampled_csr_supported(max_fanout), SGF_E_UNSUPPORTED,
              "sgf_sampled_csr_build: max_fanout %d > %d (rows are ranked in place: use sgf_csr_build)", max_fanout, kMaxFanout);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_rows, dim3(grid_for(node_cap + 1)), dim3(kThreads), 0, st, edge_dst_local, counts, node_cap, edge_cap,
                     rowptr_b, deg_b);
  SGF_LAUNCH_CHECK();
  if (edge_cap > 0) {
    hipLaunchKernelGGL(k_entries, dim3(grid_for(edge_cap)), dim3(kThreads), 0, st, edge_src_local, edge_dst_local, counts, node_cap,
                       edge_cap, rowptr_b, deg_b, colind_b, val_b);
    SGF_LAUNCH_CHECK();
  }
  return SGF_OK;
}

extern "C" size_t sgf_sampled_csr_transpose_workspace_bytes(int64_t n, int64_t nnz) {
  if (n < 0 || nnz < 0 || nnz >= (int64_t{1} << 31) - 2) return 0;
  sgf::TPlan p;
  if (sgf::t_plan(n, nnz, &p) != SGF_OK) return 0;
  return p.total;
}

extern "C" int sgf_sampled_csr_transpose(const int64_t* rowptr, const int32_t* colind, const float* val, int64_t n, int64_t nnz,
                                         int64_t* t_rowptr, int32_t* t_colind, float* t_val, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  using namespace sgf;
  SGF_REQUIRE(n >= 0 && nnz >= 0, SGF_E_INVALID, "sgf_sampled_csr_transpose: negative size");
  SGF_REQUIRE(rowptr && t_rowptr && (nnz == 0 || (colind && val && t_colind && t_val)), SGF_E_INVALID,
              "sgf_sampled_csr_transpose: null pointer");
  SGF_REQUIRE(n > 0 || nnz == 0, SGF_E_INVALID, "sgf_sampled_csr_transpose: %lld entries in a graph without nodes",
              static_cast<long long>(nnz));
  SGF_REQUIRE(n < (int64_t{1} << 31) && nnz < (int64_t{1} << 31) - 2, SGF_E_UNSUPPORTED,
              "sgf_sampled_csr_transpose: n and nnz must be < 2^31 (int32 columns and entry numbers)");
  // a workspace that cannot even hold the two entry arrays is refused before any HIP call; the exact size needs rocPRIM's
  // query (t_plan), which may ask the runtime for the device
  const size_t arrays = 2 * align_up(static_cast<size_t>(nnz) * 4, 256) + 256;
  SGF_REQUIRE(workspace && workspace_bytes >= arrays, SGF_E_WORKSPACE, "sgf_sampled_csr_transpose: workspace %zu < %zu", workspace_bytes,
              arrays);
  TPlan p;
  int rc = t_plan(n, nnz, &p);
  if (rc != SGF_OK) return rc;
  SGF_REQUIRE(workspace_bytes >= p.total, SGF_E_WORKSPACE, "sgf_sampled_csr_transpose: workspace %zu < %zu", workspace_bytes, p.total);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  int32_t* keys = reinterpret_cast<int32_t*>(ws + p.keys);
  int32_t* order = reinterpret_cast<int32_t*>(ws + p.order);
  if (nnz > 0) {
    size_t tb = p.tmp_bytes;
    SGF_CHECK_HIP(rocprim::radix_sort_pairs(ws + p.tmp, tb, colind, keys, rocprim::counting_iterator<int32_t>(0), order,
                                            static_cast<size_t>(nnz), 0u, source_bits(n), st));
  }
  hipLaunchKernelGGL(k_bounds, dim3(grid_for(n + 1)), dim3(kThreads), 0, st, keys, nnz, n, t_rowptr);
  SGF_LAUNCH_CHECK();
  if (nnz > 0) {
    hipLaunchKernelGGL(k_gather, dim3(grid_for(nnz)), dim3(kThreads), 0, st, order, rowptr, val, n, nnz, t_colind, t_val);
    SGF_LAUNCH_CHECK();
  }
  return SGF_OK;
}
