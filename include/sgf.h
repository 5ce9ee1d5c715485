/*
 * sgf.h — C ABI of libsgf.so: the MI355X (gfx950) hot path of SGFormer forward/backward.
 *
 * This is the drop-in boundary.  The reference (qitianwu/SGFormer) has no FFI of
 * its own: its hot path is a chain of stock PyTorch / torch_sparse calls inside large/ours.py,
 * medium/ours.py and 100M/ours.py.  Every entry point below names the reference lines whose
 * arithmetic it replaces.  The host-side mirror of the reference's nn.Module surface
 * (sgformer_amd/ours.py) binds these with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / HIP types in any signature
 *     (`stream` is a hipStream_t passed as void*; NULL = the default stream).
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - the caller allocates and owns every buffer, including outputs and workspaces
 *     (sizes from the *_workspace_bytes queries).  No hidden allocation, no host sync,
 *     no per-thread compute state: calls are re-entrant and may come from the autograd thread.
 *   - return value: 0 = ok, negative = error (SGF_E_*); sgf_last_error() gives the text of the
 *     most recent failure ON THE CALLING THREAD (errno-style; valid until that thread's next failure).
 *   - matrices are row-major with an explicit leading dimension `ld*` counted in ELEMENTS.
 *   - dtype codes: SGF_F32 = 0 (fp32 storage), SGF_BF16 = 1 (bf16 storage, fp32 accumulate),
 *     SGF_F32_BF16X3 = 2 (fp32 storage whose matrix products are formed as three bf16 products, see below).
 */
#ifndef SGF_H_
#define SGF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGF_VERSION 671 /* 0.6.17: sgf_spmm_coded_bytes / sgf_spmm_coded_supported / sgf_spmm_code_rows / sgf_spmm_code_values / sgf_spmm_coded, the SpMM gathering lossless 12-bit coded operand rows with the row scale folded into the CSR values (csrc/spmm_coded.hip, csrc/spmm.hip); 0.6.16: sgf_gat_supported / _lap_rows / sgf_gat_scores / _fwd / _bwd_dst / _bwd_src, attention over the stored entries of a CSR (GATConv's edge softmax, block N10, csrc/gat.hip); 0.6.15: sgf_pair_sigmoid_x3_supported / _lap_rows / _fwd / _bwd_q / _bwd_kv and sgf_pair_softmax_x3_supported / _lap_rows / _fwd / _bwd_q / _bwd_kv, the all-pair attention kernels for SGF_F32_BF16X3 (csrc/pair_attn.hip); 0.6.14: sgf_ew_lap_rows, host query for the rows one loop iteration of the capped grid covers in the persistent element-wise, LayerNorm / BatchNorm and loss kernels (csrc/fused.hip); 0.6.13: sgf_pair_softmax_supported / _workspace_bytes / _lap_rows / sgf_pair_softmax_fwd / _bwd_q / _bwd_kv, the exact softmax all-pair attention as tiled products with an online maximum (csrc/pair_attn.hip); 0.6.12: sgf_pair_sigmoid_supported / _workspace_bytes / _lap_rows / sgf_pair_sigmoid_fwd / _bwd_q / _bwd_kv, DIFFormer's all-pair sigmoid attention as tiled products without the n x l score tensor (csrc/pair_attn.hip); 0.6.11: sgf_head_rows_supported / _fwd_workspace_bytes / _bwd_workspace_bytes / sgf_head_rows_fwd / sgf_head_rows_bwd, the head, its cross-entropy and their gradient on the selected (seed) rows of a sampled batch (csrc/head_rows.hip); 0.6.10: sgf_row_lap_rows, host query for the rows one lap of the persistent bf16 row kernels covers (csrc/rowgemm.hip, csrc/head.hip); 0.6.9: sgf_bn_apply_packed / sgf_spmm_packed / sgf_spmm_packed_supported / sgf_spmm_packed_bytes, the forward GCN SpMM gathering zero-elided operand rows (csrc/fused.hip, csrc/spmm.hip); 0.6.8: sgf_spmm_arm / sgf_spmm_blocked_arm, host queries for the kernel a SpMM launch would run; 0.6.7: sgf_attn_max_blocks / sgf_attn_tile_rows, host queries for the grid cap and tile heights of the persistent attention kernels; 0.6.6: sgf_dropout_dev, sgf_dropout with its 64-bit seed read from device memory when the kernel runs (a launch captured into a hipGraph draws a new mask per replay); 0.6.5: sgf_sampled_csr_supported / _build_workspace_bytes / _build / _transpose_workspace_bytes / _transpose, the normalised CSR of a neighbour-sampled batch and its transpose without the edge-list sort (csrc/sampled_csr.hip); 0.6.4: sgf_rocauc_workspace_bytes / sgf_rocauc_counts / sgf_argmax_workspace_bytes / sgf_argmax_count, the evaluation metrics as integer counts (csrc/metrics.hip); 0.6.3: sgf_attn_h_supported; sgf_attn_h_fwd / _bwd_reduce / _bwd_apply take SGF_F32_BF16X3 (csrc/attn_f32x.hip); 0.6.2: sgf_bce_workspace_bytes / sgf_bce_fwd / sgf_bce_bwd, the multi-label loss on the training rows (csrc/bce.hip); 0.6.1: dtype code SGF_F32_BF16X3 (csrc/linear_f32x.hip, csrc/gram_f32x.hip) */

#define SGF_F32 0
#define SGF_BF16 1
/* SGF_F32_BF16X3: fp32 storage (every tensor exactly as for SGF_F32) whose matrix products are formed as three bf16
 * products, a = hi + lo with hi = bf16(a), lo = bf16(a - hi) (round to nearest even; lo = 0 where hi is not finite):
 *     a b ~ hi_a hi_b + hi_a lo_b + lo_a hi_b,  fp32 accumulation,
 * torch.set_float32_matmul_precision('high') ("each float32 number as the sum of two bfloat16 numbers").  Per product the
 * error is at most 3 * 2^-16 |a b|; an inf / NaN input gives a non-finite output wherever SGF_F32 would.  Accepted only
 * by the entries that say so and by their *_supported queries (same shapes as SGF_F32); every other entry rejects it.
 * The all-pair attention (N7, N8) takes it through entries of its own, sgf_pair_*_x3_* (N9), which accept nothing else.
 * Where `dtype` names an output's storage (sgf_combine_fc_bwd: dx1 / dx2), SGF_F32_BF16X3 means fp32 outputs. */
#define SGF_F32_BF16X3 2

#define SGF_OK 0
#define SGF_E_INVALID (-1)   /* bad argument (shape, alignment, dtype)            */
#define SGF_E_WORKSPACE (-2) /* workspace too small                                */
#define SGF_E_HIP (-3)       /* a HIP runtime call or kernel launch failed         */
#define SGF_E_UNSUPPORTED (-4) /* shape outside what the gfx950 kernels implement  */

int sgf_version(void);
const char* sgf_last_error(void);
/* Experiment switches (SGF_* environment variables read by the library) are cached per process; call this after changing
 * one so that it is read again at its next use. */
int sgf_reload_env(void);

/* ------------------------------------------------------------------------------------------
 * T1 — adjacency normalisation + CSR build.   Replaces large/ours.py:26-33
 * (= 100M/ours.py:72-79): degree(col, N); value = sqrt(1/d[col]) * sqrt(1/d[row]);
 * nan_to_num(->0); SparseTensor(row=col, col=row, value) i.e. A[col_e, row_e] = v_e with entries
 * ordered by (target, source), duplicates kept.  In the reference this (an argsort over all nnz
 * edges) is redone in every layer of every forward; here it is built once and cached by the
 * caller.
 *
 *   edge_index : int64 [2, nnz] row-major (edge_index[0] = source "row", edge_index[1] = target "col")
 *   rowptr     : int64 [n+1]   out — CSR row pointer over TARGET nodes
 *   colind     : int32 [nnz]   out — source node of each stored entry, ascending inside a row
 *   val        : fp32  [nnz]   out — sqrtf(1.0f/deg[tgt]) * sqrtf(1.0f/deg[src]), non-finite -> 0
 *   deg        : int32 [n]     out — in-degree (count of edges whose target is i)
 * Bit-exact contract: rowptr / colind equal a stable sort of the edges by key tgt*N+src; val is the
 * IEEE fp32 product of two correctly rounded sqrt(1/d) terms.  Requires 0 <= node id < n < 2^31.
 * ------------------------------------------------------------------------------------------ */
size_t sgf_csr_workspace_bytes(int64_t nnz, int64_t n);
int sgf_csr_build(const int64_t* edge_index, int64_t nnz, int64_t n, int64_t* rowptr,
                  int32_t* colind, float* val, int32_t* deg, void* workspace,
                  size_t workspace_bytes, void* stream);

/* CSR of A^T (needed by the SpMM backward, dX = A^T dY, large/ours.py:34 under autograd, whenever
 * A is not symmetric: neighbour-sampled batches 100M/nb-sample.py:125-133, --directed runs,
 * ogbn-proteins).  `deg` is the in-degree array produced by sgf_csr_build.  `is_symmetric`
 * (int32[1], device) is set to 1 when A^T == A entry for entry, in which case the caller may
 * reuse the forward CSR and drop the transposed arrays. */
int sgf_csr_transpose(const int64_t* edge_index, int64_t nnz, int64_t n, const int32_t* deg,
                      const int64_t* rowptr, const int32_t* colind, int64_t* t_rowptr,
                      int32_t* t_colind, float* t_val, int32_t* is_symmetric, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N1 — induced subgraph of a node subset, the per-mini-batch step of the reference's
 * random-partition trainer.   Replaces torch_geometric.utils.subgraph(idx_i, edge_index, num_nodes=n,
 * relabel_nodes=True) at large/main-batch.py:139 and large/eval.py:94 (third-party PyG 1.7.2, run on
 * the HOST by the reference: an O(E) mask + filter over all edges for every batch):
 *     keep edge e iff both endpoints are in `subset`; kept edges stay in their ORIGINAL ORDER;
 *     with relabel_nodes, node subset[j] becomes j.
 * Two calls around one host read of the output size:
 *     sgf_subgraph_plan : relabel[v] = position of v in subset (-1 = absent; int32 [n], out),
 *                         *total (device int64) = number of kept edges; per-block offsets stay in
 *                         `workspace`, which must be passed unchanged to
 *     sgf_subgraph_emit : out int64 [2, total] (row 0 sources, row 1 targets); out_eid int64 [total]
 *                         (optional, NULL to skip) = position of each kept edge in edge_index, for
 *                         filtering edge attributes.
 * `subset` must hold distinct node ids (the trainer's are slices of a permutation).  Ids outside
 * [0, n) never match.  n < 2^31.
 * ------------------------------------------------------------------------------------------ */
size_t sgf_subgraph_workspace_bytes(int64_t nnz, int64_t n);
int sgf_subgraph_plan(const int64_t* edge_index, int64_t nnz, int64_t n, const int64_t* subset,
                      int64_t m, int32_t* relabel, int64_t* total, void* workspace,
                      size_t workspace_bytes, void* stream);
int sgf_subgraph_emit(const int64_t* edge_index, int64_t nnz, int64_t n, const int32_t* relabel,
                      int32_t relabel_nodes, int64_t total, int64_t* out, int64_t* out_eid,
                      void* workspace, size_t workspace_bytes, void* stream);

/* N1 + T1 in one step (r05; csrc/subgraph_csr.hip): the induced subgraph of `subset` AND its normalised CSR, straight from
 * the CSR of the PARENT graph (sgf_csr_build of the full edge list, cached by the caller) — a batch of m nodes reads its m
 * parent rows (20 MB per 100 k-node batch at ogbn-products size) instead of all parent edges twice (4 GB) plus a radix
 * sort of the result.  Replaces large/main-batch.py:139 + large/ours.py:26-33 for the batch:
 *     rowptr_b int64 [m + 1], colind_b int32 [total], val_b fp32 [total], deg_b int32 [m]  == bit for bit what
 *     sgf_csr_build returns for torch_geometric's subgraph(subset, edge_index, relabel_nodes=True);
 *     edge_index_b int64 [2, total] (optional): that edge list in (target, source) order — the same multiset of edges as
 *     the reference's, whose order (the parent's edge order) no consumer on the path depends on.
 * Two calls around ONE host read:  _plan -> total (int64 [3]): total[0] = number of kept entries, total[1] = 1 if `subset`
 * repeats a node or holds an id outside [0, n) (then call _emit with total = 0, which only resets the table, and use
 * sgf_subgraph_* instead), total[2] = the longest row of the batch CSR (<= sgf_spmm's long-row threshold: sgf_spmm_split is
 * not needed for it); _emit with the value read.  local_of: int32 [n] owned by the caller, all -1 between calls (the library restores it).
 * deg_b has m + 1 slots (the last one is scratch).  Workspaces: _plan_workspace_bytes(m), _emit_workspace_bytes(m, total). */
size_t sgf_subgraph_csr_plan_workspace_bytes(int64_t m);
size_t sgf_subgraph_csr_emit_workspace_bytes(int64_t m, int64_t total);
int sgf_subgraph_csr_plan(const int64_t* rowptr, const int32_t* colind, int64_t n, const int64_t* subset, int64_t m,
                          int32_t* local_of, int64_t* rowptr_b, int32_t* deg_b, int64_t* total, void* workspace,
                          size_t workspace_bytes, void* stream);
int sgf_subgraph_csr_emit(const int64_t* rowptr, const int32_t* colind, int64_t n, const int64_t* subset, int64_t m,
                          int32_t* local_of, const int64_t* rowptr_b, const int32_t* deg_b, int64_t total, int32_t* colind_b,
                          float* val_b, int64_t* edge_index_b, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N2 — the trainer's graph prologue.   Replaces large/main.py:75-79 (and
 * 100M/nb-sample.py:79-80), three torch_geometric 1.7.2 utilities the trainers run on the HOST:
 *     to_undirected      : concatenate both directions, coalesce = sort by row*N+col, drop duplicates
 *     remove_self_loops  : keep entries with row != col, order preserved
 *     add_self_loops     : append (i, i) for i in [0, n)
 * Any subset of the three, applied in that order, selected by the flags.  Two calls around one host
 * read of the output size (as sgf_subgraph_*): _plan leaves the sorted keys / scan in `workspace`
 * and writes *total (device int64); _emit writes out int64 [2, total] (row 0 = edge_index[0]).
 * Without to_undirected the entries keep the caller's order.  n < 2^31, 2 m < 2^32 - 1.
 * ------------------------------------------------------------------------------------------ */
size_t sgf_graph_prologue_workspace_bytes(int64_t m, int64_t n);
int sgf_graph_prologue_plan(const int64_t* edge_index, int64_t m, int64_t n, int32_t to_undirected,
                            int32_t remove_self_loops, int32_t add_self_loops, int64_t* total,
                            void* workspace, size_t workspace_bytes, void* stream);
int sgf_graph_prologue_emit(int64_t m, int64_t n, int32_t to_undirected, int32_t add_self_loops,
                            int64_t total, int64_t* out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * T2 — sum-reduce CSR SpMM.   Replaces torch_sparse.matmul(adj, x) at large/ours.py:34
 * (third-party torch_sparse 0.6.10 spmm, reduce="sum"):  Y[i,:] = sum_e val[e] * X[colind[e],:]
 * for e in [rowptr[i], rowptr[i+1]), accumulated in fp32 in stored order.
 * Backward (dX = A^T dY) is the same call on the transposed CSR (or the same CSR if symmetric).
 *   x : [n_cols, d] dtype, leading dim ldx (n_cols = columns of A = rows of x; when n_cols * ldx * elsize
 *       < 2^32 the row kernel addresses x with 32-bit buffer offsets: 8 instead of 21 instructions per
 *       stored entry);  y : [n_rows, d] dtype, leading dim ldy.
 * d, ldx, ldy must be multiples of 4 elements; x and y aligned to 4 elements.
 * ------------------------------------------------------------------------------------------ */
int sgf_spmm(const int64_t* rowptr, const int32_t* colind, const float* val, const void* x,
             int64_t ldx, int64_t n_cols, void* y, int64_t ldy, int64_t n_rows, int32_t d,
             int32_t dtype, void* stream);

/* sgf_spmm with long rows split across workgroups (power-law graphs: a hub row of 17 k entries walked
 * by ONE wave is a latency-bound tail).  Rows with more than `long_len` stored entries are cut into
 * segments of sgf_spmm_segment_len() entries, each reduced by a whole workgroup into an fp32 partial;
 * a row's partials are then added in segment order (deterministic).  `long_segments` = the number of
 * such segments, sum over rows with len > long_len of ceil(len / segment_len), computed by the caller
 * once per CSR (0 = plain sgf_spmm).  Same result as sgf_spmm up to fp32 summation order. */
int32_t sgf_spmm_segment_len(void);
/* Which kernel the next sgf_spmm / sgf_spmm_split (stream = 0) or sgf_spmm_stream (stream = 1) launch with these operands
 * would run, under the current (cached) SGF_SPMM_KERNEL — a host query, no GPU needed; it calls the launcher's own rule.
 * aligned16: x and y are both 16-byte aligned.  Returns arm | lanes_per_row << 8 with arm 0 = k_spmm_seg_bf16x2 (the
 * stream of bf16 row pairs), 1 = k_spmm_seg, 2 = k_spmm_row, 3 = k_spmm_wave, 4 = k_spmm_sub<lanes_per_row>;
 * lanes_per_row is non-zero only for arm 4.  -1 for an unknown dtype. */
int32_t sgf_spmm_arm(int32_t d, int32_t dtype, int64_t ldx, int64_t ldy, int64_t n_cols, int32_t aligned16,
                     int32_t stream);
size_t sgf_spmm_split_workspace_bytes(int64_t long_segments, int32_t d);
int sgf_spmm_split(const int64_t* rowptr, const int32_t* colind, const float* val, const void* x,
                   int64_t ldx, int64_t n_cols, void* y, int64_t ldy, int64_t n_rows, int32_t d, int32_t dtype,
                   int64_t long_len, int64_t long_segments, void* workspace, size_t workspace_bytes,
                   void* stream);

/* sgf_spmm_split with a PACKED copy of x next to the dense one (bf16, d = 256; written by sgf_bn_apply_packed below).
 * On a graph without locality the launch is bound by the bytes of its gathers, and an operand that is the output of a
 * ReLU holds many exact zeros.  Packed row format: one slot of slot_bytes (384 or 448) per row of x, 128-byte aligned:
 *     bytes [0, 32)  a 256-bit mask, bit c (byte c / 8, bit c % 8) set iff the bf16 bits of column c are not 0x0000
 *                    (-0.0 is a value);
 *     bytes [32, ..) the bf16 values of the set columns in column order, at most (slot_bytes - 32) / 2 = 176 / 208;
 *     the rest zero.  A slot decodes to the dense row bit for bit.
 * `packed` holds sgf_spmm_packed_bytes(n_cols, slot_bytes) bytes (the slots and a tail the kernel may read, never uses);
 * `overflow` (device int32 [1]) is the producer's count of rows with more non-zeros than a slot holds.  The launch reads
 * it ON THE DEVICE: zero -> it gathers the slots (slot_bytes / 512 of the dense bytes), anything else -> the dense rows,
 * all or nothing.  It decodes the same four bf16 per lane and runs the same fp32 FMAs in the same order, so y equals
 * sgf_spmm_split's bit for bit either way.  The slots are gathered only where sgf_spmm_packed_supported answers 1 — the
 * launch would run the wave-per-row kernel (sgf_spmm_arm = 2) on bf16 rows of exactly 256 columns, SGF_SPMM_PACKED != 0
 * (cached switch) — every other launch is sgf_spmm_split's on the dense rows; rows longer than long_len go to the long-row
 * queue as in sgf_spmm_split and are reduced from the dense rows. */
size_t sgf_spmm_packed_bytes(int64_t n, int32_t slot_bytes);
int32_t sgf_spmm_packed_supported(int32_t d, int32_t dtype, int64_t ldx, int64_t ldy, int64_t n_cols, int32_t aligned16,
                                  int32_t slot_bytes);
int sgf_spmm_packed(const int64_t* rowptr, const int32_t* colind, const float* val, const void* x, int64_t ldx,
                    int64_t n_cols, const void* packed, int32_t slot_bytes, const int32_t* overflow, void* y, int64_t ldy,
                    int64_t n_rows, int32_t d, int32_t dtype, int64_t long_len, int64_t long_segments, void* workspace,
                    size_t workspace_bytes, void* stream);

/* sgf_spmm_split with a lossless 12-BIT CODED copy of x next to the dense one (bf16, d = 256).  A bf16 value is
 * s | Ek (8) | m (7).  Per row of x, E = the largest exponent field Ek among its finite non-zero elements (15 if it has
 * none); an element is coded s | e | m with e = Ek - (E - 15) in 1..15, a zero of either sign s | 0 | 0: 256 x 12 bits =
 * 384 bytes, 3 fetch lines where the dense row takes 4.  Placing e in the low four bits of an fp32 exponent field decodes
 * a zero to itself and any other element to a normal float d of [2^-126, 2^-111) with element = d * 2^(E - 15), exactly.
 * A row ESCAPES (is not coded) when an element is subnormal, Inf or NaN or lies more than 14 binades under the largest.
 *   sgf_spmm_code_rows    one pass over x: `coded` (sgf_spmm_coded_bytes(n) bytes, 128-byte aligned) takes the slots,
 *                         scale_u8[r] = E of row r or 255 for an escaped row (its slot is zero bytes), *n_escaped (device
 *                         int32) the number of escaped rows (scale_u8 16-byte aligned).  Slot: dword l (l = 0..63, byte 4 l) holds columns 4l, 4l+1
 *                         and the exponents of 4l+2, 4l+3 — bits 15..0 s0 | e2 | e0 | m0, bits 31..16 s1 | e3 | e1 | m1 —
 *                         and half l (byte 256 + 2 l) bits 7..0 s2 | m2, bits 15..8 s3 | m3.
 *   sgf_spmm_code_values  one pass over the CSR: val_coded[e] = val[e] * 2^(scale_u8[colind[e]] - 15) where val[e] is a
 *                         normal float > 0, the source row is coded and the product is a normal float; else -val[e], the
 *                         ESCAPE TAG (val 0 becomes -0.0).  *n_unsupported (device int32) counts the val[e] with the sign bit set (-0.0 included), which
 *                         the tag cannot mark.  colind, val, val_coded 16-byte aligned.
 *   sgf_spmm_coded        y = A x: an entry with val_coded >= 0 decodes its row from the slot and multiplies by
 *                         val_coded — fmaf(v * 2^s, x * 2^-s, acc) is fmaf(v, x, acc) bit for bit while both factors are
 *                         normal floats — a tagged entry reads the dense row of x and multiplies by |val_coded| = val.
 *                         Same FMAs in the same order as sgf_spmm_split: y is equal bit for bit.  *n_unsupported != 0
 *                         (read ON THE DEVICE) runs the whole launch on x and val.  The slots are gathered only where
 *                         sgf_spmm_coded_supported answers 1 — the launch would run the wave-per-row kernel
 *                         (sgf_spmm_arm = 2) on bf16 rows of exactly 256 columns, slots within 32-bit offsets,
 *                         SGF_SPMM_CODED != 0 (cached switch) — every other launch is sgf_spmm_split's on x and val;
 *                         rows longer than long_len are reduced from x and val as in sgf_spmm_split. */
size_t sgf_spmm_coded_bytes(int64_t n);
int32_t sgf_spmm_coded_supported(int32_t d, int32_t dtype, int64_t ldx, int64_t ldy, int64_t n_cols, int32_t aligned16);
int sgf_spmm_code_rows(const void* x, int64_t ldx, int64_t n, void* coded, uint8_t* scale_u8, int32_t* n_escaped,
                       void* stream);
int sgf_spmm_code_values(const int32_t* colind, const float* val, int64_t nnz, const uint8_t* scale_u8, float* val_coded,
                         int32_t* n_unsupported, void* stream);
int sgf_spmm_coded(const int64_t* rowptr, const int32_t* colind, const float* val, const float* val_coded, const void* x,
                   int64_t ldx, int64_t n_cols, const void* coded, const int32_t* n_unsupported, void* y, int64_t ldy,
                   int64_t n_rows, int32_t d, int32_t dtype, int64_t long_len, int64_t long_segments, void* workspace,
                   size_t workspace_bytes, void* stream);

/* sgf_spmm_split for a CSR whose gathers mostly hit in L2 (a locality-restoring node order, sgf_reorder
 * below).  The vector memory pipe's address rate is per LANE, so bf16 rows (512 B) are then fetched TWO per
 * 16-byte-per-lane load: lanes 0-31 take the row of stream entry 2j, lanes 32-63 the row of entry 2j+1; a
 * wave walks the stored entries of 8 consecutive rows as one stream, the two half-waves keep partial sums of
 * the even / odd positions and are added when a row ends (k_spmm_seg_bf16x2).  Equal to sgf_spmm up to fp32
 * summation order, deterministic.  fp32 storage (already 16 B per lane) and operands beyond 4 GiB run the
 * sgf_spmm kernels.  long_segments = 0: no row is split. */
int sgf_spmm_stream(const int64_t* rowptr, const int32_t* colind, const float* val, const void* x,
                    int64_t ldx, int64_t n_cols, void* y, int64_t ldy, int64_t n_rows, int32_t d, int32_t dtype,
                    int64_t long_len, int64_t long_segments, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * T2 with on-chip reuse: a locality-restoring node order + an LDS-staged row-block SpMM.
 * Same arithmetic as sgf_spmm (large/ours.py:34, torch_sparse.matmul, sum-reduce) — what changes is
 * how often a neighbour row crosses the L2 / HBM boundary.
 *
 * sgf_reorder — a numbering that puts communities next to each other, from the graph alone: two
 *   levels of synchronous label propagation (nodes, then communities over the inter-community edges;
 *   a node adopts the label most of its in-neighbours carry, ties to the smallest), then nodes sorted
 *   by (level-2 label, level-1 community, id).  perm[p] = old id at new position p, inv[v] = new
 *   position of old node v, community[v] (optional, NULL to skip) = level-1 community index of v.
 *   Deterministic.  The caller relabels edge_index with inv and calls sgf_csr_build again; the module
 *   permutes x once on entry and the logits once on exit (everything in between is
 *   permutation-equivariant).  nnz < 2^32.
 *
 * sgf_spmm_plan — for a CSR (rowptr, colind, val) and blocks of `rows_per_block` consecutive rows: the
 *   sources referenced by >= 2 stored entries of a block, at most `lds_rows` of them (most-referenced
 *   first), are listed in sh_cols[sh_ptr[b] .. sh_ptr[b+1]) — the rows block b stages in LDS, slot =
 *   position in that list.  ecode / eval are colind / val with, inside every row, the entries served
 *   from LDS moved to the front (stable) and their code set to 0x80000000 | slot; nlds[row] = their
 *   number.  Rows longer than `long_len` keep plain source ids.  stats (int64[4], device): entries
 *   served from LDS, rows staged (sum over blocks), distinct (block, source) pairs, nnz.
 *   sh_cols must hold ceil(n / rows_per_block) * lds_rows entries.  nnz < 2^32 - 1.
 *
 * sgf_spmm_blocked — Y = A X with that plan: one workgroup per block (rows_per_block / 8 waves), the
 *   staged rows fetched once per block into LDS (144 KiB: lds_rows <= sgf_spmm_lds_rows_len(dtype)
 *   = 288 bf16 / 144 fp32), every other entry gathered as in sgf_spmm.  rows_per_block: multiple of 8,
 *   <= 128; d <= 256.  long_len / long_segments / workspace as for sgf_spmm_split (0 segments = none).
 *   Per row the LDS entries are accumulated first, then the gathered ones, each in ascending source
 *   order: equal to sgf_spmm up to fp32 summation order, deterministic.
 * ------------------------------------------------------------------------------------------ */
size_t sgf_reorder_workspace_bytes(int64_t nnz, int64_t n);
int sgf_reorder(const int64_t* edge_index, int64_t nnz, int64_t n, int32_t iters1, int32_t iters2,
                int32_t* perm, int32_t* inv, int32_t* community, void* workspace, size_t workspace_bytes,
                void* stream);
size_t sgf_spmm_plan_workspace_bytes(int64_t nnz, int64_t n, int32_t rows_per_block);
int sgf_spmm_plan(const int64_t* rowptr, const int32_t* colind, const float* val, int64_t n, int64_t nnz,
                  int32_t rows_per_block, int32_t lds_rows, int64_t long_len, int32_t* ecode, float* eval,
                  int32_t* nlds, int32_t* sh_ptr, int32_t* sh_cols, int64_t* stats, void* workspace,
                  size_t workspace_bytes, void* stream);
int32_t sgf_spmm_lds_rows_len(int32_t dtype);
/* Which row-block kernel the next sgf_spmm_blocked launch with these operands would run, under the current (cached)
 * SGF_SPMM_BLK2 (host query; the launcher's own rule): 0 = k_spmm_blk2 (bf16, two entries per instruction), 1 / 2 =
 * k_spmm_blk in its lean / deep register budget.  aligned16: x and y both 16-byte aligned.  -1 for an unknown dtype or a
 * rows_per_block / lds_rows that sgf_spmm_blocked rejects. */
int32_t sgf_spmm_blocked_arm(int32_t d, int32_t dtype, int64_t ldx, int64_t ldy, int64_t n_rows, int32_t rows_per_block,
                             int32_t lds_rows, int32_t aligned16);
int sgf_spmm_blocked(const int64_t* rowptr, const int32_t* ecode, const float* eval, const int32_t* nlds,
                     const int32_t* sh_ptr, const int32_t* sh_cols, const void* x, int64_t ldx, void* y,
                     int64_t ldy, int64_t n_rows, int32_t d, int32_t dtype, int32_t rows_per_block,
                     int32_t lds_rows, int64_t long_len, int64_t long_segments, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * T2 on a re-ordered graph, the matrix-core form (csrc/spmm_tile.hip).   Same product as sgf_spmm
 * (large/ours.py:34, torch_sparse.matmul, sum-reduce); bf16 storage, d = 128 or 256.
 * After sgf_reorder a community is a run of consecutive rows whose entries mostly point back into
 * the run: the diagonal blocks of A are 15-60 % dense.  Per block of <= 256 rows the sources that at
 * least `min_count` of the block's entries reference are STAGED (their rows of X pass once per block
 * through LDS) and the block's entries towards them are multiplied as a dense tile on the matrix
 * cores (value = hi + lo bf16, relative error <= 2^-17; products of bf16 values are exact in fp32,
 * fp32 accumulation); every other entry keeps its CSR form and is gathered; a row's two parts are
 * added in fp32 and rounded to bf16 once.  Deterministic.  Non-finite values of X spread inside a
 * block (0 x inf through the tile's zero cells).
 *
 * sgf_spmm_tile_blocks — block boundaries from the level-1 communities of sgf_reorder:
 *   comm_sorted[p] = community of the row at NEW position p (device; NULL = fixed blocks of max_rows).
 *   Runs of one community are packed greedily: consecutive runs share a block while they fit
 *   max_rows (a multiple of 32, <= 256); a longer run is cut into ceil(len / max_rows) pieces of
 *   min(max_rows, round_up(ceil(len / pieces), 32)) rows.  blk_row (device, int32[blk_cap + 1]) gets
 *   nb + 1 boundaries, *nb_out (host) the count (SGF_E_WORKSPACE with *nb_out set when blk_cap is too
 *   small; 4 n / max_rows + 4 always suffices).  Synchronises the stream (one device -> host copy of n ints).
 * sgf_spmm_tile_plan — for a CSR and those blocks: per block the <= cap (multiple of 32, <= 1024)
 *   most-referenced sources with >= min_count references, most-referenced first, ties to the smaller id,
 *   padded to a multiple of 32 with the block's first row: sh_cols[sh_ptr[b] .. sh_ptr[b+1]), slot =
 *   position (sh_cols must hold nb * cap entries).  ecode / eval / nlds as sgf_spmm_plan (tile entries
 *   first in every row, code 0x80000000 | slot).  tile_ptr[b] (int64[nb + 1]) = first 2 KiB fragment of
 *   block b, ceil(rows / 32) * (slots / 16) fragments per block; rem_rowptr (int64[n + 1]) = row
 *   pointers of the entries left on the gather path, every row's share padded to an EVEN count (the
 *   padding repeats the row's last source with value 0: the kernel fetches two rows of X per instruction
 *   and no pair straddles two target rows).  Rows longer than long_len stay entirely on it.
 *   stats (int64[8], device): tile entries, staged rows incl. padding, distinct (block, source) pairs,
 *   nnz, fragments, gathered entries incl. padding, 0, 1 if a block has 0 or more than 256 rows (plan unusable).
 * sgf_spmm_tile_fill — the arrays whose size the plan determines: tiles (n_frag * 2048 bytes; fragment
 *   of chunk q = slot / 32, row tile t, k-step s = (slot / 16) % 2 at tile_ptr[b] + (q * T + t) * 2 + s;
 *   inside: [hi: 64 lanes x 8 bf16][lo: 64 lanes x 8 bf16], lane = (row % 32) + 32 * ((slot % 16) / 8),
 *   element slot % 8 — the A operand of v_mfma_f32_32x32x16_bf16; duplicate edges are summed in fp32 in
 *   stored order), rem_col / rem_val (stats[5] entries, stored order + padding).
 * sgf_spmm_tile_pack_layout / sgf_spmm_tile_pack — the fragments in the form the kernel streams them (the kernel is
 *   bound by fabric traffic, and a 2 KiB fragment costs its 2 KiB whether 5 or 500 of its 512 cells are occupied;
 *   on a community graph 10-25 % are).  A GROUP = the two fragments (k-steps) one wave multiplies per chunk, numbered
 *   wave-major: g = tile_ptr[b] / 2 + t * Q_b + q (row tile t, chunk q, Q_b chunks in block b).  grp[2 g + 1] = its
 *   occupied cells if there are at most sgf_spmm_tile_sparse_len() (sparse), else -1 (dense); grp[2 g] = its offset
 *   in the pool in 16-byte units.  Sparse: the occupied cells as 8-byte entries {byte offset of the cell's hi element
 *   in the 4 KiB [k-step][hi, lo][lane][8] image, hi | lo << 16}, in image order, padded with a zero entry to an even
 *   count; dense: the 4 KiB image.  _layout writes grp and *pool_units (device); the caller allocates
 *   pool_units * 16 + 4096 bytes (the kernel fetches whole KiB) and calls _pack.  n_frag = tile_ptr[nb].
 *   The dense fragments are not needed afterwards.
 * sgf_spmm_tile — Y = A X with that plan; block_rows = the max_rows the blocks were made with (<= 128: four
 *   waves per block and two blocks per CU, else eight waves and one).  x: [n_cols, d] bf16, n_cols * ldx * 2 < 2^32; ldx, ldy
 *   multiples of 8, x / y 16-byte aligned.  long_len / long_segments / workspace as for sgf_spmm_split,
 *   counted on the REMAINDER row lengths (0 segments = no row is split).
 * ------------------------------------------------------------------------------------------ */
int sgf_spmm_tile_supported(int32_t d, int32_t dtype);
int sgf_spmm_tile_blocks(const int32_t* comm_sorted, int64_t n, int32_t max_rows, int32_t* blk_row,
                         int64_t blk_cap, int64_t* nb_out, void* stream);
size_t sgf_spmm_tile_plan_workspace_bytes(int64_t nnz, int64_t n, int64_t nb);
int sgf_spmm_tile_plan(const int64_t* rowptr, const int32_t* colind, const float* val, int64_t n, int64_t nnz,
                       const int32_t* blk_row, int64_t nb, int32_t cap, int32_t min_count, int64_t long_len,
                       int32_t* ecode, float* eval, int32_t* nlds, int32_t* sh_ptr, int32_t* sh_cols,
                       int64_t* tile_ptr, int64_t* rem_rowptr, int64_t* stats, void* workspace,
                       size_t workspace_bytes, void* stream);
int sgf_spmm_tile_fill(const int64_t* rowptr, const int32_t* ecode, const float* eval, const int32_t* nlds,
                       int64_t n, int64_t nnz, const int32_t* blk_row, int64_t nb, const int64_t* tile_ptr,
                       int64_t n_frag, const int64_t* rem_rowptr, void* tiles, int32_t* rem_col, float* rem_val,
                       void* stream);
int32_t sgf_spmm_tile_sparse_len(void);
size_t sgf_spmm_tile_pack_workspace_bytes(int64_t n_frag);
int sgf_spmm_tile_pack_layout(const int32_t* blk_row, int64_t nb, const int64_t* tile_ptr, const void* tiles,
                              int64_t n_frag, int32_t* grp, int64_t* pool_units, void* workspace,
                              size_t workspace_bytes, void* stream);
int sgf_spmm_tile_pack(const int32_t* blk_row, int64_t nb, const int64_t* tile_ptr, const void* tiles, int64_t n_frag,
                       const int32_t* grp, void* pool, int64_t pool_units, void* stream);
int sgf_spmm_tile(const int32_t* blk_row, int64_t nb, int32_t block_rows, const int32_t* sh_ptr, const int32_t* sh_cols,
                  const int64_t* tile_ptr, const int32_t* grp, const void* pool, const int64_t* rem_rowptr,
                  const int32_t* rem_col, const float* rem_val, const void* x, int64_t ldx, int64_t n_cols, void* y, int64_t ldy,
                  int64_t n_rows, int32_t d, int32_t dtype, int64_t long_len, int64_t long_segments,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N2 — layer-wise neighbour sampling on the device.   Replaces NeighborLoader(data,
 * num_neighbors=[15, 10, 5], ...) of 100M/nb-sample.py:125-151 (third-party pyg-lib / torch_sparse
 * neighbor_sample, replace=False, directed=True).  Hop h gives every node that ENTERED the batch in
 * hop h-1 (the seeds for h = 0) min(in-degree, fanout) of its in-neighbours, drawn without
 * replacement (fanout < 0: all of them; Floyd's subset sampling up to 32, selection sampling above); a neighbour not yet in the batch gets
 * the next local id in order of first appearance (so the seeds are rows [0, batch_size): the trainer
 * slices [:batch_size], 100M/nb-sample.py:29-30); sampled edges point neighbour -> node, in local ids.
 * The reference's random stream cannot be matched; the draw is a counter-based hash of
 * (seed, batch, hop, node id): reproducible and independent of the launch geometry.
 *   rowptr / colind : CSR over TARGET nodes (sgf_csr_build): colind[rowptr[v] .. rowptr[v+1]) = the
 *                     in-neighbours of v
 *   local_of        : int32[n_nodes] state, INT32_MIN = node not in the batch (fill it once);
 *                     sgf_neighbor_sample_mark sets local_of[ids[j]] = base + j (seeds: base 0) or INT32_MIN
 *                     (base < 0: reset after the batch)
 *   frontier        : the m nodes that entered in the previous hop, global ids, local ids
 *                     frontier_local0 .. frontier_local0 + m - 1;  n_known = nodes in the batch so far
 *   out             : edge_src_local / edge_dst_local / src_global [edge_cap >= m * fanout], new_nodes
 *                     (global ids of the nodes that entered, in local-id order), counts (device int64[2]:
 *                     edges, new nodes).  Synchronises the stream once (the edge count sizes the launches).
 * ------------------------------------------------------------------------------------------ */
size_t sgf_neighbor_sample_workspace_bytes(int64_t m, int64_t edge_cap);
int sgf_neighbor_sample_mark(int32_t* local_of, const int32_t* ids, int64_t count, int32_t base, void* stream);
int sgf_neighbor_sample_hop(const int64_t* rowptr, const int32_t* colind, const int32_t* frontier, int64_t m,
                            int32_t frontier_local0, int32_t fanout, uint64_t seed, uint64_t batch, int32_t hop,
                            int32_t* local_of, int32_t n_known, int64_t edge_cap, int32_t* edge_src_local,
                            int32_t* edge_dst_local, int32_t* src_global, int32_t* new_nodes, int64_t* counts,
                            void* workspace, size_t workspace_bytes, void* stream);

/* A whole batch — every hop of it — WITHOUT a host read (fan-outs >= 0): the frontier size, the local-id base and the output
 * offsets of every hop stay in device memory, the launches are sized for the capacities
 *   frontier_0 = batch_size, edges_h = frontier_h * fanout_h, frontier_{h+1} = edges_h
 * (sgf_neighbor_sample_batch_workspace_bytes also returns them: node_cap = batch_size + sum edges_h, edge_cap = sum edges_h;
 * 0 bytes = a negative fan-out or more than 2^31 - 2 entries: not supported).  Same draws, same local ids, same edge order as
 * sgf_neighbor_sample_mark + one sgf_neighbor_sample_hop per hop + the un-marking, bit for bit.
 *   nodes  : out, int32[node_cap] global ids in local-id order (seeds first)
 *   edge_* : out, int32[edge_cap] local ids, hop after hop
 *   counts : out, device int64[2 + 2 * hops] = { nodes, edges, edges of hop 0, nodes entered in hop 0, ... } — the ONE read the
 *            caller needs to size its views.  local_of is back to INT32_MIN for every node of the batch on return. */
size_t sgf_neighbor_sample_batch_workspace_bytes(int64_t batch_size, const int32_t* fanouts, int32_t hops, int64_t* node_cap,
                                                  int64_t* edge_cap);
int sgf_neighbor_sample_batch(const int64_t* rowptr, const int32_t* colind, const int32_t* seeds, int64_t batch_size,
                              const int32_t* fanouts, int32_t hops, uint64_t seed, uint64_t batch, int32_t* local_of,
                              int32_t* nodes, int64_t node_cap, int32_t* edge_src_local, int32_t* edge_dst_local,
                              int64_t edge_cap, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N2 + T1 — the normalised CSR of a neighbour-sampled batch, and its transpose, from what the sampler emits
 * (csrc/sampled_csr.hip).   Replaces 100M/ours.py:72-79 (= large/ours.py:26-33) for the batch — the degree + argsort every
 * GraphConvLayer.forward redoes — and, for the transpose, large/ours.py:34 under autograd (torch_sparse transposes the
 * adjacency in the backward of matmul).  sgf_csr_build / sgf_csr_transpose do the same for ANY edge list with two radix sorts
 * of 64-bit keys and a symmetry flag read on the host; a sampled batch needs neither.
 *
 * sgf_sampled_csr_build (100M/ours.py:72-79 = large/ours.py:26-33): runs BEFORE the batch's one host read.
 *   edge_src_local / edge_dst_local : int32 [edge_cap], what sgf_neighbor_sample_batch wrote
 *   counts     : the device array sgf_neighbor_sample_batch wrote; counts[0] = nn (nodes), counts[1] = ne (edges), read on
 *                the device — launches are sized by node_cap / edge_cap
 *   rowptr_b   : int64 [node_cap + 1], colind_b int32 [edge_cap], val_b fp32 [edge_cap], deg_b int32 [node_cap + 1]   out
 * Contract: rowptr_b[:nn + 1], colind_b[:ne], val_b[:ne], deg_b[:nn] == bit for bit what sgf_csr_build returns for the edge
 * list (edge_src_local[:ne], edge_dst_local[:ne]) with n = nn: entries ordered by (target, source), duplicates kept,
 * val = the IEEE fp32 product of two correctly rounded sqrtf(1.0f / deg) terms, non-finite -> 0 (the nodes that entered in the
 * last hop have in-degree 0).  Nothing is written behind those prefixes.
 * Precondition (what the sampler guarantees: edges hop after hop, frontier order inside a hop, every node a frontier node
 * once): edge_dst_local[:ne] is non-decreasing and no row is longer than max_fanout.  rowptr is then a lower bound into
 * edge_dst_local and a row is ordered by ranking its <= max_fanout sources.  Entries that break the precondition are dropped,
 * never written out of bounds.
 * sgf_sampled_csr_supported(max_fanout): 1 for 0 <= max_fanout <= 256 (a row is ranked in O(len^2)), else 0 — there
 * sgf_sampled_csr_build returns SGF_E_UNSUPPORTED and the caller keeps sgf_csr_build.  Inside the kernels max_fanout is
 * advisory: a row longer than it is still ordered correctly, only in more time.
 * No radix sort, no atomics, no host synchronisation, no hidden allocation (the workspace query returns 0: `workspace` may
 * be NULL); deterministic whatever the launch geometry.
 *
 * sgf_sampled_csr_transpose (large/ours.py:34 under autograd: dX = A^T dY): host-known n / nnz, called lazily at the first
 * backward, for any CSR whose rows are in ascending source order.
 *   t_rowptr int64 [n + 1], t_colind int32 [nnz], t_val fp32 [nnz] == bit for bit the t_rowptr / t_colind / t_val of
 *   sgf_csr_transpose for the same graph: entries ordered by (source, target), the value that of the forward entry.
 * A stable sort of (source, forward entry number) pairs by the ceil(log2 n) significant bits of the 32-bit source (rocPRIM
 * LSD radix sort: a counting sort per digit) — forward entries are already in target order, so stability IS the order
 * inside a transposed row, however long that row is; t_rowptr = lower bounds into the sorted sources.  No 64-bit keys, no
 * atomics in the library's own kernels (rocPRIM's sort counts digits with integer atomics; it is stable, so the result is
 * deterministic), no symmetry test and no host read: the caller treats the batch graph as not symmetric (if it happens to
 * be, the transposed arrays equal the forward ones).  A workspace too small for the two entry arrays (8 bytes per entry) is
 * refused before any HIP call; the exact size check follows rocPRIM's size query.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_sampled_csr_supported(int32_t max_fanout);
size_t sgf_sampled_csr_build_workspace_bytes(int64_t node_cap, int64_t edge_cap);
int sgf_sampled_csr_build(const int32_t* edge_src_local, const int32_t* edge_dst_local, const int64_t* counts,
                          int64_t node_cap, int64_t edge_cap, int32_t max_fanout, int64_t* rowptr_b, int32_t* colind_b,
                          float* val_b, int32_t* deg_b, void* workspace, size_t workspace_bytes, void* stream);
size_t sgf_sampled_csr_transpose_workspace_bytes(int64_t n, int64_t nnz);
int sgf_sampled_csr_transpose(const int64_t* rowptr, const int32_t* colind, const float* val, int64_t n, int64_t nnz,
                              int64_t* t_rowptr, int32_t* t_colind, float* t_val, void* workspace, size_t workspace_bytes,
                              void* stream);

/* dst[i, :] = src[idx[i], :] with an optional fp32 <-> bf16 storage change.  Replaces the row
 * gathers at the module boundary: x[idx_i] of a mini-batch (large/main-batch.py:138) and the
 * x[perm] / logits[inv] pair around a re-ordered graph.  idx: int32 or int64 (idx_is_int64) device
 * array of n_out row numbers; numbers outside [0, n_src) give zero rows.  Any d. */
int sgf_gather_rows(const void* src, int64_t lds, int32_t src_dtype, int64_t n_src, const void* idx,
                    int32_t idx_is_int64, int64_t n_out, int32_t d, void* dst, int64_t ldd,
                    int32_t dst_dtype, void* stream);
/* The same copy for feature widths that are not a multiple of 4 (pokec f = 65, Cora f = 1433; large/ours.py:77,:198 read x
 * as it comes): dst[i, :d] = src[idx ? idx[i] : i, :d], dst[i, d:d_pad] = 0, with the same optional storage change.  idx may
 * be NULL (identity).  Done once per feature tensor at the module entry; the stems then run on the aligned kernels with
 * zero-padded weight columns. */
int sgf_pad_rows(const void* src, int64_t lds, int32_t src_dtype, int64_t n_src, const void* idx, int32_t idx_is_int64,
                 int64_t n_out, int32_t d, int32_t d_pad, void* dst, int64_t ldd, int32_t dst_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * T3 — linear global attention core.   Replaces large/ours.py:130-149,157
 * (= medium/ours.py:14-46 full_attention_conv, 100M/ours.py:12-53), per head h:
 *     qn = Q/||Q||_F ; kn = K/||K||_F            (Frobenius norms over the WHOLE [N,H,d] tensors)
 *     S = kn^T V ; z = sum_l kn_l ; num = qn S + N V ; den = qn z + N ; out = mean_h(num/den)
 * The library never writes normalised copies of Q/K: it reduces the un-normalised partials
 *     stats = [ S0 = K^T V  (H*d*d) | z0 = sum_l K_l (H*d) | ssq_q | ssq_k ]       (fp32)
 * in one streaming pass (sgf_attn_fwd_reduce), which is also exactly the buffer a node-sharded
 * multi-GPU run all-reduces, and applies them in a second pass
 * (sgf_attn_fwd_apply) with  c = 1/(||Q|| ||K||):
 *     den_n = c * Q_n.z0 + Ntot ;  out_n = (1/H) sum_h (c * Q_n S0 + Ntot * V_n) / den_n
 *
 *   q,k  : [n, H, d] (leading dims ldq/ldk >= H*d);   v : [n, Hv, d], Hv = H or 1 (Hv = 1 is the
 *          use_weight=False broadcast of large/ours.py:128,138)
 *   stats: fp32 [H*d*d + H*d + 2]  (sgf_attn_stats_len)
 *   n_total : the N that appears in num/den (global node count when node-sharded)
 *   den  : fp32 [n, H] out (saved for backward);  o_heads : [n, H, d] per-head outputs, required
 *          (non-NULL) when H > 1, ignored when H == 1 (then o == out).
 * Supported: d % 4 == 0 and d <= 256 (all reference recipes use 64 / 128 / 256).
 * ------------------------------------------------------------------------------------------ */
int64_t sgf_attn_stats_len(int32_t heads, int32_t d);
size_t sgf_attn_workspace_bytes(int64_t n, int32_t heads, int32_t d);
/* Geometry of the persistent row kernels behind the sgf_attn_* / sgf_attn_h_* entries (host queries, no GPU needed): a launch
 * has at most sgf_attn_max_blocks() workgroups, and workgroup b walks the row tiles b, b + grid, ... of
 * sgf_attn_tile_rows(kind, d, dtype) rows each; kind 0 = the reduce kernels (sgf_attn_fwd_reduce / _bwd_reduce /
 * _h_bwd_reduce, sgf_gram's own kernel), kind 1 = the apply kernels.  d is padded to 64 / 128 / 256; dtype SGF_F32 or SGF_BF16.
 * -1 for an unknown kind, width or dtype.  (bf16 sgf_attn_h_fwd / _h_bwd_apply at d in {64, 128, 256} with 16-byte rows run
 * csrc/rowgemm.hip instead: 32-row tiles per WAVE.) */
int32_t sgf_attn_max_blocks(void);
int32_t sgf_attn_tile_rows(int32_t kind, int32_t d, int32_t dtype);

int sgf_attn_fwd_reduce(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                        int64_t ldv, int64_t n, int32_t heads, int32_t v_heads, int32_t d,
                        int32_t dtype, float* stats, void* workspace, size_t workspace_bytes,
                        void* stream);

int sgf_attn_fwd_apply(const void* q, int64_t ldq, const void* v, int64_t ldv, int64_t n,
                       double n_total, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype,
                       const float* stats, void* out, int64_t ldo, float* den, void* o_heads,
                       void* stream);

/* Backward of the above (hand-derived), given g = dL/dout [n, d]:
 *     dnum = (g/H)/den ; dden = -((g/H).o)/den                              (row-local)
 *     bstats = [ dS0 = sum_n Q_n^T dnum_n (H*d*d) | dz0 = sum_n Q_n dden_n (H*d) ]   (fp32)
 * (sgf_attn_bwd_reduce; again the all-reduce payload when node-sharded), then with
 *     s = c * (<S0,dS0> + <z0,dz0>)        (= <qn,dqn> = <kn,dkn>, both radial terms)
 *     dQ = c (dnum S0^T + dden z0) - s Q/||Q||^2
 *     dK = c (V dS0^T + dz0)       - s K/||K||^2
 *     dV = Ntot dnum + c K dS0                       (summed over heads when Hv == 1)
 * (sgf_attn_bwd_apply).  `o` is o_heads when H > 1 and `out` when H == 1.
 * bstats has H*d*d + H*d + 1 floats: the last slot is zeroed by sgf_attn_bwd_reduce (so the whole
 * buffer can be all-reduced) and filled with <S0,dS0> + <z0,dz0> by sgf_attn_bwd_apply. */
int64_t sgf_attn_bstats_len(int32_t heads, int32_t d);

int sgf_attn_bwd_reduce(const void* q, int64_t ldq, const void* g, int64_t ldg, const void* o,
                        int64_t ldo, const float* den, int64_t n, int32_t heads, int32_t d,
                        int32_t dtype, float* bstats, void* workspace, size_t workspace_bytes,
                        void* stream);

int sgf_attn_bwd_apply(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                       int64_t ldv, const void* g, int64_t ldg, const void* o, int64_t ldo,
                       const float* den, int64_t n, double n_total, int32_t heads,
                       int32_t v_heads, int32_t d, int32_t dtype, const float* stats,
                       float* bstats, void* dq, int64_t lddq, void* dk, int64_t lddk,
                       void* dv, int64_t lddv, void* stream);
/* The same two calls for PER-HEAD output gradients: full_attention_conv returns [N, H, D] (medium/ours.py:14-46,
 * 100M/ours.py:12-53) and a caller may differentiate through the heads before any mean.  g: [n, H, d] (ldg >= H * d); head h's
 * gradient enters as it is (no 1/H).  H = 1 coincides with sgf_attn_bwd_reduce / _apply. */
int sgf_attn_bwd_reduce_heads(const void* q, int64_t ldq, const void* g, int64_t ldg, const void* o, int64_t ldo,
                              const float* den, int64_t n, int32_t heads, int32_t d, int32_t dtype, float* bstats,
                              void* workspace, size_t workspace_bytes, void* stream);
int sgf_attn_bwd_apply_heads(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* g,
                             int64_t ldg, const void* o, int64_t ldo, const float* den, int64_t n, double n_total,
                             int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, const float* stats, float* bstats,
                             void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, void* stream);

/* ------------------------------------------------------------------------------------------
 * T3 + T4 fused — attention straight from the un-projected layer input (H = 1, query == source:
 * every recipe of the reference).  Replaces large/ours.py:123-157 as a whole: the projections
 * Q = h Wq^T + bq, K = h Wk^T + bk, V = h Wv^T + bv are never materialised.  Because the attention
 * only needs K^T V, sum K, ||Q||, ||K|| and Q applied to d x d matrices, everything global follows
 * from the Gram matrix G = h^T h and s = sum_n h_n (sgf_gram(h, h) with its column sums):
 *     S0 = Wk G Wv^T + (Wk s) bv^T + bk (Wv s)^T + N bk bv^T        z0 = Wk s + N bk
 *     ||Q||^2 = tr(Wq G Wq^T) + 2 bq.(Wq s) + N |bq|^2   (same for K)    c = 1 / (||Q|| ||K||)
 *     num = h M + m,  M = c Wq^T S0 + Ntot Wv^T,  m = c bq S0 + Ntot bv
 *     den = h.w + beta,  w = c Wq^T z0,  beta = c bq.z0 + Ntot            out = num / den
 * The d x d algebra (M, m, w, beta and its backward) is a handful of tiny fp32 GEMMs done by the
 * caller (sgformer_amd/ops.py, on device, autograd); the library streams the [N, d] operands:
 *     sgf_attn_h_fwd        : out = (h M + m) / (h.w + beta), den saved            (reads h once)
 *     sgf_attn_h_bwd_reduce : hstats = [ dM = sum h^T dnum | dw = sum h dden | dm = sum dnum |
 *                             dbeta = sum dden ],  dnum = g/den, dden = -(g.out)/den
 *     sgf_attn_h_bwd_apply  : dh = dnum M^T + dden w + h D + ds   with D = dG + dG^T, ds from the
 *                             caller's backward through the d x d algebra
 * HBM traffic per layer: 3 [N,d] passes forward, 9 backward — against ~31 for the materialised
 * Q/K/V form (projection GEMM + its dX / dW, two reduce and four apply passes).  Node-sharded runs
 * all-reduce [G | s] and hstats (d^2 + d and d^2 + 2d + 1 floats).
 * M, D: fp32 [d, d] row-major (M[k][j]: input feature k -> output feature j); m, w, ds: fp32 [d];
 * beta: fp32 [1]; all DEVICE pointers.  d % 4 == 0, d <= 256.
 * These three entries accept SGF_F32_BF16X3 (sgf_attn_h_supported): h M, dnum M^T, h D and h^T dnum are then formed as
 * three bf16 products; the row dots h.w and g.out, 1 / den, dnum, dden, the vector sums of hstats and the vectors m, w, ds
 * stay exact fp32 (den is the SGF_F32 value up to summation order).  Same tensors, same workspaces as SGF_F32.
 * ------------------------------------------------------------------------------------------ */
int64_t sgf_attn_h_bstats_len(int32_t d);
/* 1 where sgf_attn_h_fwd / _bwd_reduce / _bwd_apply run head dim `d` under dtype code `dtype`, else 0 (host query) */
int32_t sgf_attn_h_supported(int32_t d, int32_t dtype);
int sgf_attn_h_fwd(const void* h, int64_t ldh, int64_t n, int32_t d, int32_t dtype, const float* M,
                   const float* m, const float* w, const float* beta, void* out, int64_t ldo,
                   float* den, void* stream);
int sgf_attn_h_bwd_reduce(const void* h, int64_t ldh, const void* g, int64_t ldg, const void* o,
                          int64_t ldo, const float* den, int64_t n, int32_t d, int32_t dtype,
                          float* hstats, void* workspace, size_t workspace_bytes, void* stream);
int sgf_attn_h_bwd_apply(const void* h, int64_t ldh, const void* g, int64_t ldg, const void* o,
                         int64_t ldo, const float* den, int64_t n, int32_t d, int32_t dtype,
                         const float* M, const float* w, const float* D, const float* ds, void* dh,
                         int64_t lddh, void* workspace, size_t workspace_bytes, void* stream);
/* scratch of sgf_attn_h_bwd_apply: bf16 storage with d in {64, 128, 256} runs as two per-wave streaming passes
 * (csrc/rowgemm.hip) with the first product parked in the matrix cores' accumulator layout; 0 otherwise (fp32 storage
 * under either code needs none) */
size_t sgf_attn_h_bwd_apply_workspace_bytes(int64_t n, int32_t d, int32_t dtype);
/* The same backward as three calls (bf16 storage, d in {64, 128, 256}: sgf_attn_h_bwd_split_supported), ordered so that
 * the node reduction can use what the first apply pass computes anyway:
 *   sgf_attn_h_bwd_pre            : partial (in `workspace`, sgf_attn_h_bwd_apply_workspace_bytes) = dnum M^T + dden w,
 *                                   and rowscal[n][2] = (1 / den, dden = -(g . out) / den) per node;
 *   sgf_attn_h_bwd_reduce_scaled  : hstats as sgf_attn_h_bwd_reduce, from h, g and rowscal — two streams instead of
 *                                   three (no `out`, no per-row dot);
 *   sgf_attn_h_bwd_post           : dh = h D + ds + partial [+ addend].  `addend` (nullable, storage dtype, leading
 *                                   dim ldadd): a second gradient of h — the residual branch's, large/ours.py:206-208 uses
 *                                   the layer input twice — added to the rounded result here instead of in a separate
 *                                   three-tensor pass.
 * sgf_attn_h_bwd_reduce + sgf_attn_h_bwd_apply remain for everything else; these three calls and the query reject
 * SGF_F32_BF16X3. */
int32_t sgf_attn_h_bwd_split_supported(int32_t d, int32_t dtype);
int sgf_attn_h_bwd_pre(const void* g, int64_t ldg, const void* o, int64_t ldo, const float* den, int64_t n, int32_t d,
                       int32_t dtype, const float* M, const float* w, void* workspace, size_t workspace_bytes,
                       float* rowscal, void* stream);
int sgf_attn_h_bwd_reduce_scaled(const void* h, int64_t ldh, const void* g, int64_t ldg, const float* rowscal, int64_t n,
                                 int32_t d, int32_t dtype, float* hstats, void* workspace, size_t workspace_bytes,
                                 void* stream);
int sgf_attn_h_bwd_post(const void* h, int64_t ldh, int64_t n, int32_t d, int32_t dtype, const float* D, const float* ds,
                        const void* workspace, size_t workspace_bytes, const void* addend, int64_t ldadd, void* dh,
                        int64_t lddh, void* stream);

/* The d x d algebra between the two node passes, as ONE entry each way (csrc/attn_small.hip; r05 — r04 issued it from
 * Python as 12 + 20 ATen / rocBLAS launches).  Replaces the small dense part of large/ours.py:123-149 with the projections
 * folded in (formulas above), written on augmented operands:
 *   sgf_attn_h_small_fwd : (G [d_in, d_in], s [d_in], n_rows, n_total, wq / wk / wv [d_out, d_in] with leading dim ldw,
 *                           bq / bk / bv [d_out]; wv = NULL: V is h itself, use_weight=False, needs d_in == d_out)
 *                          -> M [d_in, d_out] (ldm), m [d_out], w [d_in], beta [1]   — the operands of sgf_attn_h_fwd;
 *                          `saved` (sgf_attn_h_small_saved_bytes, caller-owned, opaque) keeps what the backward needs.
 *                          6 launches: pack, 3 products on the exact-fp32 matrix cores (csrc/gemm.hip), ||Q||^2 / ||K||^2
 *                          (one block, fixed summation order), scale + unpack.
 *   sgf_attn_h_small_bwd : (dM [d_in, d_out] (lddm), dw [d_in], dm [d_out], dbeta [1] = the blocks of hstats, after the
 *                          ranks' all-reduce) -> dG2 = dG + dG^T [d_in, d_in] (lddg) and ds [d_in] — the D / ds operands
 *                          of sgf_attn_h_bwd_post / _apply — and the six parameter gradients gwq / gwk / gwv [d_out, d_in]
 *                          (ldgw), gbq / gbk / gbv [d_out] (any of them NULL to skip).  9 launches; workspace:
 *                          sgf_attn_h_small_workspace_bytes.
 * n_rows = the number of rows behind G and s (global count when sharded); n_total = the N of large/ours.py:133.
 * Everything fp32 and on the device: no host synchronisation, no host read of ||Q|| or ||K||. */
size_t sgf_attn_h_small_saved_bytes(int32_t d_in, int32_t d_out);
size_t sgf_attn_h_small_workspace_bytes(int32_t d_in, int32_t d_out);
int sgf_attn_h_small_fwd(const float* G, int64_t ldg, const float* s, float n_rows, float n_total, const float* wq,
                         const float* bq, const float* wk, const float* bk, const float* wv, const float* bv, int64_t ldw,
                         int32_t d_in, int32_t d_out, float* M, int64_t ldm, float* m, float* w, float* beta, void* saved,
                         size_t saved_bytes, void* stream);
int sgf_attn_h_small_bwd(const float* dM, int64_t lddm, const float* dw, const float* dm, const float* dbeta, float n_total,
                         int32_t d_in, int32_t d_out, const void* saved, size_t saved_bytes, float* dG2, int64_t lddg,
                         float* ds, float* gwq, float* gbq, float* gwk, float* gbk, float* gwv, float* gbv, int64_t ldgw,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * T4/T6/T7 — weight and bias gradients of the Linear layers.   Replaces what autograd does for
 * every nn.Linear on the path under loss.backward() (large/main.py:142): the projections
 * large/ours.py:123-126, the GraphConvLayer weight :36-40, the stems :77,:198 and the head :275:
 *     dW = dY^T X   ([N, m]^T [N, k] -> [m, k]),    db = sum_n dY[n, :]
 * i.e. a d x d <- [N x d]^T [N x d] contraction over ALL nodes: the same streaming skeleton as
 * sgf_attn_fwd_reduce (K^T V), on the bf16 matrix cores for SGF_BF16 and the exact-fp32 MFMA for
 * SGF_F32, fp32 accumulation, deterministic two-stage reduction.  hipBLASLt's kernels for this
 * shape ran at 0.7 TB/s (3.6 ms per call at ogbn-products scale, profiles/); this one is HBM-bound.
 *     c[i, j] = sum_n a[n, i] * b[n, j]       c: fp32 [m, k] row-major, leading dim ldc
 *     colsum_a[i] = sum_n a[n, i]             fp32 [m], optional (NULL to skip)
 * m, k multiples of 4 (any size: tiled in 256 x 256 blocks).  Node-sharded runs all-reduce c.
 * ------------------------------------------------------------------------------------------ */
size_t sgf_gram_workspace_bytes(int64_t n, int32_t m, int32_t k);
int sgf_gram(const void* a, int64_t lda, int32_t m, const void* b, int64_t ldb, int32_t k,
             int64_t n, int32_t dtype, float* c, int64_t ldc, float* colsum_a, void* workspace,
             size_t workspace_bytes, void* stream);
/* Two such products that share a — c1 = a^T b1, c2 = a^T b2 (dW of the two-operand Linear: a = dz, b1 = Ax, b2 = x0) — in ONE
 * paired launch (bf16 storage, m, k <= 256): workgroups b and b + 8 (one XCD) walk the same row tiles, a's second read is an
 * L2 hit.  Other shapes / fp32: two sgf_gram launches.  Same workspace as sgf_gram; colsum_a as there. */
int sgf_gram2(const void* a, int64_t lda, int32_t m, const void* b1, int64_t ldb1, const void* b2, int64_t ldb2, int32_t k,
              int64_t n, int32_t dtype, float* c1, int64_t ldc1, float* c2, int64_t ldc2, float* colsum_a, void* workspace,
              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * T5 — TransConv glue.   Replaces large/ours.py:198-202 and :210-216 (medium/ours.py:150-156,
 * 100M/ours.py:262-268):   y = [relu]( LayerNorm( a * x + b * res ) )   row-wise
 * (large: a = b = 1/2; medium / 100M: a = alpha, b = 1 - alpha; input stem: a = 1, res = NULL).
 * res NULL = no residual; gamma NULL = no LayerNorm (use_bn False; beta then ignored).
 * Saves mean / rstd per row (fp32 [n] each, may be NULL when gamma is NULL) for the backward.
 * d % 4 == 0, d <= 1024.
 * ------------------------------------------------------------------------------------------ */
int sgf_ln_fwd(const void* x, int64_t ldx, const void* res, int64_t ldr, float a, float b,
               const float* gamma, const float* beta, int32_t relu, float eps, int64_t n,
               int32_t d, int32_t dtype, void* y, int64_t ldy, float* mean, float* rstd,
               void* stream);

/* Backward: dz = dy masked by relu (y > 0);  LayerNorm backward to dpre;  dx = a * dpre,
 * dres = b * dpre (dres may be NULL);  dgamma / dbeta (fp32 [d], may be NULL when gamma is NULL)
 * are reduced deterministically through per-block partials in `workspace`. */
size_t sgf_ln_bwd_workspace_bytes(int64_t n, int32_t d);
int sgf_ln_bwd(const void* dy, int64_t lddy, const void* y, int64_t ldy, const void* x,
               int64_t ldx, const void* res, int64_t ldr, float a, float b, const float* gamma,
               int32_t relu, const float* mean, const float* rstd, int64_t n, int32_t d,
               int32_t dtype, void* dx, int64_t lddx, void* dres, int64_t lddres, float* dgamma,
               float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * T6 — GraphConv glue.   Replaces large/ours.py:77-81 and :87-93:
 *     y = [relu]( BatchNorm1d(x) ) [+ res]          (dropout, when p > 0, stays in the caller)
 * BatchNorm1d statistics in training mode are over ALL rows — a hidden global reduction — so the
 * op is split at the reduction, which is also where a node-sharded run all-reduces:
 *     sgf_colstats     : stats = [ sum_n (x[n,j]-shift[j]) | sum_n (x[n,j]-shift[j])^2 ]  fp32 [2*d]
 *                        (shift NULL = 0).  Two calls give a two-pass mean / variance.
 *     sgf_bn_apply     : y = [relu]((x - mean[j]) * rstd[j] * gamma[j] + beta[j]) [+ res]
 *     sgf_bn_bwd_stats : stats = [ sum_n dz[n,j] | sum_n dz[n,j] * xhat[n,j] ]   (= dbeta | dgamma)
 *                        dz = dy masked by the recomputed relu, xhat = (x - mean) * rstd
 *     sgf_bn_bwd_apply : dx = gamma*rstd * (dz - [training](stats0*inv_n + xhat*stats1*inv_n))
 * The residual gradient is dy itself.  gamma / beta NULL = 1 / 0.  d % 4 == 0, d <= 1024.
 * ------------------------------------------------------------------------------------------ */
size_t sgf_colstats_workspace_bytes(int64_t n, int32_t d);
int sgf_colstats(const void* x, int64_t ldx, const float* shift, int64_t n, int32_t d,
                 int32_t dtype, float* stats, void* workspace, size_t workspace_bytes,
                 void* stream);
/* BatchNorm's bookkeeping between its statistics pass and its apply pass, one launch: from the shifted column sums
 * sums = [sum (x - shift) | sum (x - shift)^2] over n_total rows (shift may be null):  mean, rstd = 1 / sqrt(var + eps) with
 * the biased variance, and — when the pointers are given — nn.BatchNorm1d's running update
 *   running_mean = (1 - momentum) running_mean + momentum mean,  running_var likewise with the UNBIASED variance. */
int sgf_bn_finalize(const float* sums, const float* shift, double n_total, float eps, float momentum, float* running_mean,
                    float* running_var, int32_t d, float* mean, float* rstd, void* stream);
int sgf_bn_apply(const void* x, int64_t ldx, const float* mean, const float* rstd,
                 const float* gamma, const float* beta, const void* res, int64_t ldr,
                 int32_t relu, int64_t n, int32_t d, int32_t dtype, void* y, int64_t ldy,
                 void* stream);
/* sgf_bn_apply that ALSO writes every row of y in the packed form sgf_spmm_packed gathers (format above; bf16, d = 256,
 * rows 16-byte aligned, `packed` 128-byte aligned with sgf_spmm_packed_bytes(n, slot_bytes) bytes): y is sgf_bn_apply's bit
 * for bit.  *overflow (device int32) = the number of rows with more non-zeros than a slot holds (an integer count: exact,
 * order-independent); such a row's slot holds the values that fit and is never decoded. */
int sgf_bn_apply_packed(const void* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma,
                        const float* beta, const void* res, int64_t ldr, int32_t relu, int64_t n, int32_t d, int32_t dtype,
                        void* y, int64_t ldy, void* packed, int32_t slot_bytes, int32_t* overflow, void* stream);
int sgf_bn_bwd_stats(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, int32_t relu,
                     int64_t n, int32_t d, int32_t dtype, float* stats, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same sums for a tensor with TWO incoming gradients (dy + dy2, added in fp32; dy2 may be null): the stem's output feeds
 * the first SpMM and the layers' residuals / Linear blocks, whose gradients arrive separately. */
int sgf_bn_bwd_stats2(const void* dy, int64_t lddy, const void* dy2, int64_t lddy2, const void* x, int64_t ldx,
                      const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t relu, int64_t n,
                      int32_t d, int32_t dtype, float* stats, void* workspace, size_t workspace_bytes, void* stream);
/* dW / db of a Linear whose output z feeds a BatchNorm, without a materialised dz (the stem of GraphConv, large/ours.py:77-81:
 * its input is data, nobody else needs dz):  c[m, k] = dz^T b,  colsum[m] = sum_n dz,  where
 * dz = sgf_bn_bwd_apply(g1 [+ g2], z, ...) is formed per 4 x 4 patch inside the Gram kernel's staging step (bf16 storage, m and
 * k multiples of 4 up to 256).  stats as returned by sgf_bn_bwd_stats2; workspace: sgf_gram_workspace_bytes. */
/* The LayerNorm form (TransConv's stem, large/ours.py:198-201: Linear -> LayerNorm -> relu, input = data): from g = d(output),
 * the LayerNorm's input xin and the forward's per-row mean / rstd:
 *   c[m, k] = dl^T b, colsum[m] = sum_n dl (the Linear's dW / db), dgamma[m] = sum g' xhat, dbeta[m] = sum g' (the LayerNorm's),
 * dl = sgf_ln_bwd's input gradient, formed per 4 x 4 patch inside the Gram kernel (row means over the m columns across the
 * lanes of a patch row) and never written.  bf16 storage, m in {64, 128, 256}, k % 4 == 0 up to 256.  gamma / beta null: a
 * LayerNorm without affine terms (NOT sgf_ln_fwd's "no LayerNorm"); dgamma / dbeta may be null.  workspace:
 * sgf_gram_workspace_bytes. */
int32_t sgf_gram_ln_bwd_supported(int32_t m, int32_t k, int32_t dtype);
int sgf_gram_ln_bwd(const void* g, int64_t ldg, const void* xin, int64_t ldx, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, int32_t relu, int32_t m, const void* b, int64_t ldb, int32_t k,
                    int64_t n, int32_t dtype, float* c, int64_t ldc, float* colsum, float* dgamma, float* dbeta, void* workspace,
                    size_t workspace_bytes, void* stream);
int32_t sgf_gram_bn_bwd_supported(int32_t m, int32_t k, int32_t dtype);
int sgf_gram_bn_bwd(const void* g1, int64_t ldg1, const void* g2, int64_t ldg2, const void* z, int64_t ldz, const float* mean,
                    const float* rstd, const float* gamma, const float* beta, int32_t relu, const float* stats, float inv_n,
                    int32_t training, int32_t m, const void* b, int64_t ldb, int32_t k, int64_t n, int32_t dtype, float* c,
                    int64_t ldc, float* colsum, void* workspace, size_t workspace_bytes, void* stream);
/* A GraphConv layer's BatchNorm backward AND both blocks of its weight gradient in ONE pass over (g, z) (large/ours.py:36-40,
 * 87-93 differentiated; replaces sgf_bn_bwd_apply + sgf_gram2 — five [n, d] tensors of traffic instead of six):
 *   dz[n, m] = sgf_bn_bwd_apply(g, z, ...)  (written: sgf_gcn_epilogue_dx2_acc reads it next),
 *   c1[m, k] = dz^T b1, c2[m, k] = dz^T b2, colsum[m] = sum_n dz   (b1 = A x, b2 = x0: dW of W [A x | x0], db).
 * bf16 storage, m, k multiples of 8 up to 256, n >= 16384, every tensor operand 16-byte aligned with ld % 8 == 0
 * (sgf_gram2_bn_bwd_supported checks the sizes; a misaligned operand is SGF_E_INVALID).  workspace: sgf_gram_workspace_bytes. */
int32_t sgf_gram2_bn_bwd_supported(int32_t m, int32_t k, int64_t n, int32_t dtype);
int sgf_gram2_bn_bwd(const void* g, int64_t ldg, const void* z, int64_t ldz, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, int32_t relu, const float* stats, float inv_n, int32_t training,
                     int32_t m, const void* b1, int64_t ldb1, const void* b2, int64_t ldb2, int32_t k, int64_t n, int32_t dtype,
                     void* dz, int64_t lddz, float* c1, int64_t ldc1, float* c2, int64_t ldc2, float* colsum, void* workspace,
                     size_t workspace_bytes, void* stream);
int sgf_bn_bwd_apply(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, int32_t relu,
                     const float* stats, float inv_n, int32_t training, int64_t n, int32_t d,
                     int32_t dtype, void* dx, int64_t lddx, void* stream);

/* ------------------------------------------------------------------------------------------
 * T7 — branch combine + output layer, fused (the "residual + MLP" kernel).   Replaces
 * large/ours.py:269-270,275 (aggregate == 'add'):
 *     x = graph_weight * x2 + (1 - graph_weight) * x1;   logits = fc(x) = x W^T + bias
 *   sgf_combine_fc_fwd : logits[n, classes] (fp32, leading dim ldl) = (a x1 + b x2) W^T + bias in ONE pass
 *                        over x1, x2 — the combined activations are rounded to the storage dtype once (where
 *                        the unfused axpby rounds them) and fed to the bf16 matrix cores, never written.
 *   sgf_combine_fc_bwd : dx1 = a (dlogits W), dx2 = b (dlogits W), storage dtype, one pass over dlogits
 *                        (fp32 [n, classes], leading dim lddl; rounded to the storage dtype in registers).
 *   dW = a dlogits^T x1 + b dlogits^T x2 and db are node reductions: sgf_gram.
 * W: fp32 [classes, d] row-major, bias fp32 [classes].  Implemented for bf16 storage, d % 32 == 0,
 * d <= 256, classes <= 64 (sgf_combine_fc_supported); anything else: sgf_axpby + a library GEMM.
 * bf16 storage, backward: n < 2^31 (SGF_E_UNSUPPORTED beyond).
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_combine_fc_supported(int32_t d, int32_t classes, int32_t dtype);
int sgf_combine_fc_fwd(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b,
                       const float* w, const float* bias, int64_t n, int32_t d, int32_t classes,
                       int32_t dtype, float* logits, int64_t ldl, void* stream);
int sgf_combine_fc_bwd(const float* dlogits, int64_t lddl, const float* w, int64_t n, int32_t d,
                       int32_t classes, float a, float b, int32_t dtype, void* dx1, int64_t ld1, void* dx2,
                       int64_t ld2, void* stream);
/* The same pair with the module's row permutation folded in (bf16 storage, classes <= 64): on a graph the library has
 * re-ordered (sgf_reorder) the model works on permuted rows and its logits must go back to the caller's order
 * (sgformer_amd/ours.py; large/ours.py:275 returns them in the order of x).  _fwd_mapped stores row j of the product as row
 * row_map[j] of `logits`; _bwd_mapped reads row row_map[j] of `dlogits` for row j of dx1 / dx2.  row_map: int32[n], a
 * permutation of [0, n).  Saves the two [N, C] fp32 gather passes around the head. */
int sgf_combine_fc_fwd_mapped(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b, const float* w,
                              const float* bias, int64_t n, int32_t d, int32_t classes, int32_t dtype, float* logits,
                              int64_t ldl, const int32_t* row_map, void* stream);
int sgf_combine_fc_bwd_mapped(const float* dlogits, int64_t lddl, const float* w, int64_t n, int32_t d, int32_t classes,
                              float a, float b, int32_t dtype, void* dx1, int64_t ld1, void* dx2, int64_t ld2,
                              const int32_t* row_map, void* stream);
/* sgf_combine_fc_bwd / _bwd_mapped (row_map may be null) that also leaves the logits' gradient in the storage dtype:
 * g_out[n, 16 ceil(classes / 16)] bf16, zero-padded, in the module's row order (row j = row row_map[j] of dlogits) — the operand
 * of dW = a g^T x1 + b g^T x2 (sgf_gram) — written from the matrix-core fragments the kernel holds anyway instead of by a
 * cast and a pad pass over dlogits.  bf16 storage, classes <= 64; g_out 16-byte aligned, ldg % 8 == 0. */
int sgf_combine_fc_bwd_g(const float* dlogits, int64_t lddl, const float* w, int64_t n, int32_t d, int32_t classes, float a,
                         float b, int32_t dtype, void* dx1, int64_t ld1, void* dx2, int64_t ld2, const int32_t* row_map,
                         void* g_out, int64_t ldg, void* stream);

/* ------------------------------------------------------------------------------------------
 * T6 / K8 — the dense half of a GCN layer as one streaming pass.   Replaces, for large/ours.py:36-40,87-88
 *     x = self.W(gcn_conv(...));  x = self.bns[i](x)        (the Linear and BatchNorm1d's batch statistics)
 *   sgf_gcn_epilogue_stats : y[n, d_out] = a[n, d_in] W^T + bias, W [d_out, d_in] row-major in the storage
 *                            dtype, bias fp32 or null; fp32 accumulation on the matrix cores, y rounded to the
 *                            storage dtype.  With stats != null also, in the same pass,
 *                              stats[j] = sum_i (y_ij - shift_j),  stats[d_out + j] = sum_i (y_ij - shift_j)^2
 *                            of the ROUNDED y (what sgf_colstats(y, shift) returns, without re-reading y);
 *                            shift fp32 [d_out] or null.  workspace: sgf_gcn_epilogue_workspace_bytes (only
 *                            used with stats).  The normalise / ReLU / dropout / residual half of the layer
 *                            is sgf_bn_apply (+ sgf_dropout_*).
 *   sgf_gcn_epilogue_dx    : dx[n, d_in] = dy[n, d_out] W   (the Linear's input gradient; dW, db: sgf_gram).
 * W stays resident in LDS (one 8-wave block per CU), every wave streams 32-row tiles on its own; see
 * csrc/rowgemm.hip.  Implemented for bf16 storage and d_in == d_out in {64, 128, 256}
 * (sgf_gcn_epilogue_supported); rows of a / y / dy / dx / W must be 16-byte aligned.  Anything else: a
 * library GEMM + sgf_colstats.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_gcn_epilogue_supported(int32_t d_in, int32_t d_out, int32_t dtype);
size_t sgf_gcn_epilogue_workspace_bytes(int64_t n, int32_t d_out);
int sgf_gcn_epilogue_stats(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias,
                           int64_t n, int32_t d_in, int32_t d_out, int32_t dtype, void* y, int64_t ldy,
                           const float* shift, float* stats, void* workspace, size_t workspace_bytes,
                           void* stream);
/* Both input gradients of the two-operand Linear W [a1 | a2] (large/ours.py:36-38) from one read of dy out of HBM:
 * dx1 = dy w1, dx2 = dy w2 with w1 = W[:, :d], w2 = W[:, d:] (same leading dimension ldw).  pair != 0: ONE launch whose
 * workgroups come in pairs on one XCD walking the same row tiles (the second read of a tile is an L2 hit); pair = 0 or
 * fp32 storage: two sgf_gcn_epilogue_dx launches.  Results are identical either way. */
int sgf_gcn_epilogue_dx2(const void* dy, int64_t lddy, const void* w1, const void* w2, int64_t ldw, int64_t n, int32_t d,
                         int32_t dtype, void* dx1, int64_t lddx1, void* dx2, int64_t lddx2, int32_t pair, void* stream);

/* The same two gradients with the gradient of x0 = layer_[0] ACCUMULATED IN PLACE across the layers (large/ours.py:83-93: x0
 * feeds every layer's Linear and its residual; the layers' backward nodes run last-to-first):
 *     dy      = dz W[:, :d]
 *     acc_out = dz W[:, d:] + gadd + acc_in        gadd (nullable): this layer's residual gradient of x0;
 *                                                  acc_in (nullable): the running sum the layers before left
 * One launch, w = [W1 | W2] as the Linear stores it (ldw >= 2 d).  d = 256 runs as PAIRS of workgroups that each produce
 * half of the columns of BOTH results (balanced: the pair reads dz once through L2 and equal shares of the addends).  bf16
 * storage, d in {64, 128, 256}; acc_out may alias acc_in (same rows, same columns are read before they are written).
 * Replaces sgf_gcn_epilogue_dx2 + the final k-operand sgf_sum_n: 14 T instead of 16 T of traffic for three layers. */
int32_t sgf_gcn_epilogue_dx2_acc_supported(int32_t d, int32_t dtype);
int sgf_gcn_epilogue_dx2_acc(const void* dz, int64_t lddz, const void* w, int64_t ldw, int64_t n, int32_t d, int32_t dtype,
                             void* dy, int64_t lddy, const void* gadd, int64_t ldg, const void* acc_in, int64_t ldai,
                             void* acc_out, int64_t ldao, void* stream);
int sgf_gcn_epilogue_dx(const void* dy, int64_t lddy, const void* w, int64_t ldw, int64_t n, int32_t d_in,
                        int32_t d_out, int32_t dtype, void* dx, int64_t lddx, void* stream);
/* GraphConvLayer with use_init (large/ours.py:36-38):  y = [a1 | a2] W^T + bias,  W = [W1 | W2] of width 2 d.
 *   sgf_gcn_epilogue_partial   : partial = a1 W1^T + bias, rounded to the storage dtype and kept in the matrix
 *                                cores' accumulator layout (an opaque buffer of sgf_gcn_epilogue_partial_bytes,
 *                                16-byte aligned; lane-contiguous 16-byte stores, no transposition);
 *   sgf_gcn_epilogue_stats_add : y = a2 W2^T + partial (+ the column sums, as sgf_gcn_epilogue_stats) — the addend
 *                                returns to the registers it left from and the sum is rounded once: the arithmetic
 *                                of a library GEMM with beta = 1 on the rounded first product.
 * W1 / W2 are passed as pointers into W with ldw = 2 d.  5 [n, d] passes in total where
 * GEMM + GEMM(beta = 1) + sgf_colstats take 6. */
/* the other half of the layer (SURVEY.md §7 K8 "gcn_epilogue_apply"): BN normalise -> ReLU -> + residual, one
 * elementwise pass; the same entry as sgf_bn_apply under the name the layer-level API uses */
int sgf_gcn_epilogue_apply(const void* y, int64_t ldy, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, const void* res, int64_t ldr, int32_t relu, int64_t n, int32_t d,
                           int32_t dtype, void* out, int64_t ldo, void* stream);
/* Backward of the GCN layer's dense half in ONE launch (large/ours.py:36-40 + :87-93 differentiated; bf16 storage,
 * d in {64, 128, 256}).  Forward:  z = [Ax | x0] W^T + b,  out = [relu](BatchNorm(z)) [+ x0].  Given gy = d out, z, the
 * BatchNorm coefficients and the reduced statistics stats = [sum g' | sum g' xhat] of sgf_bn_bwd_stats:
 *     dz    = sgf_bn_bwd_apply(gy, z, ...)                 written row-major (the weight gradients read it: sgf_gram)
 *     dy    = dz W[:, :d]                                  gradient of Ax, row-major
 *     dx0'  = dx0 + dz W[:, d:] (+ gy when add_gy)         gradient of x0, ACCUMULATED over the layers of the branch:
 * acc_in (null for the first call) / acc_out are opaque buffers of sgf_gcn_epilogue_partial_bytes(n, d) holding the running
 * sum in the matrix cores' accumulator layout (bf16); the LAST call passes dx0 != null (and acc_out = null) and gets the
 * total row-major.  Exactly one of acc_out / dx0 is non-null.  gy and z leave HBM once: the workgroups that produce the
 * 2 d virtual output columns of one row tile (128 columns each) are launched 8 apart, i.e. on one XCD, and share the tiles
 * through its L2 (placement affects traffic only); with a workspace (sgf_gcn_bn_bwd_dx_workspace_bytes, may be null) those
 * workgroups meet once per tile — a bounded wait on device-scope counters, timing only — so that they stay inside the L2's
 * window.  inv_n = 1 / (global row count); training = 0: running statistics (no mean terms). */
int32_t sgf_gcn_bn_bwd_dx_supported(int32_t d, int32_t dtype);
size_t sgf_gcn_bn_bwd_dx_workspace_bytes(int64_t n, int32_t d);   /* arrival counters of the per-tile rendezvous (optional) */
int sgf_gcn_bn_bwd_dx(const void* gy, int64_t ldg, const void* z, int64_t ldz, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int32_t relu, const float* stats, float inv_n,
                      int32_t training, const void* w, int64_t ldw, int64_t n, int32_t d, int32_t dtype, void* dz,
                      int64_t lddz, void* dy, int64_t lddy, const void* acc_in, void* acc_out, size_t acc_bytes,
                      void* dx0, int64_t lddx0, int32_t add_gy, void* workspace, size_t workspace_bytes, void* stream);
/* The same two-operand Linear in ONE pass over a1 and a2 (bf16 storage, d = d_in = d_out in {64, 128, 256}; W [d, 2 d]):
 *   y = [a1 | a2] W^T + bias  [+ stats, as sgf_gcn_epilogue_stats].   d <= 128: W (64 KiB) is resident in LDS whole.
 *   d = 256: W is 256 KiB, more than a CU's LDS, so the launch is PAIRED — workgroups b and b + 8 (one XCD) walk the same
 *   row tiles, each producing one half of the output columns from its 128 rows of W; the second read of a tile is served
 *   by the XCD's L2.  Placement and timing affect only the traffic, never the result.  Rounding: the sum of both products
 *   is rounded ONCE (sgf_gcn_epilogue_partial / _stats_add round the first product to the storage dtype first).
 * workspace: sgf_gcn_epilogue_workspace_bytes(n, d), only when stats != null. */
int32_t sgf_gcn_epilogue_cat_supported(int32_t d, int32_t dtype);
int sgf_gcn_epilogue_cat(const void* a1, int64_t lda1, const void* a2, int64_t lda2, const void* w, int64_t ldw,
                         const float* bias, int64_t n, int32_t d, int32_t dtype, void* y, int64_t ldy, const float* shift,
                         float* stats, void* workspace, size_t workspace_bytes, void* stream);
size_t sgf_gcn_epilogue_partial_bytes(int64_t n, int32_t d_out);
size_t sgf_gcn_epilogue_dtype_partial_bytes(int64_t n, int32_t d_out, int32_t dtype);   /* fp32 storage: n * d_out * 4 */
int sgf_gcn_epilogue_partial(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, int64_t n,
                             int32_t d_in, int32_t d_out, int32_t dtype, void* partial, size_t partial_bytes,
                             void* stream);
int sgf_gcn_epilogue_stats_add(const void* a, int64_t lda, const void* w, int64_t ldw, const void* partial,
                               size_t partial_bytes, int64_t n, int32_t d_in, int32_t d_out, int32_t dtype,
                               void* y, int64_t ldy, const float* shift, float* stats, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * T4 / K10 — both input stems from ONE read of the node features.   Replaces the first line of each branch,
 * large/ours.py:77 (GraphConv: x = self.fcs[0](x), followed by BatchNorm1d :79) and :198 (TransConv):
 *     y0 = x W0^T + b0  [+ stats0 = column sums of the rounded y0, as sgf_gcn_epilogue_stats],   y1 = x W1^T + b1
 * x [n, d_in] in the storage dtype with d_in % 4 == 0, d_in <= 128 (rows 8-byte aligned: 100 features = 200 bytes);
 * W0, W1 [d_out, d_in] in the storage dtype, biases fp32 or null; w1 / y1 null = one output.  Same per-wave
 * streaming skeleton as sgf_gcn_epilogue_stats with both weight matrices resident in LDS (csrc/rowgemm.hip).
 * bf16 storage, d_out in {64, 128, 256} (sgf_stem_pair_supported); workspace (with stats0 only):
 * sgf_gcn_epilogue_workspace_bytes(n, d_out).
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_stem_pair_supported(int32_t d_in, int32_t d_out, int32_t dtype);
/* Geometry of the persistent bf16 row kernels behind the T4 / T6 / T7 entries (host query, no GPU needed).  Every wave of a
 * launch streams 32-row tiles t, t + waves, ...; the result is the number of rows ONE lap of all waves covers when the grid
 * is at its cap: virtual blocks (the groups of 1, 2 or 4 workgroups that walk the same tiles) x waves per block x 32.  A
 * launch over more than k times that many rows gives every wave more than k tiles.  kind, one per launch geometry:
 *   0 sgf_gcn_epilogue_stats / _dx / _partial / _stats_add      4 sgf_gcn_epilogue_cat
 *   1 sgf_gcn_epilogue_dx2 with pair != 0                       5 sgf_stem_pair (d = d_out)
 *   2 sgf_gcn_epilogue_dx2_acc                                  6 sgf_combine_fc_fwd / _fwd_mapped
 *   3 sgf_gcn_bn_bwd_dx                                         7 sgf_combine_fc_bwd / _bwd_mapped / _bwd_g
 * d in {64, 128, 256} (kinds 6, 7: d % 32 == 0, d <= 256, at most 64 classes), dtype SGF_BF16; -1 for anything else (fp32
 * storage runs other kernels: csrc/linear_f32.hip).  The entries size their grids with the functions this reads. */
int32_t sgf_row_lap_rows(int32_t kind, int32_t d, int32_t dtype);
int sgf_stem_pair(const void* x, int64_t ldx, int64_t n, int32_t d_in, const void* w0, int64_t ldw0,
                  const float* bias0, const void* w1, int64_t ldw1, const float* bias1, int32_t d_out, int32_t dtype,
                  void* y0, int64_t ldy0, void* y1, int64_t ldy1, const float* shift0, float* stats0, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * T4 — the general Linear: every shape the streaming kernels above do not take (csrc/gemm.hip; r05).   Replaces
 * F.linear / addmm / matmul for large/ours.py:77,:198 with input widths such as f = 1433 (Cora, medium/ours.py:133-145) or
 * widths that are not multiples of 4, the multi-head projections :123-126, medium/models.py GCNConv's x @ weight, the dX of
 * any of them — no Linear of the path leaves this library, whatever its shape:
 *     c[i, j] = alpha * sum_k A(i, k) B(k, j) + bias[j] + beta * addend[i, j]          i < m, j < n
 *     A(i, k) = a[i * a_rs + k * a_cs],   B(k, j) = b[k * b_rs + j * b_cs]             (element strides: any transposition)
 * y = x W^T + b : a = x (a_rs = ldx, a_cs = 1), b = W (b_rs = 1, b_cs = ldw);   dx = g W : b = W (b_rs = ldw, b_cs = 1).
 * Any m, n, k, any alignment.  Both operands bf16: bf16 matrix cores (exact products, fp32 sums); otherwise the exact-fp32
 * matrix cores (a bf16 operand is widened).  alpha_dev (nullable): a DEVICE scalar multiplied into alpha; bias fp32 [n] or
 * NULL; addend [m, n] (ldadd, add_dtype) or NULL, may alias c.  64 x 64 output tile per workgroup; not split over k
 * (node reductions such as dW = g^T x belong on sgf_gram).
 * ------------------------------------------------------------------------------------------ */
int sgf_gemm(const void* a, int64_t a_rs, int64_t a_cs, int32_t a_dtype, const void* b, int64_t b_rs, int64_t b_cs,
             int32_t b_dtype, int64_t m, int32_t n, int64_t k, float alpha, const float* alpha_dev, const float* bias,
             float beta, const void* addend, int64_t ldadd, int32_t add_dtype, void* c, int64_t ldc, int32_t c_dtype,
             void* stream);

/* ------------------------------------------------------------------------------------------
 * T7 — branch combine alone.   large/ours.py:269-270:  y = gw * x2 + (1 - gw) * x1.
 * (generic axpby: y = a * x1 + b * x2; the 'cat' aggregate is a plain copy done by the caller.)
 * ------------------------------------------------------------------------------------------ */
int sgf_axpby(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b,
              int64_t n, int32_t d, int32_t dtype, void* y, int64_t ldy, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dropout.   Replaces F.dropout(x, p, training=True) at large/ours.py:81,92,202,216 (and the
 * residual add that follows it in GraphConv, :92-93):   y = x * keep / (1 - p) [+ res]
 * keep ~ Bernoulli(1 - p) is a pure function of (seed, logical element index row*d + col) —
 * Philox4x32-10 — so NO mask is stored: the backward is the same call on dL/dy with the same seed
 * and res = NULL.  (The RNG stream differs from ATen's, as the CPU and CUDA streams of the
 * reference differ from each other; parity with dropout on is statistical.)  d % 4 == 0.
 * ------------------------------------------------------------------------------------------ */
int sgf_dropout(const void* x, int64_t ldx, const void* res, int64_t ldr, float p, uint64_t seed,
                int64_t n, int32_t d, int32_t dtype, void* y, int64_t ldy, void* stream);

/* sgf_dropout with the seed in DEVICE memory: the kernel reads all 64 bits of *seed_slot when it RUNS (each thread once,
 * ahead of its loop), so a launch captured into a hipGraph draws a new mask on every replay once the slot has been
 * rewritten on the same stream.  For the same seed value the output is bit-identical to sgf_dropout's.  seed_slot:
 * non-null and 8-byte aligned when n > 0 (else SGF_E_INVALID); not read when n == 0. */
int sgf_dropout_dev(const void* x, int64_t ldx, const void* res, int64_t ldr, float p,
                    const uint64_t* seed_slot, int64_t n, int32_t d, int32_t dtype, void* y, int64_t ldy,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * N4 — the trainer's loss.   Replaces large/main.py:139-141
 *     out = F.log_softmax(out, dim=1);  loss = NLLLoss()(out[train_idx], label.squeeze(1)[train_idx])
 * (5 ATen kernels over [N, C] and [M, C] temporaries; its nll_loss forward / backward kernels alone
 * cost 4.2 ms per step at ogbn-products scale) as one pass over the M training rows:
 *     sgf_nll_fwd : loss_sum[0] = - sum_j log_softmax(logits[idx[j]])[labels[idx[j]]]   (fp32; the
 *                   caller divides by M, or by the GLOBAL count when node-sharded)
 *     sgf_nll_bwd : dlogits = 0 everywhere except rows idx[j], where
 *                   dlogits = gout[0] * inv_denom * (softmax(logits[row]) - onehot(label))
 * logits / dlogits: [n, c] storage dtype with leading dims ldl / ldd; labels int64 [n] (indexed by
 * NODE id); idx int64 [m] distinct rows; gout fp32 [1] on the device.  Labels outside [0, c) add
 * nothing to the loss and get a zero gradient row (nn.NLLLoss's ignore_index).  Deterministic (per-block
 * partials, fixed-order sum).
 * ------------------------------------------------------------------------------------------ */
size_t sgf_nll_workspace_bytes(int64_t m);
int sgf_nll_fwd(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype,
                const int64_t* labels, const int64_t* idx, int64_t m, float* loss_sum,
                void* workspace, size_t workspace_bytes, void* stream);
int sgf_nll_bwd(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype,
                const int64_t* labels, const int64_t* idx, int64_t m, const float* gout,
                float inv_denom, void* dlogits, int64_t ldd, void* stream);

/* ------------------------------------------------------------------------------------------
 * N4b — the trainer's OTHER loss, for the multi-label / binary data sets (ogbn-proteins, deezer-europe, twitch-e, fb100,
 * yelp-chi).   Replaces large/main.py:130-137 (= large/main-batch.py:101-105, medium/main.py:158-166)
 *     loss = BCEWithLogitsLoss()(out[train_idx], true_label.squeeze(1)[train_idx].to(torch.float))
 * (a row-index kernel, a cast, the element-wise chain of binary_cross_entropy_with_logits, a mean, and in the backward an
 * index_put scatter back to [N, C]) as one pass over the M training rows:
 *     sgf_bce_fwd : loss_sum[0] = inv_denom * sum_j sum_k l(x[r_j, k], t[r_j, k]),
 *                   l(x, t) = max(x, 0) - x t + log1p(exp(-|x|)),   r_j = idx[j]
 *                   (fp32; the caller chooses the divisor: inv_denom = 1 / (M * C), 1 / (GLOBAL count * C) when
 *                   node-sharded, or 1 for the plain sum — one multiplication of the finished sum, no launch of its own)
 *     sgf_bce_bwd : dlogits = 0 everywhere except rows r_j, where
 *                   dlogits[r_j, k] = gout[0] * inv_denom * (sigmoid(x[r_j, k]) - t[r_j, k])
 * logits / dlogits: [n, c] in the storage dtype (SGF_F32 or SGF_BF16) with leading dims ldl / ldd, any c >= 1; all
 * arithmetic and the accumulation are fp32 (expf / log1pf, no fast intrinsics), the gradient is rounded once to the storage
 * dtype.  idx: int64 [m] distinct rows in [0, n); idx == NULL is the DENSE form, rows 0..m-1 with m == n (one streaming
 * pass; equal to the row form with idx = 0..n-1 bit for bit).  gout fp32 [1] on the device.
 * target is indexed by NODE id (as the labels of sgf_nll_*) and read as it is stored, without a cast pass:
 *     SGF_BCE_TARGET_F32   : fp32  [n, c], leading dim ldt; soft targets allowed
 *     SGF_BCE_TARGET_I64   : int64 [n, c] of 0 / 1, leading dim ldt (F.one_hot's result, the ogbn-proteins labels)
 *     SGF_BCE_TARGET_CLASS : int64 [n] class indices, the one-hot row formed on the fly (ldt is ignored).  An index outside
 *                            [0, c) matches no column: that row's target is all zero.  The index is only compared, never
 *                            used as an address, and nothing is validated on the host.
 * 16-byte accesses when c % 4 == 0 and every operand's rows start on a 4-element boundary; one element per lane otherwise.
 * Deterministic (fixed per-thread order, fixed block tree, fixed-order sum of the per-block partials).
 * ------------------------------------------------------------------------------------------ */
#define SGF_BCE_TARGET_F32 0
#define SGF_BCE_TARGET_I64 1
#define SGF_BCE_TARGET_CLASS 2
size_t sgf_bce_workspace_bytes(int64_t m, int32_t c);
int sgf_bce_fwd(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* target,
                int64_t ldt, int32_t target_kind, const int64_t* idx, int64_t m, float inv_denom,
                float* loss_sum, void* workspace, size_t workspace_bytes, void* stream);
int sgf_bce_bwd(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* target,
                int64_t ldt, int32_t target_kind, const int64_t* idx, int64_t m, const float* gout,
                float inv_denom, void* dlogits, int64_t ldd, void* stream);

/* ------------------------------------------------------------------------------------------
 * N5 — the trainers' evaluation metrics.   Replaces large/data_utils.py:199-246 (the same functions in medium/ and 100M/):
 *     eval_rocauc : per label column a device->host copy of [m] scores and labels and one scikit-learn roc_auc_score
 *                   (a host sort) — 336 host sorts per evaluation of ogbn-proteins (112 columns, three splits)
 *     eval_acc / eval_f1 : argmax, device->host copy, numpy compare
 * Both entries return INTEGER counts on the device; the host finishes the metric with one division per column.  Every
 * result is exact and bit-reproducible whatever the launch geometry.  No hidden allocation, no host sync.
 *
 * sgf_rocauc_counts : counts int64 [c, 6]; for column k, over the selected rows r_j = idx[j] (idx == NULL: rows 0..m-1,
 *   m == n):
 *     [0] P           rows with label == 1
 *     [1] Nn          rows with label == 0
 *     [2] U2          sum over positive i of ( 2 #{negative j : s_j < s_i} + #{negative j : s_j == s_i} )
 *     [3] other       labelled rows whose label is neither 0 nor 1
 *     [4] nan_scores  labelled rows whose score is NaN
 *     [5] unlabelled  rows whose label is NaN (SGF_METRIC_TARGET_F32 only)
 *   AUC_k = U2 / (2 P Nn): scikit-learn's trapezoid AUC with ties counted half (Mann-Whitney).  Rows counted under [3], [4]
 *   or [5] do not enter P, Nn or U2 (a row can count under both [3] and [4]).  Scores compare as fp32 values: bf16 is
 *   widened exactly, -0.0 == +0.0, +-inf are ordinary values.  m < 2^31 (so U2 < 2^62), c < 2^27.
 *   logits [n, c] SGF_F32 or SGF_BF16, leading dim ldl; target [n, c] indexed by NODE id, leading dim ldt:
 *     SGF_METRIC_TARGET_F32 : fp32 (NaN = unlabelled)        SGF_METRIC_TARGET_I64 : int64
 *   idx int64 [m] rows in [0, n); an entry outside that range is not read and counts under [3] in every column.
 *   Work: one key pass, one radix sort of m * c 64-bit keys (column in the top bits: a single long column is sorted by
 *   the whole chip), one rank pass.  Workspace: sgf_rocauc_workspace_bytes(m, c) — two key buffers of 8 m c bytes
 *   and the sort's temporary of about as much again, some 24 m c bytes in all (0: the size query failed, sgf_last_error() says why).
 *
 * sgf_argmax_count : counts int64 [2] = { labelled rows, rows whose argmax equals the label } over the selected rows, one
 *   pass, no [m, c] copy and no [m] prediction tensor.  argmax as torch.argmax on the CPU: the first maximal column; a NaN
 *   counts as the maximum and the first NaN wins.  labels: one per NODE, element r at labels[r * label_stride] (the
 *   trainers keep [N, 1]); label_kind SGF_METRIC_TARGET_I64 (every row labelled) or SGF_METRIC_TARGET_F32 (NaN =
 *   unlabelled; equal when float(argmax) == label).  An idx entry outside [0, n) is not read and not counted.
 *   Per-block integer partials summed in a fixed order.  Workspace: sgf_argmax_workspace_bytes(m, c).
 * ------------------------------------------------------------------------------------------ */
#define SGF_METRIC_TARGET_F32 0
#define SGF_METRIC_TARGET_I64 1
size_t sgf_rocauc_workspace_bytes(int64_t m, int32_t c);
int sgf_rocauc_counts(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* target,
                      int64_t ldt, int32_t target_kind, const int64_t* idx, int64_t m, int64_t* counts,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t sgf_argmax_workspace_bytes(int64_t m, int32_t c);
int sgf_argmax_count(const void* logits, int64_t ldl, int64_t n, int32_t c, int32_t dtype, const void* labels,
                     int64_t label_stride, int32_t label_kind, const int64_t* idx, int64_t m, int64_t* counts,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N6 — the head, its loss and their gradient on the SEED rows of a neighbour-sampled batch.   Replaces 100M/nb-sample.py:29
 * and :41 around 100M/ours.py's last two lines
 *     output = model(graph.x, graph.edge_index)[:batch_size];  loss = nn.CrossEntropyLoss()(output, graph.y[:batch_size])
 * which compute, store and differentiate all n rows of the logits to read m of them (1 000 of 756 000 for fan-outs
 * [15, 10, 5]).  Selected rows r_j, j < m: the PREFIX 0..m-1 when idx == NULL, else idx int64 [m], distinct, in [0, n)
 * (the convention of sgf_nll_* / sgf_bce_*; an entry outside [0, n) is clamped into it, never used as it is).
 *
 * sgf_head_rows_fwd :  z_j = round_to_storage(a x1[r_j] + b x2[r_j])      (x2 == NULL: z_j = round(a x1[r_j]))
 *                      logits[j] = z_j W^T + bias                          fp32 [m, classes] COMPACT, leading dim ldl
 *   x1 / x2 [n, d] in the storage dtype (leading dims ld1 / ld2, rows 16-byte aligned), w fp32 [classes, d] row-major,
 *   bias fp32 [classes].  z is rounded where the unfused sgf_axpby rounds it.  SGF_BF16: z and W (rounded to bf16 as
 *   sgf_combine_fc_fwd rounds it) on the bf16 matrix cores, fp32 accumulation.  SGF_F32: the fp32 operands as they are,
 *   whatever the matmul-precision setting, accumulated in fp64 and rounded to fp32 once (SGF_F32_BF16X3 is not accepted).  Shapes (sgf_head_rows_supported): d <= 256 with
 *   d % 32 == 0 (bf16) or d % 4 == 0 (fp32), any 1 <= classes <= 256 — ragged class counts are masked in the kernel, no
 *   padded copy of W or bias is made.
 *   labels != NULL (int64 [m], one per SELECTED row, compact): the same launch also leaves
 *       lse      fp32 [m]    log-sum-exp of every selected row
 *       loss_sum fp32 [1]    - sum_j (logits[j][labels[j]] - lse[j]) over the rows whose label is in [0, classes)
 *       counts   int64 [2]   { rows with a label in [0, classes); of those, rows whose first maximal column is the label }
 *   (argmax as sgf_argmax_count: first maximal column, a NaN is the maximum).  A label outside [0, classes) adds nothing,
 *   is not counted and gets a zero gradient row (nn.CrossEntropyLoss's ignore_index).  Deterministic: per-block partials
 *   in `workspace` (sgf_head_rows_fwd_workspace_bytes(m); not needed without labels), summed in a fixed order.
 *   m == 0: loss_sum = 0, counts = {0, 0}, no launch.
 *
 * sgf_head_rows_bwd :  the gradient g [m, classes] is the caller's (dlogits fp32 [m, classes], leading dim lddl; any
 *   loss on the m rows) or, with dlogits == NULL, formed in registers from the forward's logits / lse and the labels:
 *       g_j = gout[0] * inv_denom * (softmax(logits[j]) - onehot(labels[j]))       (gout fp32 [1] on the device)
 *   (the label's own entry as minus the sum of the row's other entries: no cancellation where its probability is near 1)
 *   Results:
 *       dx1[r_j] = a (g_j W), dx2[r_j] = b (g_j W), rounded once to the storage dtype; EVERY other row of dx1 / dx2
 *                  ([n, d], leading dims ldd1 / ldd2, rows 16-byte aligned) is written as exact zeros by the same call
 *                  (prefix form: one launch that also streams the zeros; idx form: a zero fill, then the row scatter).
 *                  dx2 == NULL exactly when x2 == NULL.
 *       dw fp32 [classes, d] = g^T z,  db fp32 [classes] = sum_j g_j — reduced over the m rows in fixed row slices added
 *                  in a fixed order; z is recomputed from the m rows of x1 / x2, nothing of size n is read.  g enters
 *                  this reduction in fp32; dX's product takes it as the forward takes z (bf16 on the matrix cores for
 *                  SGF_BF16 as sgf_combine_fc_bwd does, fp64-accumulated FMAs for SGF_F32).
 *   workspace: sgf_head_rows_bwd_workspace_bytes(m, d, classes).  m == 0: all-zero gradients.
 * Both entries need n < 2^31.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_head_rows_supported(int32_t d, int32_t classes, int32_t dtype);
size_t sgf_head_rows_fwd_workspace_bytes(int64_t m);
size_t sgf_head_rows_bwd_workspace_bytes(int64_t m, int32_t d, int32_t classes);
int sgf_head_rows_fwd(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b, const float* w,
                      const float* bias, int64_t n, int32_t d, int32_t classes, int32_t dtype, const int64_t* idx,
                      int64_t m, float* logits, int64_t ldl, const int64_t* labels, float* lse, float* loss_sum,
                      int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int sgf_head_rows_bwd(const void* x1, int64_t ld1, float a, const void* x2, int64_t ld2, float b, const float* w,
                      int64_t n, int32_t d, int32_t classes, int32_t dtype, const int64_t* idx, int64_t m,
                      const float* dlogits, int64_t lddl, const float* logits, int64_t ldl, const float* lse,
                      const int64_t* labels, const float* gout, float inv_denom, void* dx1, int64_t ldd1, void* dx2,
                      int64_t ldd2, float* dw, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N7 — DIFFormer's all-pair sigmoid attention (medium/difformer.py:41-52, kernel='sigmoid') as tiled products: no n x l
 * tensor is formed, the scores live in registers.  Per head, with z = q_i . k_j and S = sigmoid(z):
 *     r_i = sum_j S          out_i = sum_j S v_j / r_i                                   (sgf_pair_sigmoid_fwd)
 *     delta_i = g_i . out_i  dZ = S (1 - S) (g_i . v_j - delta_i) / r_i   dq_i = sum_j dZ k_j   (sgf_pair_sigmoid_bwd_q)
 *     dv_j = sum_i (S / r_i) g_i                                          dk_j = sum_i dZ q_i   (sgf_pair_sigmoid_bwd_kv)
 * Operands, row-major, leading dimensions in elements, rows 16-byte aligned: q / g / out / dq [n, heads * d], k / dk
 * [l, heads * d], v / dv [l, v_heads * d] with v_heads == heads, or v_heads == 1 for one value head that every head shares
 * (dv is then the sum over the heads, formed inside the kernel in head order); rowsum fp32 [n, heads] (= r).
 * Shapes (sgf_pair_sigmoid_supported): d in {32, 64, 128}, 1 <= heads <= 8, SGF_F32 or SGF_BF16; anything else, and
 * SGF_F32_BF16X3, is SGF_E_UNSUPPORTED (the split-bf16 products have entries of their own: N9).  n and l
 * are arbitrary (< 2^31); a key past l adds exactly 0 (it is masked, not zero-filled: sigmoid(0) = 0.5), rows past n are
 * never stored.  z >= 17 gives S = 1, z <= -104 gives S = 0, and 1 - S is formed from S: a saturated pair has an exactly
 * zero dZ.  No NaN comes out of the exponential's overflow.
 *   SGF_BF16: z and g . v on v_mfma_f32_32x32x16_bf16 with fp32 accumulators; the sigmoid, r, delta and 1 / r in fp32; S
 *     (fwd), S / r and dZ (bwd) are rounded to bf16 only as operands of the second products — rowsum is the fp32 sum of the
 *     unrounded S; out = sum_j S~ v_j / sum_j S~ with S~ the rounded S (a convex combination of the value rows), divided in
 *     fp32 and rounded once.
 *   SGF_F32: v_mfma_f32_32x32x2_f32, exact fp32 products; S and dZ are used as they are.
 * Every result is a fixed-order sum inside one workgroup: fwd / bwd_q keep 128 query rows resident and sweep the keys,
 * bwd_kv keeps 128 keys resident and sweeps the queries; both backward launches recompute S.  No atomics: bit-reproducible.
 * sgf_pair_sigmoid_bwd_q leaves delta fp32 [n, heads] in `workspace` (sgf_pair_sigmoid_workspace_bytes(n, l, heads) =
 * 4 n heads bytes), where sgf_pair_sigmoid_bwd_kv reads it: call bwd_q first (dq == NULL: delta only, no sweep).
 * Checks, all before the first HIP call: v_heads not in {1, heads}, a null pointer, l == 0 with n > 0, a leading dimension
 * below the operand's width or one that breaks the 16-byte row alignment: SGF_E_INVALID.  n == 0: SGF_OK, no launch,
 * nothing is written.
 * sgf_pair_sigmoid_lap_rows(which, ...) (which: 0 fwd, 1 bwd_q, 2 bwd_kv; the counterpart of sgf_row_lap_rows): the
 * smallest n (bwd_kv: l) at which every workgroup walks at least `laps` resident tiles; 0 = one tile per workgroup
 * (all three kernels today), -1 for an unsupported shape.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_pair_sigmoid_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype);
size_t sgf_pair_sigmoid_workspace_bytes(int64_t n, int64_t l, int32_t heads);
int64_t sgf_pair_sigmoid_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps);
int sgf_pair_sigmoid_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n,
                         int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* out, int64_t ldo,
                         float* rowsum, void* stream);
int sgf_pair_sigmoid_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* rowsum, const void* q,
                           int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                           int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* dq, int64_t lddq, void* workspace,
                           size_t workspace_bytes, void* stream);
int sgf_pair_sigmoid_bwd_kv(const void* g, int64_t ldg, const float* rowsum, const void* q, int64_t ldq, const void* k,
                            int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l, int32_t heads, int32_t v_heads,
                            int32_t d, int32_t dtype, void* dk, int64_t lddk, void* dv, int64_t lddv, const void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N8 — the exact softmax all-pair attention (medium/ablation/oursSOFT.py, the "is linear attention enough?" ablation) on
 * the skeleton of N7: no n x l tensor, the scores live in registers, with an online maximum.  Per head, with
 * z = scale q_i . k_j:
 *     m_i = max_j z   r_i = sum_j exp(z - m_i)   out_i = sum_j exp(z - m_i) v_j / r_i   lse_i = m_i + log r_i
 *                                                                                            (sgf_pair_softmax_fwd)
 *     P = exp(z - lse_i)   delta_i = g_i . out_i   dZ = scale P (g_i . v_j - delta_i)   dq_i = sum_j dZ k_j
 *                                                                                            (sgf_pair_softmax_bwd_q)
 *     dv_j = sum_i P g_i                                                 dk_j = sum_i dZ q_i   (sgf_pair_softmax_bwd_kv)
 * Operands, layouts, leading dimensions, the 16-byte row alignment, v_heads in {heads, 1} (dv summed over the heads inside
 * the kernel, in head order), the shapes (sgf_pair_softmax_supported: d in {32, 64, 128}, 1 <= heads <= 8, SGF_F32 or
 * SGF_BF16; SGF_F32_BF16X3 is SGF_E_UNSUPPORTED here: N9), the workspace (delta fp32 [n, heads], written by bwd_q — dq == NULL:
 * delta only — and read by bwd_kv), the checks and their order, and sgf_pair_softmax_lap_rows are those of N7.  The
 * differences: `lse` fp32 [n, heads] stands where `rowsum` stood, and `scale` (after dtype) multiplies the scores; it must
 * be finite and positive, else SGF_E_INVALID (checked after the shape, before the pointers and for an empty problem too).
 * Online update, fp32, per swept stage: m' = max(m, stage max), c = exp(m - m'), r = c r + sum P, acc = c acc + P V.  m
 * starts at -inf; the stage maximum is finite from the first stage on (the two lane halves exchange it before P is
 * formed), so exp(-inf - (-inf)) is never evaluated.  A key past l is masked to -inf before the maximum: it takes no part
 * in it and adds exactly 0 (zero-filling would score exp(0 - m)); rows past n are never stored.  z - m <= 0 always: for any
 * finite scores, |z| of several thousand included, nothing overflows and no NaN or inf comes out; pairs that underflow
 * contribute exactly 0.  The backward launches recompute P from lse and need no maximum.
 *   SGF_BF16: z and g . v on v_mfma_f32_32x32x16_bf16 with fp32 accumulators, exp by the hardware exp2; m, r, lse, delta and
 *     the rescale in fp32; P (fwd) and P, dZ (bwd) are rounded to bf16 only as operands of the second products — lse holds
 *     the fp32 sum of the unrounded P; out = sum_j P~ v_j / sum_j P~ with P~ the rounded P (a convex combination of the
 *     value rows), divided in fp32 and rounded once.
 *   SGF_F32: v_mfma_f32_32x32x2_f32, exact fp32 products, expf; P and dZ are used as they are.
 * Every result is a fixed-order sum inside one workgroup (128 resident rows, the other side swept): no atomics, nothing
 * summed across workgroups, bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_pair_softmax_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype);
size_t sgf_pair_softmax_workspace_bytes(int64_t n, int64_t l, int32_t heads);
int64_t sgf_pair_softmax_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps);
int sgf_pair_softmax_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n,
                         int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale, void* out,
                         int64_t ldo, float* lse, void* stream);
int sgf_pair_softmax_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* lse, const void* q,
                           int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                           int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale, void* dq, int64_t lddq,
                           void* workspace, size_t workspace_bytes, void* stream);
int sgf_pair_softmax_bwd_kv(const void* g, int64_t ldg, const float* lse, const void* q, int64_t ldq, const void* k,
                            int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l, int32_t heads, int32_t v_heads,
                            int32_t d, int32_t dtype, float scale, void* dk, int64_t lddk, void* dv, int64_t lddv,
                            const void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N9 — N7 and N8 for SGF_F32_BF16X3: fp32 storage, every matrix product (z, g . v, S V / P V, dZ K, dZ Q, W g) formed as
 * three bf16 matrix-core products.  Two families of five entries; each entry has the argument list of its N7 / N8
 * counterpart, `dtype` included, and computes the same formulas.  `dtype` must be SGF_F32_BF16X3: SGF_F32, SGF_BF16 and
 * anything else are SGF_E_UNSUPPORTED here, exactly as the N7 / N8 entries reject SGF_F32_BF16X3.  Shapes
 * (sgf_pair_*_x3_supported): d in {32, 64, 128}, 1 <= heads <= 8, v_heads in {1, heads}.  Pointers, leading dimensions,
 * the 16-byte row alignment (4 fp32), the checks and their order, and the workspace (sgf_pair_sigmoid_workspace_bytes /
 * sgf_pair_softmax_workspace_bytes: delta fp32 [n, heads]) are those of SGF_F32 in N7 / N8.
 *   While a swept tile is staged into LDS every element is split once, hi = bf16(a), lo = bf16(a - hi) (round to nearest
 *   even, lo = 0 where hi is not finite), into two bf16 images in the SGF_BF16 layouts; the resident rows are split the same
 *   way into two fragment sets, and the fp32 score tile (S, P, dZ, S / r) is split in registers as it becomes the operand
 *   of the second product.  Each product is hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_bf16 into one fp32 accumulator:
 *   at most 3 * 2^-16 |a| |b| per product.  Operands that bf16 holds exactly give the products of SGF_F32.
 *   expf, the online maximum and rescale, lse, delta = g . out, the row sums and the denominators are the fp32 code of
 *   SGF_F32; the sums are over the unrounded weights (out is divided by r itself, not by a sum of rounded weights as under
 *   SGF_BF16).  A score error dz moves a softmax weight by the factor exp(dz): |dz| <= 2^-14 scale |q| . |k|.
 * Fixed-order sums inside one workgroup, no atomics: bit-reproducible.  sgf_pair_*_x3_lap_rows: as in N7 (0: one resident
 * tile per workgroup), for dtype SGF_F32_BF16X3 only.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_pair_sigmoid_x3_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype);
int64_t sgf_pair_sigmoid_x3_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps);
int sgf_pair_sigmoid_x3_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n,
                            int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* out, int64_t ldo,
                            float* rowsum, void* stream);
int sgf_pair_sigmoid_x3_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* rowsum, const void* q,
                              int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                              int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, void* dq, int64_t lddq, void* workspace,
                              size_t workspace_bytes, void* stream);
int sgf_pair_sigmoid_x3_bwd_kv(const void* g, int64_t ldg, const float* rowsum, const void* q, int64_t ldq, const void* k,
                               int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l, int32_t heads, int32_t v_heads,
                               int32_t d, int32_t dtype, void* dk, int64_t lddk, void* dv, int64_t lddv, const void* workspace,
                               size_t workspace_bytes, void* stream);
int32_t sgf_pair_softmax_x3_supported(int32_t heads, int32_t v_heads, int32_t d, int32_t dtype);
int64_t sgf_pair_softmax_x3_lap_rows(int32_t which, int32_t heads, int32_t d, int32_t dtype, int32_t laps);
int sgf_pair_softmax_x3_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n,
                            int64_t l, int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale, void* out,
                            int64_t ldo, float* lse, void* stream);
int sgf_pair_softmax_x3_bwd_q(const void* g, int64_t ldg, const void* out, int64_t ldo, const float* lse, const void* q,
                              int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l,
                              int32_t heads, int32_t v_heads, int32_t d, int32_t dtype, float scale, void* dq, int64_t lddq,
                              void* workspace, size_t workspace_bytes, void* stream);
int sgf_pair_softmax_x3_bwd_kv(const void* g, int64_t ldg, const float* lse, const void* q, int64_t ldq, const void* k,
                               int64_t ldk, const void* v, int64_t ldv, int64_t n, int64_t l, int32_t heads, int32_t v_heads,
                               int32_t d, int32_t dtype, float scale, void* dk, int64_t lddk, void* dv, int64_t lddv,
                               const void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * N10 — attention over the stored entries of a CSR: torch_geometric 1.7.2 GATConv without an [E, H] or [E, H, C] tensor,
 * forward or backward (csrc/gat.hip).  H heads of C channels; xw [n_src, H * C] is the projected input, row-major with
 * leading dimension ldx.  Per head h, for entry e of target row i with source j = colind[e] (val is not read; parallel
 * entries each count):
 *     al[n, h] = <xw[n, h, :], att_l[h, :]>      ar likewise with att_r                                 (sgf_gat_scores)
 *     z_e = al[j, h] + ar[i, h]      s_e = z_e > 0 ? z_e : negative_slope z_e
 *     m = max_e s_e   l = sum_e exp(s_e - m)   p_e = exp(s_e - m) / l   lse = m + log l   norm = (m, 1 / l)
 *     p~_e = p_e keep_e / (1 - p_drop)      out[i, h, :] = sum_e p~_e xw[j, h, :]                          (sgf_gat_fwd)
 *   out is [n_rows, H * C], or with mean_heads != 0 the mean over the heads [n_rows, C]; `bias` (fp32, H * C or C values,
 *   may be NULL) is added last.  An empty row gives bias alone, lse = 0, norm = (0, 0), and nothing in the backward.  The
 *   entries of a row are walked once with an online maximum (a rise rescales l and the accumulators by exp(m - m')).
 *   With g_h = g[i, h, :] (mean_heads: g[i, :] / H for every head) and dp_e = <g_h, xw[j, h, :]>:
 *     delta[i, h] = sum_e p~_e dp_e
 *     dz_e = p_e (keep_e / (1 - p_drop) dp_e - delta[i, h]) sl_e            sl_e = z_e > 0 ? 1 : negative_slope
 *     dar[i, h] = sum_{e in row i} dz_e = B - delta S,  B = sum p~ dp sl,  S = sum p sl                (sgf_gat_bwd_dst)
 *     dal[j, h] = sum_{e: colind[e] = j} dz_e
 *     dxw[j, h, :] = sum_{e: colind[e] = j} p~_e g_h[i] + dal[j, h] att_l[h, :] + dar[j, h] att_r[h, :]  (sgf_gat_bwd_src)
 *   sgf_gat_bwd_src walks the TRANSPOSED CSR (row = source j, entries = its targets i; sgf_csr_transpose) and runs after
 *   sgf_gat_bwd_dst, whose delta and dar it reads; att_l / att_r may be NULL (no score term of that side; dar may then be
 *   NULL too), and the dar term is added for j < n_rows only (targets are the first n_rows sources).  Both backward
 *   launches recompute p_e = exp(s_e - m) / l from al, ar and norm: through the fp32 lse the weights of a row of 2^k equal
 *   scores would not come out as 2^-k.  al, ar, lse [., H], norm [n_rows, H, 2], delta, dar, dal are fp32; xw, g, out, dxw
 *   are fp32 or bf16 (dtype), accumulated in fp32 and rounded once.
 * Keep decisions (p_drop > 0): Philox4x32-10 with the round function and key schedule of sgf_dropout, key = seed, counter
 *   (i, j, 0x53474154, h / 4); head h reads word h % 4 and is kept when (word >> 8) 2^-24 >= p_drop.  The decision is a
 *   function of (target, source, head): the same in both orientations, and shared by parallel entries i <- j.
 * No atomics; every sum runs in stored order inside one group of lanes: bit-reproducible.  A row of any length is walked by
 *   its one group of lanes.
 * Shapes (sgf_gat_supported): 1 <= heads <= 8, c % 4 == 0, heads * c <= 1024, SGF_F32 or SGF_BF16; else SGF_E_UNSUPPORTED.
 * Checks, in this order, all before the first HIP call: negative sizes (SGF_E_INVALID); shape and dtype; more than 2^31 - 1
 *   rows (SGF_E_UNSUPPORTED); negative_slope finite and 0 <= p_drop <= 1 (SGF_E_INVALID); nothing to walk (n, n_rows or, for
 *   bwd_src, n_src == 0): SGF_OK; null pointers; a leading dimension below the width (H * C, or C for out / g under
 *   mean_heads); rows not aligned to what a lane moves (4 channels: pointers % 16 bytes for fp32, % 8 for bf16, leading
 *   dimensions % 4 elements); att_l / att_r / bias not 16-byte aligned.
 * sgf_gat_lap_rows: rows one lap of the capped grid of kernel `which` (0 scores, 1 fwd, 2 bwd_dst, 3 bwd_src) covers (a
 *   launch over more rows gives a workgroup several laps), -1 for a bad argument.  Host query, no GPU needed.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_gat_supported(int32_t heads, int32_t c, int32_t dtype);
int64_t sgf_gat_lap_rows(int32_t heads, int32_t c, int32_t dtype, int32_t which);
int sgf_gat_scores(const void* xw, int64_t ldx, const float* att_l, const float* att_r, int64_t n, int32_t heads, int32_t c,
                   int32_t dtype, float* al, float* ar, void* stream);
int sgf_gat_fwd(const int64_t* rowptr, const int32_t* colind, const void* xw, int64_t ldx, const float* al, const float* ar,
                const float* bias, int64_t n_rows, int64_t n_src, int32_t heads, int32_t c, int32_t dtype, int32_t mean_heads,
                float negative_slope, float p_drop, uint64_t seed, void* out, int64_t ldo, float* lse, float* norm,
                void* stream);
int sgf_gat_bwd_dst(const int64_t* rowptr, const int32_t* colind, const void* g, int64_t ldg, const void* xw, int64_t ldx,
                    const float* al, const float* ar, const float* norm, int64_t n_rows, int64_t n_src, int32_t heads,
                    int32_t c, int32_t dtype, int32_t mean_heads, float negative_slope, float p_drop, uint64_t seed,
                    float* delta, float* dar, void* stream);
int sgf_gat_bwd_src(const int64_t* t_rowptr, const int32_t* t_colind, const void* g, int64_t ldg, const void* xw, int64_t ldx,
                    const float* al, const float* ar, const float* norm, const float* delta, const float* dar,
                    const float* att_l, const float* att_r, int64_t n_rows, int64_t n_src, int32_t heads, int32_t c,
                    int32_t dtype, int32_t mean_heads, float negative_slope, float p_drop, uint64_t seed, float* dal, void* dxw,
                    int64_t lddx, void* stream);

/* y = sum_i xs[i] for 1 <= k <= 8 equally shaped [n, d] operands (fp32 accumulation in operand
 * order).  Replaces the pairwise gradient accumulation autograd performs for a tensor with several
 * consumers — GraphConv's x0 (large/ours.py:83-93) receives one gradient per layer from the
 * [. | x0] Linear, one per layer from the residual and one from the first SpMM.
 * xs / lds are HOST arrays of k device pointers / leading dimensions. */
int sgf_sum_n(const void* const* xs_host, const int64_t* lds_host, int32_t k, int64_t n, int32_t d,
              int32_t dtype, void* y, int64_t ldy, void* stream);

/* Column sum out[j] = sum_n x[n,j] for ANY 1 <= d <= 256 (no multiple-of-4 requirement): the bias
 * gradient of the output layer, large/ours.py:275 under autograd, where d = number of classes
 * (47 for ogbn-products).  fp32 result, deterministic two-stage reduction. */
size_t sgf_colsum_workspace_bytes(int64_t n, int32_t d);
int sgf_colsum(const void* x, int64_t ldx, int64_t n, int32_t d, int32_t dtype, float* out,
               void* workspace, size_t workspace_bytes, void* stream);

/* Geometry of the persistent element-wise, normalisation and loss kernels of csrc/fused.hip (host query, no GPU needed; the
 * counterpart of sgf_row_lap_rows).  Their grids are capped (8 workgroups of 256 threads per CU) and every workgroup walks
 * its rows in a loop; the result is the number of rows ONE loop iteration of the capped grid covers for the kernel the
 * entry would launch, so a launch over more than k times that many rows gives every workgroup more than k iterations.
 * kind:
 *    0 sgf_ln_fwd                           5 sgf_sum_n                          10 sgf_colstats / sgf_bn_bwd_stats / _stats2
 *    1 sgf_ln_bwd                           6 sgf_dropout / sgf_dropout_dev      11 sgf_colsum
 *    2 sgf_bn_apply                         7 sgf_gather_rows                    12 sgf_nll_fwd (d = c)
 *    3 sgf_bn_bwd_apply                     8 sgf_pad_rows (d = d_pad)
 *    4 sgf_axpby                            9 sgf_nll_bwd (d = c; TRAINING rows)
 * wide = 1 asks for the kernel that moves bf16 rows as 16 bytes per lane (kinds 0, 1: d in {64, 128, 256, 512}; 2, 3, 5, 10:
 * d % 8 == 0), which the entry launches when every row is 16-byte aligned (kinds 1, 2, 3, 10 also: unless SGF_EW8=0);
 * wide = 0 for the fp32 and the 8-byte bf16 kernels.
 *   - kinds 4 - 8 are flat: a thread takes one chunk of a row (4 columns; 8 when wide; kind 8 and kind 7 with d % 4 != 0: one
 *     element) and the grid strides over all chunks, so an iteration ends INSIDE a row when the chunks per row do not divide
 *     256 * grid; the result is the whole rows of one iteration, rounded down.
 *   - kinds 10 - 12 are blocked (workgroup b takes the rows [b r, (b + 1) r), r = ceil(n / grid)): the result is the row
 *     count at which the grid stops growing; beyond it r grows, and trailing workgroups may have no rows at all.
 * -1 for an unknown kind, a width or dtype the entry rejects (kinds 0 - 6, 10: d % 4 == 0, d <= 1024; 11: d <= 256; 7, 8: d <= 2^20), or a
 * wide form that does not exist.  The entries size their grids with the functions this reads. */
int64_t sgf_ew_lap_rows(int32_t kind, int32_t d, int32_t dtype, int32_t wide);

/* ------------------------------------------------------------------------------------------
 * SURVEY.md §8b / §8e — the collectives of the node-sharded run (csrc/comm.hip): thin wrappers over RCCL, which is loaded
 * with dlopen() at the first call (libsgf.so has no link-time dependency on librccl.so).  The reference has no multi-GPU
 * path; WHAT is exchanged follows from the kernels' partial-sum layouts above: the attention statistics and BatchNorm sums
 * and the parameter gradients (all-reduce, fp32, in place), the SpMM operand's rows — whole shards (all-gather) or the
 * cut-edge rows of a halo plan (all-to-all with per-peer byte ranges).  One process per GPU; the communicator is created
 * on the calling thread's CURRENT device.  The *_host arrays are host memory (per-peer offsets / sizes in bytes, length =
 * world); everything else is device memory.  The Python host side (sgformer_amd/dist.py) issues the same collectives
 * through torch.distributed (backend `nccl` = RCCL); these entries are for a consumer binding the library from C.
 *   sgf_comm_unique_id  : rank 0 fills id_host (sgf_comm_unique_id_bytes() = 128 bytes) and hands it to the other ranks
 *                         by any out-of-band means (the launcher's rendezvous);
 *   sgf_comm_create     : blocks until all `world` ranks have called it with the same id.
 * ------------------------------------------------------------------------------------------ */
int32_t sgf_comm_available(void);                 /* 1 if librccl.so and its entry points could be loaded */
int32_t sgf_comm_unique_id_bytes(void);
int sgf_comm_unique_id(void* id_host);
int sgf_comm_create(void** comm_out, int32_t world, int32_t rank, const void* id_host);
int sgf_comm_destroy(void* comm);
int sgf_comm_all_reduce_f32(void* comm, float* buf, int64_t count, void* stream);
int sgf_comm_all_gather(void* comm, const void* send, void* recv, int64_t bytes_per_rank, void* stream);
int sgf_comm_all_to_all(void* comm, const void* send, const int64_t* send_offset_host, const int64_t* send_bytes_host,
                        void* recv, const int64_t* recv_offset_host, const int64_t* recv_bytes_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGF_H_ */
